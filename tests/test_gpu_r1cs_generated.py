"""Generated R1CS gadgets on the GPU (tests/r1cs_corpus.py) against the twin, bit for bit: verification (verdict, transcript and the
32-byte mega-check), proving (proof bytes, commitments, transcripts), the batch-combined check over all named cases in ONE call, the
pool, and a sweep of further seeds.  The named cases reach challenge powers above 1, several challenges, the split power tables' and the
ONE chunks' boundaries and the edge shapes listed in test_r1cs_generated.py::test_named_cases_reach_the_listed_features."""
import hashlib
import threading

import pytest

import r1cs_corpus as G
import r1cs_rlc_twin as T
import r1cs_twin as R
from test_gpu_r1cs_rlc import _combined, _group, _per_proof, _twin

pytestmark = pytest.mark.gpu

CAP = 128
SWEEP = [G.sweep_case(s) for s in range(2000, 2064)]
_proofs = {}


@pytest.fixture(scope="module")
def gens(oracle):
    return oracle.Gens(CAP, 1).export()


@pytest.fixture(scope="module")
def ctx():
    import bulletproofs_amd as bp
    c = bp.Context(0)
    c.gens_create(CAP, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small_ctx():
    import bulletproofs_amd as bp
    c = bp.Context(0)
    c.gens_create(8, 1)
    yield c
    c.close()


def _rng(tag, nb):
    return hashlib.shake_256(b"generated-gpu-rng" + tag).digest(32 * nb)


def _valid(case, gens, idx=0, st0=None):
    """the twin's proof of the case (kept for the module): (proof, [V], twin prover)"""
    key = (case.name, case.seed, idx, st0)
    if key not in _proofs:
        _proofs[key] = G.twin_prove(case, gens, idx, st0)
    return _proofs[key]


def _partner(case):
    """a different circuit with the same m: the next named case that has it, else the same shape under the next seed"""
    i = G.SMALL.index(case)
    for c in G.SMALL[i + 1:] + G.SMALL[:i]:
        if c.m == case.m:
            return c
    return case.with_seed(case.seed + 1)


def _check(c, circuit, gadget, gens, cap, proofs, coms, st0s, rng32, shared):
    """verify on the GPU and with the twin; verdict, transcript, and the mega-check of every proof that reaches it.  Returns
    (verdicts, how many reached the mega-check)"""
    nb, m = len(proofs), circuit.m
    ts = st0s[0] if shared else b"".join(st0s)
    v, mc, tso = circuit.verify_batch(c, proofs, b"".join(coms), ts, rng32=rng32, want_msm=True, want_transcripts=True)
    reached = 0
    for b in range(nb):
        code, emc, ets = R.verify_with(gadget, gens, cap, st0s[b], proofs[b], [coms[b][32 * j:32 * j + 32] for j in range(m)], rng32[32 * b:32 * b + 32])
        assert v[b] == code, (b, v[b], code)
        assert tso[208 * b:208 * b + 208] == ets, b
        if emc is not None:
            reached += 1
            assert mc[32 * b:32 * b + 32] == emc, b
    return v, reached


def _verify_inputs(case, gens):
    """(proofs, commitments): the tampered variants, the other serialization when one-phase, another case's valid proof, the valid proof (last)"""
    pf, Vs, _ = _valid(case, gens)
    good = pf.to_bytes()
    cases = G.tamper_cases(good, Vs)
    if good[0] == 0:
        two = pf.to_bytes(force_two_phase=True)
        cases = G.tamper_cases(two, Vs)[:-1] + [(two, b"".join(Vs))] + cases
    other = _partner(case)
    opf, oVs, _ = _valid(other, gens)
    cases.insert(0, (opf.to_bytes(), b"".join(oVs)))
    return [p for p, _ in cases], [cm for _, cm in cases]


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "own"])
@pytest.mark.parametrize("case", G.SMALL, ids=[c.name for c in G.SMALL])
def test_verify_named_case(ctx, gens, case, shared):
    proofs, coms = _verify_inputs(case, gens)
    st0 = G.st0_of(case)
    if shared:
        st0s = [st0] * len(proofs)
    else:   # every other proof starts from a transcript with one message more (a failure for the valid ones)
        t1 = R.transcript_from_state(st0)
        t1.append_message(b"extra", b"message")
        st1 = R.transcript_state(t1)
        st0s = [st1 if (len(proofs) - 1 - i) % 2 else st0 for i in range(len(proofs))]
    circuit = G.record_verifier(case).circuit()
    v, reached = _check(ctx, circuit, G.verifier_gadget(case), gens, CAP, proofs, coms, st0s, _rng(case.name.encode(), len(proofs)), shared)
    assert v[-1] == 0 and reached >= 3 and set(v) >= {0, 1, 2}


@pytest.mark.parametrize("name", ["powers", "ch256"])
def test_too_few_generators_after_the_phase_2_challenges(small_ctx, gens, name):
    """padded_n = 32 on 8 generators: InvalidGeneratorsLength, the transcript as of the phase-2 challenge draws (3 and 256 of them)"""
    case = next(c for c in G.SMALL if c.name == name)
    proofs, coms = _verify_inputs(case, gens)
    circuit = G.record_verifier(case).circuit()
    assert circuit.padded_n == 32
    v, reached = _check(small_ctx, circuit, G.verifier_gadget(case), gens, 8, proofs, coms, [G.st0_of(case)] * len(proofs), _rng(b"short", len(proofs)), True)
    assert v[-1] == 4 and set(v) <= {1, 2, 4} and reached == 0


def _own_st0(case, b):
    return R.transcript_state(R.T.Transcript(b"generated gadget %d, proof %d" % (case.seed, b)))


def _prove_and_compare(c, case, gens, shared, nb=3):
    from bulletproofs_amd import r1cs
    st0s = [G.st0_of(case) if shared else _own_st0(case, b) for b in range(nb)]
    provers = [G.record_prover(case, b, st0s[b]) for b in range(nb)]
    rng32 = b"".join(G.rng32_of(case, b) for b in range(nb))
    ins = [p.inputs() for p in provers]
    circuit = provers[0].circuit()
    ts = st0s[0] if shared else b"".join(st0s)
    proofs, coms, status, tso = provers[0].witness().prove_batch(c, circuit, nb, b"".join(i[0] for i in ins), b"".join(i[1] for i in ins),
                                                                  b"".join(i[2] for i in ins), ts, rng32, want_transcripts=True)
    assert status == bytes(nb)
    m = case.m
    for b in range(nb):
        pf, Vs, twin = _valid(case, gens, b, None if shared else st0s[b])
        assert proofs[b] == pf.to_bytes(), (case, b)
        assert coms[32 * m * b:32 * m * (b + 1)] == b"".join(Vs), (case, b)
        assert tso[208 * b:208 * (b + 1)] == R.transcript_state(twin.t), (case, b)
    verdict = G.record_verifier(case).circuit().verify_batch(c, proofs, coms, ts, rng32=_rng(b"proved" + case.name.encode(), nb))
    assert verdict == bytes(nb), case


@pytest.mark.parametrize("ct", [0, 1])
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "own"])
@pytest.mark.parametrize("case", G.SMALL, ids=[c.name for c in G.SMALL])
def test_prove_named_case(ctx, gens, case, shared, ct):
    ctx.set_option("prover_constant_time", ct)
    try:
        _prove_and_compare(ctx, case, gens, shared)
    finally:
        ctx.set_option("prover_constant_time", 0)


def test_large_case(oracle):
    """n = 1 025 (padded_n 2 048, the bucket chain), Q = 4 200 (z^(q+1) from the 65th high-table entry on), 2 100 ONE terms (66 chunks: the
    second trip of the finish kernel's stride loop): verify and prove on a context of its own"""
    import bulletproofs_amd as bp
    case = G.LARGE
    g = oracle.Gens(2048, 1).export()
    c = bp.Context(0, fixed_window_bits=8)
    c.gens_create(2048, 1)
    try:
        pf, Vs, _ = _valid(case, g)
        good = pf.to_bytes()
        bad = bytearray(good)
        bad[1 + 32 * 12 + 5] ^= 4                         # t_x
        other = case.with_seed(case.seed + 1)
        circuit = G.record_verifier(case).circuit()
        assert circuit.padded_n == 2048 and circuit.n_unique == 11 + 2 + 22
        proofs, coms = [good, bytes(bad), good], [b"".join(Vs)] * 3
        v, reached = _check(c, circuit, G.verifier_gadget(case), g, 2048, proofs, coms, [G.st0_of(case)] * 3, _rng(b"large", 3), True)
        assert list(v) == [0, 1, 0] and reached == 3
        v, reached = _check(c, G.record_verifier(other).circuit(), G.verifier_gadget(other), g, 2048, [good], coms[:1], [G.st0_of(case)], _rng(b"large2", 1), True)
        assert list(v) == [1] and reached == 1
        _prove_and_compare(c, case, g, True, nb=2)
    finally:
        c.close()


# ---- the batch-combined check: all named cases as the groups of ONE call ------------------------------------------------------
def _groups(gens, tamper):
    out = []
    for i, case in enumerate(G.SMALL):
        pf, Vs, _ = _valid(case, gens)
        good = pf.to_bytes()
        proofs = [good]
        if tamper and i in (4, 9, 16):
            bad = bytearray(good)
            if i == 4:
                bad[-40] ^= 1                             # inside a: the mega-check fails
            elif i == 9:
                bad[1 + 32 * ((3 if good[0] == 0 else 6) + 5) + 3] ^= 1     # t_x
            else:
                bad = bad[:-1]                            # a format error: stops before the mega-check
            proofs = [bytes(bad), good] if i != 9 else [good, bytes(bad)]
        out.append(_group(G.record_verifier(case).circuit(), G.verifier_gadget(case), proofs, [b"".join(Vs)] * len(proofs),
                          [G.st0_of(case)] * len(proofs), shared=i % 2 == 0))
    return out


def test_combined_all_named_cases_valid(ctx, gens):
    groups = _groups(gens, False)
    n = len(G.SMALL)
    rng, w = _rng(b"combined", n), hashlib.shake_256(b"generated weights").digest(64 * n)
    v, batch, ts = _combined(ctx, groups, rng, w)
    ev, ets = _per_proof(ctx, groups, rng)
    tw = _twin(groups, gens, CAP, rng)
    assert [c for c, _, _ in tw] == [0] * n and all(t is not None for _, _, t in tw)
    assert v == ev == bytes(n) and ts == ets
    assert T.combination([t for _, _, t in tw], w) == R.IDENTITY and batch == bytes(33)


def test_combined_all_named_cases_three_tampered(ctx, gens):
    groups = _groups(gens, True)
    n = len(G.SMALL) + 3
    rng, w = _rng(b"combined-bad", n), hashlib.shake_256(b"generated weights, tampered").digest(64 * n)
    tw = _twin(groups, gens, CAP, rng)
    v, batch, ts = _combined(ctx, groups, rng, w)
    ev, ets = _per_proof(ctx, groups, rng)
    assert v == ev and list(v) == [c for c, _, _ in tw] and ts == ets
    assert sorted(v) == [0] * (n - 3) + [1, 1, 2]
    want = T.combination([t for _, _, t in tw], w)
    assert want is not None and want != R.IDENTITY and batch == b"\x01" + want


def test_pool_threads_named_cases(gens):
    import bulletproofs_amd as bp
    pool = bp.Pool((0,), 4)
    pool.gens_create(CAP, 1)
    try:
        jobs = []
        for i, case in enumerate(G.SMALL):
            pf, Vs, _ = _valid(case, gens)
            b = bytearray(pf.to_bytes())
            if i % 4 == 3:
                b[50] ^= 1
            jobs.append((G.record_verifier(case).circuit(), G.verifier_gadget(case), bytes(b), b"".join(Vs), G.st0_of(case)))
        want = [R.verify_with(gd, gens, CAP, st, p, [cm[32 * j:32 * j + 32] for j in range(len(cm) // 32)], _rng(b"p%d" % i, 1))[::2]
                for i, (_, gd, p, cm, st) in enumerate(jobs)]
        got = [None] * len(jobs)

        def work(t):
            for i in range(t, len(jobs), 8):
                circ, _, p, cm, st = jobs[i]
                v, ts = circ.verify_batch(pool, [p], cm, st, rng32=_rng(b"p%d" % i, 1), want_transcripts=True)
                got[i] = (v[0], ts)

        th = [threading.Thread(target=work, args=(t,)) for t in range(8)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert got == want
    finally:
        pool.close()


@pytest.mark.parametrize("chunk", range(4))
def test_sweep_verify_and_prove(ctx, gens, chunk):
    for case in SWEEP[chunk::4]:
        pf, Vs, _ = _valid(case, gens)
        circuit = G.record_verifier(case).circuit()
        v, reached = _check(ctx, circuit, G.verifier_gadget(case), gens, CAP, [pf.to_bytes()], [b"".join(Vs)], [G.st0_of(case)], _rng(b"sweep%d" % case.seed, 1), True)
        assert list(v) == [0] and reached == 1, case
        _prove_and_compare(ctx, case, gens, True, nb=1)
