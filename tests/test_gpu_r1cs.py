"""R1CS proofs on the GPU (bpgpu_r1cs_verify_batch_ts, bpgpu_pool_r1cs_verify_ts) against the test twin (tests/r1cs_twin.py):
verdict, the 32-byte mega-check and the transcript each proof leaves behind, bit for bit."""
import hashlib
import random
import threading

import pytest

import r1cs_twin as R
from r1cs_corpus import tamper_cases as _tamper_cases

pytestmark = pytest.mark.gpu

CAP = 128


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


def _rng(tag, nb):
    return hashlib.shake_256(b"r1cs-rng" + tag).digest(32 * nb)


def _record(gadget, m, st0):
    from bulletproofs_amd import r1cs
    cs = r1cs.Verifier(st0)
    vs = [cs.commit(bytes(32)) for _ in range(m)]
    gadget(cs, vs)
    return cs.circuit()


def _check(c, circuit, gadget, gens, cap, proofs, coms, st0s, rng32, shared=False):
    """verify `proofs` (list of bytes) on the GPU and with the twin; compare verdict, mega-check (where it decided) and transcripts"""
    nb = len(proofs)
    m = circuit.m
    ts = st0s[0] if shared else b"".join(st0s)
    v, mc, tso = circuit.verify_batch(c, proofs, b"".join(coms), ts, rng32=rng32, want_msm=True, want_transcripts=True)
    for b in range(nb):
        code, emc, ets = R.verify_with(gadget, gens, cap, st0s[0] if shared else st0s[b], proofs[b], [coms[b][32 * j:32 * j + 32] for j in range(m)],
                                       rng32[32 * b:32 * b + 32] if rng32 else bytes(32))
        assert v[b] == code, (b, v[b], code)
        assert tso[208 * b:208 * b + 208] == ets, b
        if emc is not None and rng32 is not None:
            assert mc[32 * b:32 * b + 32] == emc, b
    return v


def _shuffle_gadget(k):
    return lambda cs, v: R.shuffle_gadget(cs, v[:k], v[k:])


def _example_gadget(c2):
    return lambda cs, v: R.example_gadget(cs, v[0], v[1], v[2], v[3], v[4], c2)


def _range_gadget(n):
    return lambda cs, v: R.range_gadget(cs, v[0], None, n)


def _shuffle_proofs(gens, k, count, label=b"ShuffleProofTest"):
    out = []
    for i in range(count):
        rnd = random.Random(k * 1000 + i)
        inp = [rnd.getrandbits(64) for _ in range(k)]
        o = inp[:]
        rnd.shuffle(o)
        pf, Vs, st0 = R.prove_shuffle(gens, CAP if k < 64 else 2048, label, inp, o, b"gpu-shuffle-%d-%d" % (k, i))
        out.append((pf, b"".join(Vs), st0))
    return out


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 24, 42])
def test_shuffle_gadget(ctx, gens, k):
    ps = _shuffle_proofs(gens, k, 2)
    circuit = _record(_shuffle_gadget(k), 2 * k, ps[0][2])
    proofs = [p.to_bytes() for p, _, _ in ps]
    if k == 1:   # one-phase: both serializations
        proofs += [p.to_bytes(force_two_phase=True) for p, _, _ in ps]
    bad = bytearray(proofs[0])
    bad[-40] ^= 1                                     # inside a
    proofs.append(bytes(bad))
    coms = [c for _, c, _ in ps] * (len(proofs) // 2) + [ps[0][1]]
    coms = coms[:len(proofs)]
    st0s = [ps[0][2]] * len(proofs)
    v = _check(ctx, circuit, _shuffle_gadget(k), gens, CAP, proofs, coms, st0s, _rng(b"s%d" % k, len(proofs)), shared=True)
    assert list(v[:-1]) == [0] * (len(proofs) - 1)


def test_example_gadget_both_serializations(ctx, gens):
    pf, Vs, st0 = R.prove_example(gens, CAP, (3, 4, 6, 1, 40), 9, b"gpu-example")
    proofs = [pf.to_bytes(), pf.to_bytes(force_two_phase=True)]
    coms = [b"".join(Vs)] * 2
    for c2, want in ((9, 0), (10, 1)):
        circuit = _record(_example_gadget(c2), 5, st0)
        v = _check(ctx, circuit, _example_gadget(c2), gens, CAP, proofs, coms, [st0, st0], _rng(b"ex", 2))
        assert list(v) == [want, want]


@pytest.mark.parametrize("n", [2, 10, 32, 63])
def test_range_gadget(ctx, gens, n):
    v_ok = random.Random(n).getrandbits(n)
    p1, V1, st0 = R.prove_range(gens, CAP, v_ok, n, b"gpu-range%d" % n)
    p2, V2, _ = R.prove_range(gens, CAP, 1 << n, n, b"gpu-range-out%d" % n)
    circuit = _record(_range_gadget(n), 1, st0)
    proofs = [p1.to_bytes(), p2.to_bytes(), p1.to_bytes(force_two_phase=True)]
    v = _check(ctx, circuit, _range_gadget(n), gens, CAP, proofs, [V1[0], V2[0], V1[0]], [st0] * 3, _rng(b"r%d" % n, 3))
    assert list(v) == [0, 1, 0]


@pytest.mark.parametrize("form", ["one-phase", "two-phase"])
def test_every_exit_path(ctx, gens, form):
    pf, Vs, st0 = R.prove_example(gens, CAP, (3, 4, 6, 1, 40), 9, b"gpu-exits")
    good = pf.to_bytes(force_two_phase=form == "two-phase")
    cases = _tamper_cases(good, Vs)
    circuit = _record(_example_gadget(9), 5, st0)
    v = _check(ctx, circuit, _example_gadget(9), gens, CAP, [p for p, _ in cases], [c for _, c in cases], [st0] * len(cases), _rng(b"x", len(cases)))
    assert v[-1] == 0 and set(v[:-1]) <= {1, 2}


def test_two_phase_exit_paths_and_per_proof_transcripts(ctx, gens):
    ps = _shuffle_proofs(gens, 5, 1)
    pf, coms, st0 = ps[0]
    Vs = [coms[32 * j:32 * j + 32] for j in range(10)]
    cases = _tamper_cases(pf.to_bytes(), Vs)
    circuit = _record(_shuffle_gadget(5), 10, st0)
    # per-proof transcripts: every other proof starts from a transcript with one message more (a failure for the valid ones)
    st1 = R.transcript_from_state(st0)
    st1.append_message(b"extra", b"message")
    st1 = R.transcript_state(st1)
    st0s = [st0 if i % 2 == 0 else st1 for i in range(len(cases))]
    v = _check(ctx, circuit, _shuffle_gadget(5), gens, CAP, [p for p, _ in cases], [c for _, c in cases], st0s, _rng(b"t", len(cases)))
    assert v[-1] == (0 if (len(cases) - 1) % 2 == 0 else 1)


def test_library_rng_and_too_small_generators(gens):
    import bulletproofs_amd as bp
    n = 10
    p1, V1, st0 = R.prove_range(gens, CAP, 1000, n, b"gpu-rng")
    circuit = _record(_range_gadget(n), 1, st0)
    c = bp.Context(0)
    c.gens_create(CAP, 1)
    v, ts = circuit.verify_batch(c, [p1.to_bytes()] * 3, V1[0] * 3, st0, want_transcripts=True)   # rng32 = NULL
    assert list(v) == [0, 0, 0] and ts[:208] == R.verify_with(_range_gadget(n), gens, CAP, st0, p1.to_bytes(), V1, bytes(32))[2]
    c.close()
    small = bp.Context(0)
    small.gens_create(8, 1)                          # padded_n = 16 > 8: InvalidGeneratorsLength
    v = _check(small, circuit, _range_gadget(n), gens, 8, [p1.to_bytes()], [V1[0]], [st0], _rng(b"g", 1))
    assert list(v) == [4]
    small.close()


def test_shuffle_1024_batch_bucket_chain(oracle):
    """k = 1024 (padded_n = 2048, 2081 points per proof: the bucket chain) on a small-table context"""
    import bulletproofs_amd as bp
    g = oracle.Gens(2048, 1).export()
    ps = _shuffle_proofs(g, 1024, 8)
    c = bp.Context(0, fixed_window_bits=8)
    c.gens_create(2048, 1)
    circuit = _record(_shuffle_gadget(1024), 2048, ps[0][2])
    assert circuit.padded_n == 2048 and circuit.n_unique == 2081
    proofs = [p.to_bytes() for p, _, _ in ps]
    coms = [cm for _, cm, _ in ps]
    bad = bytearray(proofs[3])
    bad[1 + 32 * 12 + 5] ^= 4                         # t_x
    proofs += [bytes(bad), proofs[0], proofs[1]]
    coms += [coms[3], coms[1], coms[1]]               # the last two: the wrong statement / the right one
    v = _check(c, circuit, _shuffle_gadget(1024), g, 2048, proofs, coms, [ps[0][2]] * len(proofs), _rng(b"big", len(proofs)), shared=True)
    assert list(v) == [0] * 8 + [1, 1, 0]
    c.close()


def test_pool_threads_two_circuits(gens):
    import bulletproofs_amd as bp
    pool = bp.Pool((0,), 4)
    pool.gens_create(CAP, 1)
    pe, Ve, ste = R.prove_example(gens, CAP, (3, 4, 6, 1, 40), 9, b"pool-ex")
    pr, Vr, str_ = R.prove_range(gens, CAP, 77, 8, b"pool-range")
    ce, cr = _record(_example_gadget(9), 5, ste), _record(_range_gadget(8), 1, str_)
    jobs = []
    for i in range(16):
        if i % 2 == 0:
            jobs.append((ce, _example_gadget(9), pe.to_bytes(), b"".join(Ve), ste))
        else:
            b = bytearray(pr.to_bytes())
            if i % 4 == 3:
                b[50] ^= 1
            jobs.append((cr, _range_gadget(8), bytes(b), Vr[0], str_))
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
    pool.close()
