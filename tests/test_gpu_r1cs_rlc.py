"""Batch-combined R1CS verification on the GPU (bpgpu_r1cs_verify_rlc, bpgpu_pool_r1cs_verify_rlc): verdicts and transcripts equal the
per-proof path (bpgpu_r1cs_verify_batch_ts, itself twin-checked in test_gpu_r1cs.py) and the twin, and the combination R equals ONE
oracle MSM over the twin's weighted mega-check terms (tests/r1cs_rlc_twin.py)."""
import ctypes as C
import hashlib
import random
import threading

import pytest

import r1cs_rlc_twin as T
import r1cs_twin as R
from test_gpu_r1cs import CAP, _example_gadget, _range_gadget, _record, _shuffle_gadget, _shuffle_proofs, _tamper_cases

pytestmark = pytest.mark.gpu


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


def _rng(tag, n):
    return hashlib.shake_256(b"r1cs-rlc-rng" + tag).digest(32 * n)


def _weights(tag, n):
    return hashlib.shake_256(b"r1cs-rlc-w" + tag).digest(64 * n)


def _group(circuit, gadget, proofs, coms, st0s, shared=False):
    return dict(circuit=circuit, gadget=gadget, proofs=list(proofs), coms=list(coms), st0s=list(st0s), shared=shared)


def _mixed(gens):
    """shuffles k in {1, 2, 3, 7, 24}, the example gadget in both serializations, range gadgets n in {2, 10, 32}"""
    out = []
    for k in (1, 2, 3, 7, 24):
        ps = _shuffle_proofs(gens, k, 2)
        out.append(_group(_record(_shuffle_gadget(k), 2 * k, ps[0][2]), _shuffle_gadget(k), [p.to_bytes() for p, _, _ in ps], [c for _, c, _ in ps],
                          [st for _, _, st in ps], shared=k % 2 == 1))
    pf, Vs, st0 = R.prove_example(gens, CAP, (3, 4, 6, 1, 40), 9, b"rlc-example")
    out.append(_group(_record(_example_gadget(9), 5, st0), _example_gadget(9), [pf.to_bytes(), pf.to_bytes(force_two_phase=True)], [b"".join(Vs)] * 2,
                      [st0] * 2))
    for n in (2, 10, 32):
        p1, V1, st0 = R.prove_range(gens, CAP, random.Random(n).getrandbits(n), n, b"rlc-range%d" % n)
        out.append(_group(_record(_range_gadget(n), 1, st0), _range_gadget(n), [p1.to_bytes(), p1.to_bytes(force_two_phase=True)], [V1[0]] * 2,
                          [st0] * 2, shared=True))
    return out


def _tampered(gens):
    """_tamper_cases of the example gadget (both serializations) and of a k = 5 shuffle, one group each"""
    out = []
    pf, Vs, st0 = R.prove_example(gens, CAP, (3, 4, 6, 1, 40), 9, b"rlc-exits")
    circ = _record(_example_gadget(9), 5, st0)
    for two in (False, True):
        cases = _tamper_cases(pf.to_bytes(force_two_phase=two), Vs)
        out.append(_group(circ, _example_gadget(9), [p for p, _ in cases], [c for _, c in cases], [st0] * len(cases)))
    ps = _shuffle_proofs(gens, 5, 1)
    p5, c5, st5 = ps[0]
    cases = _tamper_cases(p5.to_bytes(), [c5[32 * j:32 * j + 32] for j in range(10)])
    out.append(_group(_record(_shuffle_gadget(5), 10, st5), _shuffle_gadget(5), [p for p, _ in cases], [c for _, c in cases], [st5] * len(cases), shared=True))
    return out


def _args(groups):
    return [(g["circuit"], g["proofs"], b"".join(g["coms"]), g["st0s"][0] if g["shared"] else b"".join(g["st0s"])) for g in groups]


def _count(groups):
    return sum(len(g["proofs"]) for g in groups)


def _combined(c, groups, rng32, weights64):
    from bulletproofs_amd import r1cs
    return r1cs.verify_batch_combined(c, _args(groups), rng32=rng32, weights64=weights64, want_batch=True, want_transcripts=True)


def _per_proof(c, groups, rng32):
    """one bpgpu_r1cs_verify_batch_ts call per group: verdicts and transcripts"""
    v, ts, off = b"", b"", 0
    for (circ, proofs, coms, st), g in zip(_args(groups), groups):
        nb = len(proofs)
        vv, tt = circ.verify_batch(c, proofs, coms, st, rng32=rng32[32 * off:32 * (off + nb)] if rng32 else None, want_transcripts=True)
        v, ts, off = v + vv, ts + tt, off + nb
    return v, ts


def _twin(groups, gens, cap, rng32):
    """per proof: (code, mega-check encoding or None, terms or None)"""
    out, off = [], 0
    for g in groups:
        m = g["circuit"].m
        for b, p in enumerate(g["proofs"]):
            cm = g["coms"][b]
            code, mc, _, t = T.verify_terms(g["gadget"], gens, cap, g["st0s"][b], p, [cm[32 * j:32 * j + 32] for j in range(m)], rng32[32 * off:32 * off + 32])
            out.append((code, mc, t))
            off += 1
    return out


def test_many_gadgets_one_call_all_valid(ctx, gens):
    groups = _mixed(gens)
    n = _count(groups)
    rng, w = _rng(b"valid", n), _weights(b"valid", n)
    v, batch, ts = _combined(ctx, groups, rng, w)
    ev, ets = _per_proof(ctx, groups, rng)
    tw = _twin(groups, gens, CAP, rng)
    assert v == ev == bytes(n) and [c for c, _, _ in tw] == [0] * n
    assert T.combination([t for _, _, t in tw], w) == R.IDENTITY
    assert batch == bytes(33)                           # [0] = 0, compress(R) = the identity encoding
    assert ts == ets


def test_tampered_proofs(ctx, gens):
    groups = _mixed(gens)[4:] + _tampered(gens)
    n = _count(groups)
    rng, w = _rng(b"tampered", n), _weights(b"tampered", n)
    tw = _twin(groups, gens, CAP, rng)
    v, batch, ts = _combined(ctx, groups, rng, w)
    ev, ets = _per_proof(ctx, groups, rng)
    assert v == ev and list(v) == [c for c, _, _ in tw] and ts == ets
    assert set(v) == {0, 1, 2}
    want = T.combination([t for _, _, t in tw], w)     # (None: a combined point does not decode)
    assert batch[0] == 1 and batch[1:] == (want if want is not None else bytes(32))
    # the proofs whose points all decode (or that stop before the mega-check): compress(R) itself, not the identity
    keep = [i for i, (_, mc, t) in enumerate(tw) if t is None or mc is not None]
    sub, i = [], 0
    for g in groups:
        idx = [j for j in range(len(g["proofs"])) if i + j in keep]
        if idx:
            sub.append(_group(g["circuit"], g["gadget"], [g["proofs"][j] for j in idx], [g["coms"][j] for j in idx], [g["st0s"][j] for j in idx], g["shared"]))
        i += len(g["proofs"])
    rng2 = b"".join(rng[32 * i:32 * i + 32] for i in keep)
    w2 = b"".join(w[64 * i:64 * i + 64] for i in keep)
    v2, batch2, _ = _combined(ctx, sub, rng2, w2)
    want2 = T.combination([tw[i][2] for i in keep], w2)
    assert want2 is not None and want2 != R.IDENTITY
    assert batch2 == b"\x01" + want2 and list(v2) == [tw[i][0] for i in keep]


def test_early_exits_leave_the_combination_alone(gens):
    import bulletproofs_amd as bp
    small = bp.Context(0)
    small.gens_create(16, 1)                            # range n = 32 (padded_n 32): InvalidGeneratorsLength
    pf, Vs, st0 = R.prove_example(gens, CAP, (3, 4, 6, 1, 40), 9, b"rlc-early")
    good = pf.to_bytes(force_two_phase=True)
    exits = [good, bytes([2]) + good[1:], good[:1] + bytes(32) + good[33:], good + bytes(64), good]   # FormatError, identity A_I1, IPP too long
    groups = [_group(_record(_example_gadget(9), 5, st0), _example_gadget(9), exits, [b"".join(Vs)] * len(exits), [st0] * len(exits))]
    for n in (10, 32):
        p1, V1, s1 = R.prove_range(gens, CAP, 1000 + n, n, b"rlc-early-range%d" % n)
        groups.append(_group(_record(_range_gadget(n), 1, s1), _range_gadget(n), [p1.to_bytes()] * 2, [V1[0]] * 2, [s1] * 2, shared=True))
    n = _count(groups)
    rng, w = _rng(b"early", n), _weights(b"early", n)
    v, batch, ts = _combined(small, groups, rng, w)
    ev, ets = _per_proof(small, groups, rng)
    tw = _twin(groups, gens, 16, rng)
    assert v == ev and list(v) == [c for c, _, _ in tw] == [0, 2, 1, 1, 0, 0, 0, 4, 4]
    assert batch == bytes(33) and ts == ets
    small.close()


@pytest.mark.parametrize("others", [True, False])
def test_whole_wavefronts_of_a_group_past_the_generators(gens, others):
    """64 proofs (whole wavefronts of the weigh launch) of a circuit whose padded_n (32) exceeds the generators (16): InvalidGeneratorsLength,
    no generator term of theirs anywhere -- beside groups that fit, or alone (the combination's padded_n is then 1)"""
    import bulletproofs_amd as bp
    small = bp.Context(0)
    small.gens_create(16, 1)
    groups = []
    if others:
        p1, V1, s1 = R.prove_range(gens, CAP, 1010, 10, b"rlc-wave-range10")
        groups.append(_group(_record(_range_gadget(10), 1, s1), _range_gadget(10), [p1.to_bytes()] * 3, [V1[0]] * 3, [s1] * 3, shared=True))
    p2, V2, s2 = R.prove_range(gens, CAP, 1032, 32, b"rlc-wave-range32")
    groups.append(_group(_record(_range_gadget(32), 1, s2), _range_gadget(32), [p2.to_bytes()] * 64, [V2[0]] * 64, [s2] * 64, shared=True))
    n = _count(groups)
    rng, w = _rng(b"wave", n), _weights(b"wave", n)
    v, batch, ts = _combined(small, groups, rng, w)
    assert (v, ts) == _per_proof(small, groups, rng)
    assert list(v) == [0] * (n - 64) + [4] * 64 and batch == bytes(33)
    small.close()


def test_undecodable_point_falls_back(ctx, gens):
    pf, Vs, st0 = R.prove_example(gens, CAP, (3, 4, 6, 1, 40), 9, b"rlc-undecodable")
    coms = b"".join(Vs)
    groups = _mixed(gens)[6:]
    groups.append(_group(_record(_example_gadget(9), 5, st0), _example_gadget(9), [pf.to_bytes()] * 3, [coms, b"\xff" * 32 + coms[32:], coms], [st0] * 3))
    n = _count(groups)
    rng, w = _rng(b"undecodable", n), _weights(b"undecodable", n)
    v, batch, ts = _combined(ctx, groups, rng, w)
    assert list(v) == [0] * (n - 2) + [1, 0] and batch == b"\x01" + bytes(32)
    assert (v, ts) == _per_proof(ctx, groups, rng)


def test_library_rng_and_weights(ctx, gens):
    groups = _mixed(gens)[3:]
    n = _count(groups)
    v, batch, ts = _combined(ctx, groups, None, None)
    assert v == bytes(n) and batch == bytes(33) and ts == _per_proof(ctx, groups, _rng(b"any", n))[1]
    bad = groups[-1]
    bad["proofs"].append(bad["proofs"][0])
    bad["coms"].append(groups[-2]["coms"][0])         # the wrong statement
    bad["st0s"].append(bad["st0s"][0])
    v, batch, _ = _combined(ctx, groups, None, None)
    assert list(v) == [0] * n + [1] and batch[0] == 1
    assert v == _per_proof(ctx, groups, _rng(b"any", n + 1))[0]


def test_split_into_several_combinations(gens):
    """option r1cs_rlc_max_terms: several MSMs whose points are added before the identity test -- the same R"""
    import bulletproofs_amd as bp
    ref = bp.Context(0)
    ref.gens_create(CAP, 1)
    split = bp.Context(0)
    split.gens_create(CAP, 1)
    split.set_option("r1cs_rlc_max_terms", 64)
    groups = _mixed(gens)
    pf, Vs, st0 = R.prove_example(gens, CAP, (3, 4, 6, 1, 40), 9, b"rlc-split")
    coms = b"".join(Vs)
    groups.append(_group(_record(_example_gadget(9), 5, st0), _example_gadget(9), [pf.to_bytes()] * 2, [coms, coms[32:] + coms[:32]], [st0] * 2))
    n = _count(groups)
    rng, w = _rng(b"split", n), _weights(b"split", n)
    a = _combined(ref, groups, rng, w)
    b = _combined(split, groups, rng, w)
    assert a == b and list(a[0]) == [0] * (n - 1) + [1] and a[1][0] == 1
    assert a[1][1:] == T.combination([t for _, _, t in _twin(groups, gens, CAP, rng)], w)
    ref.close()
    split.close()


def test_1024_shuffles_of_k_1024_from_the_prover(oracle):
    """about 2.1 M proof-specific terms in one combination (bucket.h's chain); then one tampered proof found exactly"""
    import bulletproofs_amd as bp
    from bulletproofs_amd import r1cs
    from test_gpu_r1cs_prover import _sg, _shuffle, _scalars, _st0s
    k, nb, distinct = 1024, 1024, 8
    c = bp.Context(0, fixed_window_bits=8)
    c.gens_create(2 * k, 1)
    st0 = _st0s(b"RlcShuffle1024-", 1)[0]
    provers = []
    for b in range(distinct):
        cs = r1cs.Prover(st0)
        xs = [cs.commit(v, x) for v, x in zip(_shuffle(k, 7000 + b), _scalars(b"rlc-bl%d-" % b, 2 * k))]
        _sg(k)(cs, xs)
        provers.append(cs)
    ins = [p.inputs() for p in provers]
    circuit = provers[0].circuit()
    proofs, coms = [], b""
    for s0 in range(0, nb, 64):
        sel = [ins[(s0 + i) % distinct] for i in range(64)]
        pr, cm, status = provers[0].witness().prove_batch(c, circuit, 64, b"".join(i[0] for i in sel), b"".join(i[1] for i in sel),
                                                         b"".join(i[2] for i in sel), st0, _rng(b"prove%d" % s0, 64))
        assert status == bytes(64)
        proofs += pr
        coms += cm
    rng, w = _rng(b"big", nb), _weights(b"big", nb)
    c.profile_enable()
    c.profile_reset()
    v, batch = circuit.verify_batch_combined(c, proofs, coms, st0, rng32=rng, weights64=w, want_batch=True)
    prof = c.profile_report()
    c.profile_enable(False)
    assert v == bytes(nb) and batch == bytes(33)
    assert prof["r1cs_rlc_weigh"][0] == 1 and prof["r1cs_rlc_reduce"][0] == 1   # one slice, one combination
    assert "bk_accum" in prof and "bk_window" not in prof and "fb_walk" not in prof   # bucket.h's chain, not the fused one
    bad = bytearray(proofs[777])
    bad[1 + 32 * 11 + 5] ^= 4                           # t_x (a two-phase proof: element 11)
    proofs[777] = bytes(bad)
    v, batch = circuit.verify_batch_combined(c, proofs, coms, st0, rng32=rng, weights64=w, want_batch=True)
    assert [i for i in range(nb) if v[i]] == [777] and v[777] == 1 and batch[0] == 1
    c.close()


def test_pool_threads_two_circuits(gens):
    import bulletproofs_amd as bp
    from bulletproofs_amd import r1cs
    pool = bp.Pool((0,), 4)
    pool.gens_create(CAP, 1)
    c = bp.Context(0)
    c.gens_create(CAP, 1)
    pe, Ve, ste = R.prove_example(gens, CAP, (3, 4, 6, 1, 40), 9, b"rlc-pool-ex")
    pr, Vr, str_ = R.prove_range(gens, CAP, 77, 8, b"rlc-pool-range")
    ce, cr = _record(_example_gadget(9), 5, ste), _record(_range_gadget(8), 1, str_)
    jobs = []
    for i in range(16):
        b = bytearray(pr.to_bytes())
        if i % 4 == 3:
            b[50] ^= 1
        jobs.append(([(ce, [pe.to_bytes()] * 2, b"".join(Ve) * 2, ste), (cr, [bytes(b)], Vr[0], str_)], _rng(b"p%d" % i, 3), _weights(b"p%d" % i, 3)))
    want = [r1cs.verify_batch_combined(c, g, rng32=rg, weights64=wt, want_batch=True, want_transcripts=True) for g, rg, wt in jobs]
    got = [None] * len(jobs)

    def work(t):
        for i in range(t, len(jobs), 8):
            g, rg, wt = jobs[i]
            got[i] = r1cs.verify_batch_combined(pool, g, rng32=rg, weights64=wt, want_batch=True, want_transcripts=True)

    th = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got == want
    assert [w[0] for w in want] == [bytes([0, 0, 1 if i % 4 == 3 else 0]) for i in range(16)]
    pool.close()
    c.close()


def test_c_argument_validation(ctx, gens):
    from bulletproofs_amd import r1cs
    L = r1cs.lib()
    p1, V1, st0 = R.prove_range(gens, CAP, 5, 8, b"rlc-args")
    circ = _record(_range_gadget(8), 1, st0)
    sz, u32p = C.c_size_t, C.POINTER(C.c_uint32)
    ln = (C.c_uint32 * 1)(len(p1.to_bytes()))
    args = dict(circ=(C.c_void_p * 1)(circ._h.value), nb=(sz * 1)(1), pr=(C.c_char_p * 1)(p1.to_bytes()), st=(sz * 1)(len(p1.to_bytes())),
                ln=(u32p * 1)(C.cast(ln, u32p)), cm=(C.c_char_p * 1)(V1[0]), ts=(C.c_char_p * 1)(st0), tss=(sz * 1)(0))
    verdict = C.create_string_buffer(1)

    def call(ng=1, **over):
        a = dict(args, **over)
        return L.bpgpu_r1cs_verify_rlc(ctx.h, ng, a["circ"], a["nb"], a["pr"], a["st"], a["ln"], a["cm"], a["ts"], a["tss"], None, None, verdict, None, None)

    assert call() == 0 and verdict.raw == b"\x00"
    assert call(ng=0) == -1
    for key in args:
        assert call(**{key: None}) == -1, key
    assert call(tss=(sz * 1)(100)) == -1
    with pytest.raises(ValueError):
        r1cs.verify_batch_combined(ctx, [])
