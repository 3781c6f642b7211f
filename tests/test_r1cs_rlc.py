"""Batch-combined R1CS verification without a GPU: the Python layer's argument checks and grouping of recorded verifiers, the C entry
points' refusals, and r1cs_rlc.h's weigh / remap / limb-sum / reduction bodies compiled for the host (tests/r1cs_rlc_harness) against
Python big ints."""
import ctypes as C
import hashlib
import os
import random
import subprocess

import pytest

import r1cs_twin as R

HERE = os.path.dirname(os.path.abspath(__file__))
L_ORDER = R.L


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("r1rlc") / "libr1rlc.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "r1cs_rlc_harness", "harness.cpp")])
    return C.CDLL(so)


def _record(gadget, m, tag):
    from bulletproofs_amd import r1cs
    st0 = R.transcript_state(R.T.Transcript(tag))
    cs = r1cs.Verifier(st0)
    vs = [cs.commit(hashlib.shake_256(tag + b"%d" % j).digest(32)) for j in range(m)]
    gadget(cs, vs)
    return cs


def _range(n):
    return lambda cs, v: R.range_gadget(cs, v[0], None, n)


def test_python_argument_checks():
    from bulletproofs_amd import r1cs
    circ = _record(_range(8), 1, b"args").circuit()
    TS = 208
    with pytest.raises(ValueError):
        r1cs.verify_batch_combined(None, [])                                   # zero groups
    with pytest.raises(ValueError):
        r1cs.verify_batch_combined(None, [(circ, [b"x"], bytes(32))])          # not a 4-tuple
    with pytest.raises(ValueError):
        r1cs.verify_batch_combined(None, [(circ, [b"x", b"y"], bytes(32), bytes(TS))])        # commitments for one proof, two proofs
    with pytest.raises(ValueError):
        r1cs.verify_batch_combined(None, [(circ, [b"x", b"y", b"z"], bytes(96), bytes(2 * TS))])   # neither one state nor one per proof
    with pytest.raises(ValueError):
        r1cs.verify_batch_combined(None, [(circ, [b"x"], bytes(32), bytes(TS))], rng32=bytes(31))
    with pytest.raises(ValueError):
        r1cs.verify_batch_combined(None, [(circ, [b"x"], bytes(32), bytes(TS))], weights64=bytes(128))


def test_c_entry_points_refuse_without_context_or_groups():
    from bulletproofs_amd import r1cs
    L = r1cs.lib()
    circ = _record(_range(8), 1, b"cargs").circuit()
    sz = C.c_size_t
    arr = (C.c_void_p * 1)(circ._h.value)
    nb = (sz * 1)(1)
    for fn in (L.bpgpu_r1cs_verify_rlc, L.bpgpu_pool_r1cs_verify_rlc):
        assert fn(None, 1, arr, nb, None, None, None, None, None, None, None, None, None, None, None) == -1
    v = C.create_string_buffer(1)
    assert L.bpgpu_r1cs_verify_rlc(None, 0, None, None, None, None, None, None, None, None, None, None, v, None, None) == -1


def test_grouping_of_identical_recordings():
    from bulletproofs_amd import r1cs
    a = _record(_range(8), 1, b"g-a")
    b = _record(_range(8), 1, b"g-b")                  # same gadget, other commitment and transcript
    c = _record(_range(16), 1, b"g-c")
    d = _record(_range(8), 1, b"g-d")
    groups, index = r1cs.group_verifiers([(a, b"pa"), (c, b"pc"), (b, b"pb"), (d, b"pd")])
    assert len(groups) == 2
    (c0, p0, cm0, ts0), (c1, p1, cm1, ts1) = groups
    assert c0 is a.circuit() and c1 is c.circuit()
    assert p0 == [b"pa", b"pb", b"pd"] and p1 == [b"pc"]
    assert cm0 == a.V[0] + b.V[0] + d.V[0] and ts0 == a.transcript + b.transcript + d.transcript and ts1 == c.transcript
    assert index == [0, 3, 1, 2]


def _u32s(bs):
    return (C.c_uint32 * (len(bs) // 4))(*[int.from_bytes(bs[4 * i:4 * i + 4], "little") for i in range(len(bs) // 4)])


def _int(arr, i):
    return int.from_bytes(b"".join(int(arr[8 * i + q]).to_bytes(4, "little") for q in range(8)), "little")


@pytest.mark.parametrize("nproofs,pn,PN,short", [(1, 1, 1, 0), (3, 4, 16, 0), (64, 8, 8, 0), (70, 16, 64, 0), (5, 2, 2048, 0),
                                                 (64, 1024, 1, 1), (3, 64, 16, 1), (128, 16, 16, 1)])
def test_weigh_remap_and_limb_sums(harness, nproofs, pn, PN, short):
    """short: the slice's padded_n exceeds the generators (every proof stopped in launch 1; pn may exceed PN): no generator term, no row
    past the accumulators, the unique terms zero"""
    rnd = random.Random(nproofs * 7919 + pn * 31 + PN)
    U = 11 + 3 + 2 * (pn.bit_length() - 1)
    G = 2 * pn + 2
    status = [0 if rnd.random() < 0.7 else rnd.choice([1, 2, 4]) for _ in range(nproofs)]
    status[0] = 0
    if short:
        status = [4 if rnd.random() < 0.8 else 2 for _ in range(nproofs)]
    rho = [rnd.randrange(L_ORDER) for _ in range(nproofs)]
    if nproofs > 1:
        rho[1] = L_ORDER - 1                           # the largest canonical values: the limb sums' worst case
    gen = [[L_ORDER - 1 - rnd.randrange(4) if rnd.random() < 0.3 else rnd.randrange(L_ORDER) for _ in range(G)] for _ in range(nproofs)]
    usc = [[rnd.randrange(L_ORDER) for _ in range(U)] for _ in range(nproofs)]
    upt = [[rnd.getrandbits(256) for _ in range(U)] for _ in range(nproofs)]
    gp0, u0 = 5, 7
    pack = lambda rows: _u32s(b"".join(x.to_bytes(32, "little") for r in rows for x in r))
    st = (C.c_uint32 * nproofs)(*status)
    rho_w = _u32s(bytes(32 * gp0) + b"".join(x.to_bytes(32, "little") for x in rho))
    comb_sc = (C.c_uint32 * (8 * (u0 + nproofs * U)))()
    comb_pt = (C.c_uint32 * (8 * (u0 + nproofs * U)))()
    gst = (C.c_uint32 * (gp0 + nproofs))(*([0xdead] * (gp0 + nproofs)))
    out = (C.c_uint32 * (8 * (2 * PN + 2)))()
    assert harness.r1rlc_weigh_slice(nproofs, U, pn, PN, short, gp0, u0, st, rho_w, pack(gen), pack(usc), pack(upt), comb_sc, comb_pt, gst, out) == 0
    assert list(gst)[gp0:] == status and list(gst)[:gp0] == [0xdead] * gp0
    for p in range(nproofs):
        for t in range(U):
            i = u0 + p * U + t
            assert _int(comb_sc, i) == (0 if status[p] else usc[p][t] * rho[p] % L_ORDER)
            assert _int(comb_pt, i) == (0 if status[p] else upt[p][t])
    want = [0] * (2 * PN + 2)
    for p in range(nproofs):
        if status[p] or short:
            continue
        for g in range(G):
            row = g if g < 2 + pn else 2 + PN + (g - 2 - pn)          # H_i: from 2 + pn + i to 2 + PN + i
            assert harness.r1rlc_gen_row(g, pn, PN) == row
            want[row] = (want[row] + rho[p] * gen[p][g]) % L_ORDER
    assert [_int(out, r) for r in range(2 * PN + 2)] == want


def test_weight_reduction_matches_from_bytes_mod_order_wide(harness):
    for i in range(8):
        w = hashlib.shake_256(b"wide%d" % i).digest(64) if i else b"\xff" * 64
        rho = (C.c_uint32 * 16)()
        harness.r1rlc_rho(bytes(64) + w, 1, rho)      # (proof 1 of the call: its 64 bytes and its 8 words)
        assert _int(rho, 1) == int.from_bytes(w, "little") % L_ORDER
