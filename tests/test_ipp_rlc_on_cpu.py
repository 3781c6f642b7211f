"""The batch-combined InnerProductProof check without a GPU: ipp_rlc.h's rho, uniq, weigh and reduce lane bodies compiled for the host
(tests/ipp_rlc_harness) and run lane by lane -- over synthetic staging against Python big ints, over real proofs (behind ipp.h's own
front end) against the oracle's per-proof check points, and the weights against the oracle's ChaCha20 restatement."""
import ctypes as C
import hashlib
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
L_ORDER = 2**252 + 27742317777372353535851937790883648493
FILL = 0x5a5a5a5a


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ipprlc") / "libipprlc.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "ipp_rlc_harness", "harness.cpp")])
    lib = C.CDLL(so)
    lib.ipprlc_weight_domain.restype = C.c_uint32
    return lib


def _words(vals):
    return (C.c_uint32 * max(8 * len(vals), 1))(*[(x >> (32 * q)) & 0xffffffff for x in vals for q in range(8)])


def _int(arr, i):
    return sum(int(arr[8 * i + q]) << (32 * q) for q in range(8))


def _enc(x):
    return x.to_bytes(32, "little")


def _filled(nwords):
    return (C.c_uint32 * max(nwords, 1))(*([FILL] * max(nwords, 1)))


def _rho(harness, weights64, key, p):
    buf = (C.c_uint32 * (8 * (p + 1)))()
    harness.ipprlc_rho(weights64, key, p, buf)
    return _int(buf, p)


def _s(n, k, u, ui):
    """s_i = prod_b (bit_b(i) ? u : u^-1)[k-1-b] (ipp.rs:241-250) and its inverse"""
    s, sinv = [], []
    for i in range(n):
        a = b = 1
        for bb in range(k):
            j = k - 1 - bb
            a = a * (u[j] if (i >> bb) & 1 else ui[j]) % L_ORDER
            b = b * (ui[j] if (i >> bb) & 1 else u[j]) % L_ORDER
        s.append(a)
        sinv.append(b)
    return s, sinv


@pytest.mark.parametrize("walk", [False, True], ids=["row-per-lane", "gray-walk"])
@pytest.mark.parametrize("fixed", [True, False], ids=["table", "explicit"])
@pytest.mark.parametrize("n", [1, 2, 16])
@pytest.mark.parametrize("nbatch", [1, 63, 64, 65])
def test_uniq_weigh_and_reduce_lanes_against_big_integers(harness, nbatch, n, fixed, walk):
    """every combined row == sum_p rho_p coeff_{p,row} mod l, every combined-list slot == the weighted scalar beside the right point; proofs
    that stopped in the front end and the padding lanes of the last wavefront contribute nothing, and every row a lane names lies inside
    the accumulators (the harness returns non-zero otherwise).  walk: a lane takes min(8, n) rows in Gray-code order, as the runtime has
    it from 2^20 (row, proof) pairs on; else one row"""
    rnd = random.Random(10000 * nbatch + 10 * n + fixed)
    k = n.bit_length() - 1
    U, head = 2 * k + 2, 0 if fixed else 2 * n
    big = lambda: L_ORDER - 1 - rnd.randrange(4) if rnd.random() < 0.3 else rnd.randrange(L_ORDER)   # near l: the limb sums' worst case
    status = [0] * nbatch
    if nbatch > 1:
        status[rnd.randrange(nbatch)] = 1
        status[nbatch - 1] = 2
    weights = b"".join((big().to_bytes(32, "little") + bytes(32)) if rnd.random() < 0.3 else bytes(rnd.getrandbits(8) for _ in range(64)) for _ in range(nbatch))
    rho = [int.from_bytes(weights[64 * p:64 * p + 64], "little") % L_ORDER for p in range(nbatch)]
    rho_w = (C.c_uint32 * (8 * nbatch))()
    for p in range(nbatch):
        harness.ipprlc_rho(weights, None, p, rho_w)
        assert _int(rho_w, p) == rho[p]
    # what the front end leaves per proof, and the caller's inputs.  A stopped proof's staging holds whatever its lane wrote before it
    # stopped and its a / b may be anything: garbage here, and none of it may reach the outputs
    a, b = [big() for _ in range(nbatch)], [big() for _ in range(nbatch)]
    u = [[rnd.randrange(1, L_ORDER) for _ in range(k)] for _ in range(nbatch)]
    ui = [[pow(x, -1, L_ORDER) for x in row] for row in u]
    gf, hf = [[big() for _ in range(n)] for _ in range(nbatch)], [[big() for _ in range(n)] for _ in range(nbatch)]
    pts = [[rnd.getrandbits(256) for _ in range(U)] for _ in range(nbatch)]          # Q, L_0.., R_0.., P
    G, H = [rnd.getrandbits(256) for _ in range(n)], [rnd.getrandbits(256) for _ in range(n)]
    tab = (C.c_uint32 * max(20 * k * nbatch, 1))()
    us, uis, proofs = [], [], b""
    for p in range(nbatch):
        stopped = status[p] != 0
        if k:
            one = (C.c_uint32 * (20 * k))()
            harness.ipprlc_make_table(k, _words(u[p]), _words(ui[p]), one)
            for q in range(20 * k):
                tab[20 * k * p + q] = 0xffffffff if stopped else one[q]
        us += [2**256 - 1] * k if stopped else [x * x % L_ORDER for x in u[p]]
        uis += [2**256 - 1] * k if stopped else [x * x % L_ORDER for x in ui[p]]
        for j in range(k):
            proofs += _enc(pts[p][1 + j]) + _enc(pts[p][1 + k + j])
        proofs += (b"\xff" * 64) if stopped else _enc(a[p]) + _enc(b[p])
    comb_sc, comb_pt, row_out, ab = _filled(8 * (head + nbatch * U)), _filled(8 * (head + nbatch * U)), _filled(8 * (2 * n + 2)), _filled(20 * nbatch)
    cat = lambda rows: b"".join(_enc(x) for row in rows for x in row)
    rc = harness.ipprlc_run(nbatch, n, k, int(fixed), min(8, n) if walk else 1, (C.c_uint32 * nbatch)(*status), rho_w, proofs, b"".join(_enc(pts[p][U - 1]) for p in range(nbatch)),
                            b"".join(_enc(pts[p][0]) for p in range(nbatch)), _words(us), _words(uis), tab, cat(gf), cat(hf), cat([G]), cat([H]), ab,
                            comb_sc, comb_pt, row_out)
    assert rc == 0
    live = [p for p in range(nbatch) if status[p] == 0]
    s = {p: _s(n, k, u[p], ui[p]) for p in live}
    want = [sum(rho[p] * a[p] * s[p][0][i] * gf[p][i] for p in live) % L_ORDER for i in range(n)] + \
           [sum(rho[p] * b[p] * s[p][1][i] * hf[p][i] for p in live) % L_ORDER for i in range(n)]
    if fixed:
        assert [_int(row_out, r) for r in range(2 * n + 2)] == [0, 0] + want          # B_blinding = B = 0, then G.., H..
    else:
        assert [_int(comb_sc, r) for r in range(2 * n)] == want
        assert [_int(comb_pt, r) for r in range(2 * n)] == G + H                      # once, from the caller's own encodings
        assert all(x == FILL for x in row_out)
    for p in range(nbatch):
        exp = [rho[p] * a[p] * b[p]] + [-rho[p] * x * x for x in u[p]] + [-rho[p] * x * x for x in ui[p]] + [-rho[p]]
        for t in range(U):
            i = head + p * U + t
            assert _int(comb_sc, i) == (0 if status[p] else exp[t] % L_ORDER), (p, t)
            assert _int(comb_pt, i) == (0 if status[p] else pts[p][t]), (p, t)


def test_a_batch_of_stopped_proofs_adds_nothing(harness):
    nbatch, n, k, U = 65, 2, 1, 4
    junk = b"\xff" * (32 * nbatch * max(n, U))
    rho_w = _words([7] * nbatch)
    ones = (C.c_uint32 * (20 * k * nbatch))(*([0xffffffff] * (20 * k * nbatch)))
    comb_sc, comb_pt, row_out, ab = _filled(8 * nbatch * U), _filled(8 * nbatch * U), _filled(8 * (2 * n + 2)), _filled(20 * nbatch)
    rc = harness.ipprlc_run(nbatch, n, k, 1, 2, (C.c_uint32 * nbatch)(*([2] * nbatch)), rho_w, junk, junk, junk, _words([L_ORDER - 1] * (nbatch * k)),
                            _words([L_ORDER - 1] * (nbatch * k)), ones, junk, junk, None, None, ab, comb_sc, comb_pt, row_out)
    assert rc == 0 and not any(row_out) and not any(comb_sc) and not any(comb_pt)


def _five_cases(oracle, n, tag):
    """the cases of test_make_ipp_verify: valid, tampered a, wrong P, non-canonical b, identity L_0 (n > 1)"""
    insts = [oracle.ipp_test_instance(n, b"innerproducttest", b"%s-%d-%d" % (tag, n, j)) for j in range(5)]
    t = bytearray(insts[1]["proof"])
    t[-40] ^= 1
    insts[1] = dict(insts[1], proof=bytes(t))
    insts[2] = dict(insts[2], P=insts[2]["Q"])
    nc = bytearray(insts[3]["proof"])
    nc[-32:] = b"\xff" * 32
    insts[3] = dict(insts[3], proof=bytes(nc))
    if n > 1:
        li = bytearray(insts[4]["proof"])
        li[0:32] = bytes(32)
        insts[4] = dict(insts[4], proof=bytes(li))
    assert all(i["G"] == insts[0]["G"] and i["H"] == insts[0]["H"] for i in insts)    # the helper's bases are the same for every seed
    return insts


@pytest.mark.parametrize("walk", [False, True], ids=["row-per-lane", "gray-walk"])
@pytest.mark.parametrize("fixed", [True, False], ids=["table", "explicit"])
@pytest.mark.parametrize("n", [1, 2, 4, 32])
def test_real_proofs_front_end_to_combined_point(harness, oracle, n, fixed, walk):
    """ipp_vs_front_thread and the new lanes over the reference helper's proofs: rows x bases plus the combined list, summed by the oracle,
    equal sum_j rho_j Check_j over the proofs that reach the check (Check_j from oracle.ipp_verify)"""
    label = b"innerproducttest"
    insts = _five_cases(oracle, n, b"hipp-rlc")
    nb, k = len(insts), n.bit_length() - 1
    U, head, pl = 2 * k + 2, 0 if fixed else 2 * n, len(insts[0]["proof"])
    cat = lambda key: b"".join(i[key] for i in insts)
    G, H = insts[0]["G"], insts[0]["H"]
    weights = hashlib.shake_256(b"ipp-rlc-host-%d" % n).digest(64 * nb)
    rho = [int.from_bytes(weights[64 * p:64 * p + 64], "little") % L_ORDER for p in range(nb)]
    rho_w = (C.c_uint32 * (8 * nb))()
    for p in range(nb):
        harness.ipprlc_rho(weights, None, p, rho_w)
    status, us, ui, tab = (C.c_uint32 * nb)(), _filled(8 * k * nb), _filled(8 * k * nb), _filled(20 * k * nb)
    assert harness.ipprlc_front(n, nb, cat("proof"), pl, oracle.transcript_new(label), status, us, ui, tab) == 0
    res = [oracle.ipp_verify(n, i["proof"], label, i["Gf"], i["Hf"], i["P"], i["Q"], G, H) for i in insts]
    assert [r[0] for r in res] == [0, 1, 1, 2, 1 if n > 1 else 0]
    assert list(status) == [0, 0, 0, 2, 1 if n > 1 else 0]
    comb_sc, comb_pt, row_out, ab = _filled(8 * (head + nb * U)), _filled(8 * (head + nb * U)), _filled(8 * (2 * n + 2)), _filled(20 * nb)
    assert harness.ipprlc_run(nb, n, k, int(fixed), min(8, n) if walk else 1, status, rho_w, cat("proof"), cat("P"), cat("Q"), us, ui, tab, cat("Gf"), cat("Hf"), G, H, ab,
                              comb_sc, comb_pt, row_out) == 0
    if fixed:
        assert _int(row_out, 0) == 0 and _int(row_out, 1) == 0
        scal = bytes(row_out)[64:] + bytes(comb_sc)
        pts = G + H + bytes(comb_pt)
    else:
        scal, pts = bytes(comb_sc), bytes(comb_pt)
        assert pts[:64 * n] == G + H
    reach = [j for j in range(nb) if status[j] == 0]
    assert all(res[j][1] != b"\xff" * 32 for j in reach)
    want = oracle.msm(b"".join(_enc(rho[j]) for j in reach), b"".join(res[j][1] for j in reach))
    got = oracle.msm(scal, pts)
    assert got[0] == 0 and want[0] == 0 and got[1] == want[1] != bytes(32)


def test_library_drawn_weights_are_chacha20_blocks_under_their_own_domain(harness):
    """weights64 == NULL: rho_p = from_bytes_mod_order_wide(block p of ChaCha20(key, nonce = "wcpi")) -- a nonce of its own, apart from
    the linear, R1CS and range-proof combinations'"""
    from chacha_rng import chacha20_block
    dom = int.from_bytes(b"wcpi", "little")
    assert harness.ipprlc_weight_domain() == dom == 0x69706377
    others = [int.from_bytes(t, "little") for t in (b"wcln", b"wc1r", b"s1cr", b"wcmx", b"rcmx")] + [1, 2]
    assert dom not in others
    key = hashlib.shake_256(b"ipp-rlc-key").digest(32)
    seen = set()
    for p in (0, 1, 63, 64, 70000):
        got = _rho(harness, None, key, p)
        assert got == int.from_bytes(chacha20_block(key, p, dom), "little") % L_ORDER, p
        seen.add(got)
    assert len(seen) == 5
    assert _rho(harness, None, bytes(32), 0) != _rho(harness, None, key, 0)
