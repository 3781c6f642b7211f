"""The batch-combined LinearProof check without a GPU: linear_rlc.h's rho, weigh and reduce lane bodies compiled for the host
(tests/lin_rlc_harness) and run lane by lane over synthetic staging in both layouts, against Python big ints and the oracle's ChaCha20
restatement."""
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
    so = str(tmp_path_factory.mktemp("linrlc") / "liblinrlc.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "lin_rlc_harness", "harness.cpp")])
    lib = C.CDLL(so)
    lib.linrlc_weight_domain.restype = C.c_uint32
    return lib


def _words(vals):
    return (C.c_uint32 * max(8 * len(vals), 1))(*[(x >> (32 * q)) & 0xffffffff for x in vals for q in range(8)])


def _int(arr, i):
    return sum(int(arr[8 * i + q]) << (32 * q) for q in range(8))


def _rho(harness, weights64, key, p):
    buf = (C.c_uint32 * (8 * (p + 1)))()
    harness.linrlc_rho(weights64, key, p, buf)
    return _int(buf, p)


@pytest.mark.parametrize("fixed", [True, False], ids=["table", "explicit"])
@pytest.mark.parametrize("n", [1, 2, 16])
@pytest.mark.parametrize("nbatch", [1, 63, 64, 65])
def test_weigh_and_reduce_lanes_against_big_integers(harness, nbatch, n, fixed):
    """every combined row == sum_p rho_p coeff_{p,row} mod l, every combined-list slot == rho_p scalar with the right point; proofs
    that stopped in the front end and the padding lanes of the last wavefront contribute nothing"""
    rnd = random.Random(10000 * nbatch + 10 * n + fixed)
    k = n.bit_length() - 1
    U, nrows = 2 * k + 2, n + 2
    N = U if fixed else n + 2 * k + 4
    big = lambda: L_ORDER - 1 - rnd.randrange(4) if rnd.random() < 0.3 else rnd.randrange(L_ORDER)   # near l: the limb sums' worst case
    status = [0] * nbatch
    if nbatch > 1:
        status[rnd.randrange(nbatch)] = 1
        status[nbatch - 1] = 2
    weights = bytes(rnd.getrandbits(8) for _ in range(64 * nbatch))
    rho = [int.from_bytes(weights[64 * p:64 * p + 64], "little") % L_ORDER for p in range(nbatch)]
    rho_w = (C.c_uint32 * (8 * nbatch))()
    for p in range(nbatch):
        harness.linrlc_rho(weights, None, p, rho_w)
        assert _int(rho_w, p) == rho[p]
    # what k_lin_prepare leaves: per proof the unique terms (C, L.., R.., S) and the base coefficients (B, F, G..).  A stopped proof's
    # staging holds whatever its lane wrote before it stopped: garbage here, and none of it may reach the outputs
    uniq_sc = [[big() for _ in range(U)] for _ in range(nbatch)]
    uniq_pt = [[rnd.getrandbits(256) for _ in range(U)] for _ in range(nbatch)]
    coeff = [[big() for _ in range(nrows)] for _ in range(nbatch)]
    bases = [rnd.getrandbits(256) for _ in range(nrows)]
    list_sc, list_pt, gen_sc = [], [], []
    for p in range(nbatch):
        if fixed:
            list_sc += uniq_sc[p]
            list_pt += uniq_pt[p]
            gen_sc += coeff[p]
        else:                                   # B, F, C, L.., R.., G.., S
            list_sc += coeff[p][:2] + uniq_sc[p][:U - 1] + coeff[p][2:] + uniq_sc[p][U - 1:]
            list_pt += bases[:2] + uniq_pt[p][:U - 1] + bases[2:] + uniq_pt[p][U - 1:]
    assert len(list_sc) == nbatch * N
    head = 0 if fixed else nrows
    slots = head + nbatch * U
    comb_sc = (C.c_uint32 * (8 * slots))(*([FILL] * (8 * slots)))
    comb_pt = (C.c_uint32 * (8 * slots))(*([FILL] * (8 * slots)))
    row_out = (C.c_uint32 * (8 * nrows))(*([FILL] * (8 * nrows)))
    enc = lambda x: x.to_bytes(32, "little")
    rc = harness.linrlc_weigh_reduce(nbatch, n, k, int(fixed), (C.c_uint32 * nbatch)(*status), rho_w, _words(gen_sc) if fixed else None,
                                     _words(list_sc), _words(list_pt), enc(bases[0]), enc(bases[1]), b"".join(enc(x) for x in bases[2:]),
                                     comb_sc, comb_pt, row_out)
    assert rc == 0
    want = [sum(rho[p] * coeff[p][r] for p in range(nbatch) if status[p] == 0) % L_ORDER for r in range(nrows)]
    if fixed:
        assert [_int(row_out, r) for r in range(nrows)] == want
    else:
        assert [_int(comb_sc, r) for r in range(nrows)] == want
        assert [_int(comb_pt, r) for r in range(nrows)] == bases          # B, F, G_0.. once, from the caller's own encodings
        assert all(x == FILL for x in row_out)
    for p in range(nbatch):
        for u in range(U):
            i = head + p * U + u
            assert _int(comb_sc, i) == (0 if status[p] else rho[p] * uniq_sc[p][u] % L_ORDER), (p, u)
            assert _int(comb_pt, i) == (0 if status[p] else uniq_pt[p][u]), (p, u)


def test_a_batch_of_stopped_proofs_adds_nothing(harness):
    nbatch, n, k = 65, 2, 1
    U, nrows = 4, 4
    rho_w = _words([7] * nbatch)
    junk = _words([L_ORDER - 1] * (nbatch * U))
    comb_sc = (C.c_uint32 * (8 * nbatch * U))(*([FILL] * (8 * nbatch * U)))
    comb_pt = (C.c_uint32 * (8 * nbatch * U))(*([FILL] * (8 * nbatch * U)))
    row_out = (C.c_uint32 * (8 * nrows))(*([FILL] * (8 * nrows)))
    rc = harness.linrlc_weigh_reduce(nbatch, n, k, 1, (C.c_uint32 * nbatch)(*([2] * nbatch)), rho_w, _words([L_ORDER - 1] * (nbatch * nrows)), junk,
                                     junk, None, None, None, comb_sc, comb_pt, row_out)
    assert rc == 0 and not any(row_out) and not any(comb_sc) and not any(comb_pt)


def test_library_drawn_weights_are_chacha20_blocks_under_their_own_domain(harness):
    """weights64 == NULL: rho_p = from_bytes_mod_order_wide(block p of ChaCha20(key, nonce = "wcln")) -- a nonce of its own, apart from
    the R1CS and range-proof combinations'"""
    from chacha_rng import chacha20_block
    dom = int.from_bytes(b"wcln", "little")
    assert harness.linrlc_weight_domain() == dom
    others = [int.from_bytes(t, "little") for t in (b"wc1r", b"s1cr", b"wcmx", b"rcmx")] + [1, 2]
    assert dom not in others
    key = hashlib.shake_256(b"lin-rlc-key").digest(32)
    seen = set()
    for p in (0, 1, 63, 64, 70000):
        got = _rho(harness, None, key, p)
        assert got == int.from_bytes(chacha20_block(key, p, dom), "little") % L_ORDER, p
        seen.add(got)
    assert len(seen) == 5
    assert _rho(harness, None, bytes(32), 0) != _rho(harness, None, key, 0)
