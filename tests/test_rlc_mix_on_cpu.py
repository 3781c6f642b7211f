"""The batch-combined check over range proofs of mixed shapes without a GPU: rlc_mix.h's row remap, weigh lane body and library-drawn
randomness compiled for the host (tests/rlc_mix_harness) against Python big ints and the oracle's ChaCha20 restatement."""
import ctypes as C
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
L_ORDER = 2**252 + 27742317777372353535851937790883648493


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rlcmix") / "librlcmix.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "rlc_mix_harness", "harness.cpp")])
    lib = C.CDLL(so)
    lib.rlcmix_gen_row.restype = C.c_uint32
    return lib


def gen_ids(n, m, cap_n, cap_m):
    """gen_ids_for (csrc/bpgpu.hip): the generator terms of an (n, m) proof -- B_blinding, B, G(n, m), H(n, m) -- as ids into the table of
    BulletproofGens::new(cap_n, cap_m)"""
    tot = cap_n * cap_m
    return [0, 1] + [2 + j * cap_n + i for j in range(m) for i in range(n)] + [2 + tot + j * cap_n + i for j in range(m) for i in range(n)]


@pytest.mark.parametrize("N,M", [(64, 8), (64, 16), (32, 8)])
def test_row_remap_follows_gen_ids_for(harness, golden, N, M):
    """every (n, m) of the golden set that fits into the call's (N, M): row g of the proof's own list and its image name the same
    generator, the images are injective, rows 0 and 1 stay"""
    shapes = sorted({(c["n"], c["m"]) for c in golden["cases"]})
    assert len(shapes) == 16
    big = gen_ids(N, M, 64, 16)
    for n, m in shapes:
        if n > N or m > M:
            continue
        own = gen_ids(n, m, 64, 16)
        img = [harness.rlcmix_gen_row(g, n, m, N, M) for g in range(2 * n * m + 2)]
        assert img[:2] == [0, 1]
        assert len(set(img)) == len(img) and max(img) < 2 * N * M + 2
        assert [big[r] for r in img] == own, (n, m)
        for j in range(m):
            for i in range(n):
                assert img[2 + j * n + i] == 2 + j * N + i and img[2 + n * m + j * n + i] == 2 + N * M + j * N + i


def _u32s(bs):
    return (C.c_uint32 * max(len(bs) // 4, 1))(*[int.from_bytes(bs[4 * i:4 * i + 4], "little") for i in range(len(bs) // 4)])


def _int(arr, i):
    return int.from_bytes(b"".join(int(arr[8 * i + q]).to_bytes(4, "little") for q in range(8)), "little")


def _pack(vals):
    return _u32s(b"".join(x.to_bytes(32, "little") for x in vals))


def _unique_point(pr, cm, k, u):
    """rp_unique_point_ptr: A, S, T_1, T_2, L_0.., R_0.., V_0.."""
    if u < 4:
        return pr[32 * u:32 * u + 32]
    if u < 4 + k:
        return pr[224 + 64 * (u - 4):][:32]
    if u < 4 + 2 * k:
        return pr[224 + 64 * (u - 4 - k) + 32:][:32]
    return cm[32 * (u - 4 - 2 * k):][:32]


@pytest.mark.parametrize("nb0,nb1", [(1, 65), (63, 64), (64, 1), (65, 63)])
def test_weigh_lanes_of_two_groups(harness, nb0, nb1):
    """two groups of different shape, (16, 2) and (8, 8), into the call's (N, M) = (16, 8): the combined list and the reduced row sums
    against big integers; one proof of every group stopped; 1 / 63 / 64 / 65 proofs exercise the padding lanes"""
    rnd = random.Random(1000 * nb0 + nb1)
    N, M = 16, 8
    nrows = 2 * N * M + 2
    acc = (C.c_uint64 * (nrows * 10))()
    gp_total = 3 + nb0 + nb1
    gst = (C.c_uint32 * gp_total)(*([0xdead] * gp_total))
    groups = [(16, 2, 5, nb0, 3, 7), (8, 8, 6, nb1, 3 + nb0, 7 + nb0 * (4 + 2 * 5 + 2))]
    u_end = groups[1][5] + nb1 * (4 + 2 * 6 + 8)
    comb_sc = (C.c_uint32 * (8 * u_end))(*([0x5a5a5a5a] * (8 * u_end)))
    comb_pt = (C.c_uint32 * (8 * u_end))(*([0x5a5a5a5a] * (8 * u_end)))
    want = [0] * nrows
    checks = []
    for n, m, k, nb, gp0, u0 in groups:
        U, plen = 4 + 2 * k + m, 32 * (9 + 2 * k)
        big = lambda: L_ORDER - 1 - rnd.randrange(4) if rnd.random() < 0.3 else rnd.randrange(L_ORDER)   # near l: the limb sums' worst case
        status = [0] * nb
        status[rnd.randrange(nb)] = rnd.choice([1, 2])
        proofs = bytes(rnd.getrandbits(8) for _ in range(nb * plen))
        coms = bytes(rnd.getrandbits(8) for _ in range(nb * m * 32))
        row0, row1 = [big() for _ in range(nb)], [big() for _ in range(nb)]
        usc = [[rnd.randrange(L_ORDER) for _ in range(U)] for _ in range(nb)]
        coef = [[0 if status[p] else big() for _ in range(2 * n * m)] for p in range(nb)]
        rc = harness.rlcmix_weigh_group(nb, n, m, k, N, M, gp0, u0, proofs, coms, (C.c_uint32 * nb)(*status), _pack(row0), _pack(row1),
                                        _pack([x for r in usc for x in r]), _pack([x for r in coef for x in r]), comb_sc, comb_pt, gst, acc)
        assert rc == 0
        for p in range(nb):
            if status[p]:
                continue
            want[0] = (want[0] + row0[p]) % L_ORDER
            want[1] = (want[1] + row1[p]) % L_ORDER
            for j in range(m):
                for i in range(n):
                    want[2 + j * N + i] = (want[2 + j * N + i] + coef[p][j * n + i]) % L_ORDER
                    want[2 + N * M + j * N + i] = (want[2 + N * M + j * N + i] + coef[p][n * m + j * n + i]) % L_ORDER
        checks.append((n, m, k, nb, gp0, u0, U, plen, status, proofs, coms, usc))
    out = (C.c_uint32 * (8 * nrows))()
    harness.rlcmix_reduce(nrows, acc, out)
    assert [_int(out, r) for r in range(nrows)] == want
    assert list(gst)[:3] == [0xdead] * 3
    for n, m, k, nb, gp0, u0, U, plen, status, proofs, coms, usc in checks:
        assert list(gst)[gp0:gp0 + nb] == status
        for p in range(nb):
            pr, cm = proofs[plen * p:plen * (p + 1)], coms[32 * m * p:32 * m * (p + 1)]
            for t in range(U):
                i = u0 + p * U + t
                assert _int(comb_sc, i) == (0 if status[p] else usc[p][t])
                assert _int(comb_pt, i) == (0 if status[p] else int.from_bytes(_unique_point(pr, cm, k, t), "little"))
    assert all(x == 0x5a5a5a5a for x in list(comb_sc)[:8 * 7])          # nothing before the first group's slice


def test_library_drawn_randomness_is_keyed_by_the_call_global_index(harness):
    """weights and batching challenges the caller did not bring: block i of ChaCha20(key, nonce = the entry point's own domain) with i the
    proof's index within the CALL -- (group 0, proof 0) and (group 1, proof 0) of one call never share a weight"""
    from chacha_rng import chacha20_block
    key = bytes(range(32))
    nb0 = 5                                                   # group 0 holds proofs 0 .. 4 of the call, group 1 starts at 5
    doms = {0: int.from_bytes(b"wcmx", "little"), 1: int.from_bytes(b"rcmx", "little")}
    for which, dom in doms.items():
        got = {}
        for gp in (0, 1, nb0, nb0 + 1, 70000):
            buf = C.create_string_buffer(64)
            harness.rlcmix_draw(key, gp, which, buf)
            got[gp] = buf.raw
            assert buf.raw == chacha20_block(key, gp, dom), (which, gp)
        assert got[0] != got[nb0] and len(set(got.values())) == len(got)
        assert int.from_bytes(got[0], "little") % L_ORDER != int.from_bytes(got[nb0], "little") % L_ORDER
    a, b = C.create_string_buffer(64), C.create_string_buffer(64)
    harness.rlcmix_draw(key, 3, 0, a)
    harness.rlcmix_draw(key, 3, 1, b)
    assert a.raw != b.raw                                     # the two domains differ
    for dom in doms.values():
        assert dom not in (1, 2)                              # ... and from the one-shape chain's (RP_SEED_RNG, RP_SEED_WEIGHTS)
