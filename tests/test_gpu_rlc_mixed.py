"""GPU parity tests of the batch-combined check over range proofs of MIXED shapes, bpgpu_rangeproof_verify_rlc_mixed and its pool form
(include/bpgpu.h, csrc/rlc_mix.h): the combined point
    R = sum_i rho_i * MegaCheck_i     (MegaCheck_i = the MSM of src/range_proof/mod.rs:421-443 for proof i, i over ALL groups of the call)
must equal, bit for bit, ONE oracle multiscalar multiplication over the weighted terms of the proofs the front end accepts, and every
proof's verdict must equal the one bpgpu_rangeproof_verify_batch gives it in a call of its own shape with the same rng bytes."""
import hashlib
import os
import random

import pytest

pytestmark = pytest.mark.gpu

L = 2**252 + 27742317777372353535851937790883648493


@pytest.fixture(scope="module", params=["lookup", "bucket"])
def ctx64x8(request):
    """Both forms of the call's one MSM over the proof-specific terms (as test_gpu_rlc.py: window sums / the bucket form)"""
    import bulletproofs_amd as bp
    c = bp.Context(0)
    c.set_option("bucket_min_terms", 1 if request.param == "bucket" else 2**31 - 1)
    c.gens_create(64, 8)
    yield c
    c.close()


def expected_combination(oracle, gg, groups, rng, wts):
    """test_gpu_rlc.py's expected_combination over groups: rho_i and the rng bytes by the proof's index within the call"""
    all_s, all_p, included = [], [], []
    gp = 0
    for n, m, proofs, plen, coms, label in groups:
        for b in range(len(proofs) // plen):
            rc, sc_, pt_ = oracle.verify_terms(gg, proofs[plen * b:plen * (b + 1)], coms[32 * m * b:32 * m * (b + 1)], n, label, rng[64 * gp:64 * gp + 64])
            ok = rc == 0 and all(oracle.lib().oracle_point_decompress_ok(pt_[32 * j:32 * j + 32]) for j in range(len(pt_) // 32))
            included.append(ok)
            if ok:
                rho = int.from_bytes(wts[64 * gp:64 * gp + 64], "little") % L
                all_s.append(b"".join((int.from_bytes(sc_[32 * j:32 * j + 32], "little") * rho % L).to_bytes(32, "little") for j in range(len(sc_) // 32)))
                all_p.append(pt_)
            gp += 1
    if not all_s:
        return included, bytes(32)
    st, enc = oracle.msm(b"".join(all_s), b"".join(all_p))
    assert st == 0
    return included, enc


def per_shape_verdicts(ctx, groups, rng):
    """every group through bpgpu_rangeproof_verify_batch, a call of its own shape with its slice of the rng bytes"""
    out, gp = b"", 0
    for n, m, proofs, plen, coms, label in groups:
        nb = len(proofs) // plen
        if nb:
            out += ctx.rangeproof_verify_batch(n, m, proofs, plen, coms, label, rng[64 * gp:64 * gp + 64 * nb])
        gp += nb
    return out


def total_of(groups):
    return sum(len(g[2]) // g[3] for g in groups)


def rand64(tag, total):
    return hashlib.shake_256(tag).digest(64 * total)


def golden_groups(golden, copies=2):
    return [(c["n"], c["m"], bytes.fromhex(c["proof"]) * copies, len(c["proof"]) // 2, golden["vc_bytes"][:32 * c["m"]] * copies, golden["label"])
            for c in golden["cases"]]


def with_proof(group, b, fn):
    """the group with its proof b rewritten by fn(bytearray)"""
    n, m, proofs, plen, coms, label = group
    pr = bytearray(proofs[plen * b:plen * (b + 1)])
    fn(pr)
    return (n, m, proofs[:plen * b] + bytes(pr) + proofs[plen * (b + 1):], plen, coms, label)


def test_all_golden_shapes_in_one_call(ctx64x8, golden):
    """every (n, m) of {8, 16, 32, 64} x {1, 2, 4, 8}, two copies each with different rng bytes and weights: one identity check"""
    groups = golden_groups(golden)
    assert len({(g[0], g[1]) for g in groups}) == 16
    tot = total_of(groups)
    rng, wts = rand64(b"mix-r", tot), rand64(b"mix-w", tot)
    for r, w in ((rng, wts), (rng, None), (None, wts), (None, None)):
        verdict, ok, enc = ctx64x8.rangeproof_verify_rlc_mixed(groups, r, w)
        assert ok and enc == bytes(32) and verdict == bytes(tot)


def test_golden_shapes_with_bad_members(ctx64x8, oracle, oracle_gens_64_8, golden):
    """a tampered, a malformed and an undecodable copy in three different groups: R is the oracle's combination of the included proofs of
    ALL groups, the verdicts are each group's per-proof ones"""
    groups = golden_groups(golden)

    def tamper(pr):
        pr[130] ^= 0x10

    def fmt(pr):
        pr[128:160] = b"\xff" * 32

    def und(pr):
        pr[32] |= 1

    groups[2] = with_proof(groups[2], 1, tamper)     # (8, 4)
    groups[7] = with_proof(groups[7], 0, fmt)        # (16, 8)
    groups[12] = with_proof(groups[12], 1, und)      # (64, 1)
    tot = total_of(groups)
    rng, wts = rand64(b"mixbad-r", tot), rand64(b"mixbad-w", tot)
    verdict, ok, enc = ctx64x8.rangeproof_verify_rlc_mixed(groups, rng, wts)
    included, exp = expected_combination(oracle, oracle_gens_64_8, groups, rng, wts)
    assert not ok and enc == exp and enc != bytes(32)
    assert included == [i not in (2 * 7, 2 * 12 + 1) for i in range(tot)]
    assert verdict == per_shape_verdicts(ctx64x8, groups, rng)
    assert [i for i, v in enumerate(verdict) if v] == [2 * 2 + 1, 2 * 7, 2 * 12 + 1] and verdict[2 * 7] == 2
    # the malformed and the undecodable copy alone: they are left out, R is the identity, their codes stay
    groups[2] = golden_groups(golden)[2]
    verdict, ok, enc = ctx64x8.rangeproof_verify_rlc_mixed(groups, rng, wts)
    assert ok and enc == bytes(32) and [(i, v) for i, v in enumerate(verdict) if v] == [(14, 2), (25, 1)]


def test_four_shapes_of_one_proof_length(ctx64x8, golden):
    """(8, 8), (16, 4), (32, 2) and (64, 1) all have 672-byte proofs and n m = 64: only the per-shape rows tell them apart.  A (16, 4)
    proof inside the (64, 1) group fails; every other proof passes."""
    by = {(c["n"], c["m"]): bytes.fromhex(c["proof"]) for c in golden["cases"]}
    vc, label = golden["vc_bytes"], golden["label"]
    shapes = [(8, 8), (16, 4), (32, 2), (64, 1)]
    assert all(len(by[s]) == 672 for s in shapes)
    groups = [(n, m, by[(n, m)], 672, vc[:32 * m], label) for n, m in shapes]
    tot = total_of(groups)
    rng, wts = rand64(b"672-r", tot + 1), rand64(b"672-w", tot + 1)
    verdict, ok, enc = ctx64x8.rangeproof_verify_rlc_mixed(groups, rng[:64 * tot], wts[:64 * tot])
    assert ok and enc == bytes(32) and verdict == bytes(tot)
    groups[3] = (64, 1, by[(64, 1)] + by[(16, 4)], 672, vc[:32] * 2, label)
    verdict, ok, enc = ctx64x8.rangeproof_verify_rlc_mixed(groups, rng, wts)
    assert not ok and enc != bytes(32) and list(verdict) == [0, 0, 0, 0, 1]
    assert verdict == per_shape_verdicts(ctx64x8, groups, rng)


def test_groups_rejected_as_a_whole(ctx64x8, golden):
    """n = 24, m = 16 on (64, 8) generators, an n m that does not match the proof length, proof_len = 100: the per-shape path's codes,
    the valid group beside them unaffected; nbatch = 0 in the middle of a call; ngroups = 0"""
    by = {(c["n"], c["m"]): bytes.fromhex(c["proof"]) for c in golden["cases"]}
    vc, label = golden["vc_bytes"], golden["label"]
    valid = (32, 2, by[(32, 2)] * 3, len(by[(32, 2)]), vc[:64] * 3, label)
    empty = (16, 1, b"", len(by[(16, 1)]), b"", label)
    fmt_bad = bytearray(by[(8, 1)])
    fmt_bad[128:160] = b"\xff" * 32                               # FormatError outranks the shape's code
    rejected = [
        ((24, 1, by[(8, 1)] * 2, len(by[(8, 1)]), vc[:32] * 2, label), [3, 3]),                                    # InvalidBitsize
        ((8, 16, (by[(8, 8)] + bytes(64)) * 2, len(by[(8, 8)]) + 64, (vc[:256] * 2) * 2, label), [4, 4]),          # InvalidGeneratorsLength
        ((8, 2, by[(8, 1)] + bytes(fmt_bad), len(by[(8, 1)]), vc[:64] * 2, label), [1, 2]),                        # n m != 2^k: VerificationError
        ((8, 1, bytes(300), 100, vc[:32] * 3, label), [2, 2, 2]),                                                  # FormatError by length
    ]
    for bad, codes in rejected:
        for groups in ([bad, valid], [valid, empty, bad], [bad, empty, valid, bad]):
            tot = total_of(groups)
            rng = rand64(b"rej-r%d" % len(groups), tot)
            verdict, ok, enc = ctx64x8.rangeproof_verify_rlc_mixed(groups, rng, rand64(b"rej-w", tot))
            assert ok and enc == bytes(32)
            assert verdict == per_shape_verdicts(ctx64x8, groups, rng)
            want = []
            for g in groups:
                want += codes if g is bad else [0] * (len(g[2]) // g[3])
            assert list(verdict) == want
    # all four beside one valid group, library-drawn randomness
    groups = [r[0] for r in rejected[:2]] + [valid] + [r[0] for r in rejected[2:]]
    verdict, ok, enc = ctx64x8.rangeproof_verify_rlc_mixed(groups)
    assert ok and enc == bytes(32) and list(verdict) == [3, 3, 4, 4, 0, 0, 0, 1, 2, 2, 2, 2]
    # a failing proof in the valid group: fallback, the rejected groups keep their codes
    groups[2] = with_proof(valid, 1, lambda pr: pr.__setitem__(130, pr[130] ^ 0x10))
    verdict, ok, enc = ctx64x8.rangeproof_verify_rlc_mixed(groups)
    assert not ok and list(verdict) == [3, 3, 4, 4, 0, 1, 0, 1, 2, 2, 2, 2]
    # only rejected / empty groups, and no group at all
    verdict, ok, enc = ctx64x8.rangeproof_verify_rlc_mixed([rejected[0][0], empty])
    assert ok and enc == bytes(32) and list(verdict) == [3, 3]
    assert ctx64x8.rangeproof_verify_rlc_mixed([empty]) == (b"", True, bytes(32))
    assert ctx64x8.rangeproof_verify_rlc_mixed([]) == (b"", True, bytes(32))


@pytest.fixture(scope="module")
def small_proofs(oracle, oracle_gens_64_8):
    nb = 265
    vals = [int.from_bytes(hashlib.shake_256(b"v%d" % i).digest(1), "little") for i in range(nb)]
    bl = b"".join(hashlib.shake_256(b"b%d" % i).digest(31) + b"\x00" for i in range(nb))
    return oracle.prove_batch(oracle_gens_64_8, vals, bl, 1, 8, b"small", b"seed-mix", threads=min(16, os.cpu_count() or 1))


def test_wavefront_edges(ctx64x8, oracle, oracle_gens_64_8, golden, small_proofs):
    """65 and 200 (8, 1) proofs as two groups (a full wavefront plus one lane; three full ones plus eight lanes) beside three (64, 8)
    proofs: clean, then one flipped byte in the 200-proof group"""
    proofs, coms = small_proofs
    pl = oracle.proof_len(8, 1)
    big = next(c for c in golden["cases"] if (c["n"], c["m"]) == (64, 8))
    groups = [(8, 1, proofs[:65 * pl], pl, coms[:65 * 32], b"small"),
              (64, 8, bytes.fromhex(big["proof"]) * 3, len(big["proof"]) // 2, golden["vc_bytes"][:256] * 3, golden["label"]),
              (8, 1, proofs[65 * pl:], pl, coms[65 * 32:], b"small")]
    tot = total_of(groups)
    assert tot == 268
    rng, wts = rand64(b"edge-r", tot), rand64(b"edge-w", tot)
    verdict, ok, enc = ctx64x8.rangeproof_verify_rlc_mixed(groups, rng, wts)
    assert ok and enc == bytes(32) and verdict == bytes(tot)
    groups[2] = with_proof(groups[2], 131, lambda pr: pr.__setitem__(130, pr[130] ^ 0x10))
    verdict, ok, enc = ctx64x8.rangeproof_verify_rlc_mixed(groups, rng, wts)
    included, exp = expected_combination(oracle, oracle_gens_64_8, groups, rng, wts)
    assert all(included) and not ok and enc == exp
    assert verdict == per_shape_verdicts(ctx64x8, groups, rng) and [i for i, v in enumerate(verdict) if v] == [68 + 131]


@pytest.mark.parametrize("form", ["lookup", "bucket"])
def test_call_maximum_below_the_generators(oracle, golden, form):
    """generators (64, 16), groups (8, 2) and (16, 1) only: the call's MSM runs over (N, M) = (16, 2), rows of the big table; both forms
    of that MSM, as ctx64x8"""
    import bulletproofs_amd as bp
    c = bp.Context(0)
    c.set_option("bucket_min_terms", 1 if form == "bucket" else 2**31 - 1)
    c.gens_create(64, 16)
    g = oracle.Gens(64, 16)
    by = {(x["n"], x["m"]): bytes.fromhex(x["proof"]) for x in golden["cases"]}
    vc, label = golden["vc_bytes"], golden["label"]
    groups = [(8, 2, by[(8, 2)] * 3, len(by[(8, 2)]), vc[:64] * 3, label), (16, 1, by[(16, 1)] * 2, len(by[(16, 1)]), vc[:32] * 2, label)]
    rng, wts = rand64(b"low-r", 5), rand64(b"low-w", 5)
    verdict, ok, enc = c.rangeproof_verify_rlc_mixed(groups, rng, wts)
    assert ok and enc == bytes(32) and verdict == bytes(5)
    groups[0] = with_proof(groups[0], 2, lambda pr: pr.__setitem__(130, pr[130] ^ 0x10))
    groups[1] = with_proof(groups[1], 0, lambda pr: pr.__setitem__(32, pr[32] | 1))
    verdict, ok, enc = c.rangeproof_verify_rlc_mixed(groups, rng, wts)
    included, exp = expected_combination(oracle, g, groups, rng, wts)
    assert included == [True, True, True, False, True] and not ok and enc == exp
    assert verdict == per_shape_verdicts(c, groups, rng) and list(verdict) == [0, 0, 1, 1, 0]
    c.close()


def test_pool_and_python_api(ctx64x8, golden):
    """the same batch through bpgpu_pool_rangeproof_verify_rlc_mixed, and RangeProof.verify_mixed_combined with shuffled items: verdicts
    in the caller's order, rng / weight rows following their items"""
    import bulletproofs_amd as bp
    from bulletproofs_amd import BulletproofGens, RangeProof, Transcript, VerificationError, FormatError
    groups = golden_groups(golden)
    groups[5] = with_proof(groups[5], 0, lambda pr: pr.__setitem__(130, pr[130] ^ 0x10))
    groups[9] = with_proof(groups[9], 1, lambda pr: pr.__setitem__(slice(128, 160), b"\xff" * 32))
    tot = total_of(groups)
    rng, wts = rand64(b"pool-r", tot), rand64(b"pool-w", tot)
    want = ctx64x8.rangeproof_verify_rlc_mixed(groups, rng, wts)
    assert not want[1] and [i for i, v in enumerate(want[0]) if v] == [10, 19]
    pool = bp.Pool((0,), 2)
    pool.gens_create(64, 8)
    assert pool.rangeproof_verify_rlc_mixed(groups, rng, wts) == want
    clean = golden_groups(golden)
    assert pool.rangeproof_verify_rlc_mixed(clean) == (bytes(tot), True, bytes(32))
    assert pool.rangeproof_verify_rlc_mixed([]) == (b"", True, bytes(32))
    pool.close()
    # the crate-shaped mirror: items in any order
    bp_gens = BulletproofGens(64, 8)
    pc_gens = bp_gens.pedersen()
    items, gp = [], 0
    for n, m, proofs, plen, coms, label in groups:
        for b in range(len(proofs) // plen):
            items.append((gp, n, proofs[plen * b:plen * (b + 1)], [coms[32 * (m * b + j):32 * (m * b + j) + 32] for j in range(m)]))
            gp += 1
    random.Random(7).shuffle(items)
    call = [(Transcript(golden["label"]), pr, cm, n) for _, n, pr, cm in items]
    rows = lambda buf: b"".join(buf[64 * i:64 * i + 64] for i, _, _, _ in items)
    res = RangeProof.verify_mixed_combined(bp_gens, pc_gens, call, rows(rng), rows(wts))
    assert [None if v == 0 else (VerificationError() if v == 1 else FormatError()) for v in (want[0][i] for i, _, _, _ in items)] == res
    assert sum(r is not None for r in res) == 2
    assert RangeProof.verify_mixed_combined(bp_gens, pc_gens, []) == []
    used = Transcript(golden["label"])
    used.append_message(b"x", b"y")
    with pytest.raises(ValueError):
        RangeProof.verify_mixed_combined(bp_gens, pc_gens, [(used, items[0][2], items[0][3], items[0][1])])
