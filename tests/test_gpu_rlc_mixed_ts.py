"""GPU parity tests of the mixed-shape batch-combined check on the callers' own transcripts, bpgpu_rangeproof_verify_rlc_mixed_ts and its pool
form (include/bpgpu.h, csrc/rlc_mix.h): every proof starts from a pre-bound Merlin state, shared by its group or its own, at any STROBE
position.  R must be, bit for bit, ONE oracle multiscalar multiplication sum_i rho_i MegaCheck_i; verdicts and advanced states must be those
of bpgpu_rangeproof_verify_batch_ts group by group, and the oracle's."""
import os
import subprocess

import pytest

import rlc_ts_cases as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["lookup", "bucket"])
def ctx64x8(request):
    """Both forms of the call's one MSM over the proof-specific terms (as test_gpu_rlc_mixed.py)"""
    import bulletproofs_amd as bp
    c = bp.Context(0)
    c.set_option("bucket_min_terms", 1 if request.param == "bucket" else 2**31 - 1)
    c.gens_create(64, 8)
    yield c
    c.close()


def golden_groups(golden, copies=2):
    return [(c["n"], c["m"], bytes.fromhex(c["proof"]) * copies, len(c["proof"]) // 2, golden["vc_bytes"][:32 * c["m"]] * copies, golden["label"])
            for c in golden["cases"]]


def with_proof(group, b, fn):
    n, m, proofs, plen, coms, last = group
    pr = bytearray(proofs[plen * b:plen * (b + 1)])
    fn(pr)
    return (n, m, proofs[:plen * b] + bytes(pr) + proofs[plen * (b + 1):], plen, coms, last)


def total_of(groups):
    return sum(len(g[2]) // g[3] for g in groups)


def test_single_state_of_a_label_equals_the_label_entry_point(ctx64x8, oracle, golden):
    """the 16 golden shapes, every group with the single state Transcript::new(label) and stride 0: verdicts, batch verdict and the 32-byte
    R are those of bpgpu_rangeproof_verify_rlc_mixed for the same rng bytes and weights -- all good, and with a tampered, a malformed and
    an undecodable copy in three different groups"""
    groups = golden_groups(golden)
    assert len({(g[0], g[1]) for g in groups}) == 16
    tot = total_of(groups)
    rng, wts = T.rand64(b"eq-r", tot), T.rand64(b"eq-w", tot)
    st0 = oracle.transcript_new(golden["label"])
    on_ts = lambda gs: [g[:5] + (st0,) for g in gs]
    want = ctx64x8.rangeproof_verify_rlc_mixed(groups, rng, wts)
    assert want == (bytes(tot), True, bytes(32))
    assert ctx64x8.rangeproof_verify_rlc_mixed_ts(on_ts(groups), rng, wts) == want
    groups[2] = with_proof(groups[2], 1, lambda pr: pr.__setitem__(130, pr[130] ^ 0x10))               # (8, 4): tampered
    groups[7] = with_proof(groups[7], 0, lambda pr: pr.__setitem__(slice(128, 160), b"\xff" * 32))     # (16, 8): malformed
    groups[12] = with_proof(groups[12], 1, lambda pr: pr.__setitem__(32, pr[32] | 1))                  # (64, 1): undecodable
    want = ctx64x8.rangeproof_verify_rlc_mixed(groups, rng, wts)
    assert not want[1] and want[2] != bytes(32) and [i for i, v in enumerate(want[0]) if v] == [2 * 2 + 1, 2 * 7, 2 * 12 + 1]
    assert ctx64x8.rangeproof_verify_rlc_mixed_ts(on_ts(groups), rng, wts) == want


SIZES = [(8, 1, 70), (8, 2, 7), (16, 4, 7), (64, 1, 7)]


def bound_sets(oracle, gens):
    return [T.proofs_on_states(oracle, gens, n, m, cnt, "differing", b"mx%d-%d" % (n, m)) for n, m, cnt in SIZES]


def test_prebound_per_proof_states_at_differing_positions(ctx64x8, oracle, oracle_gens_64_8):
    """(8, 1) x 70 -- across the 64-lane block, a ragged tail --, (8, 2) x 5, (16, 4) x 4, (64, 1) x 3, every proof made by the oracle's prover on
    its own bound state, positions differing within every group: one identity check, the oracle's end states; with explicit and with
    library-drawn randomness"""
    sets = bound_sets(oracle, oracle_gens_64_8)
    take = [70, 5, 4, 3]
    groups = [T.as_call_group(s, 0, k) for s, k in zip(sets, take)]
    assert all(len({st[200] for st in s["states"][:k]}) > 1 for s, k in zip(sets, take))
    tot = sum(take)
    rng, wts = T.rand64(b"pb-r", tot), T.rand64(b"pb-w", tot)
    ends = b"".join(e[2] for s, k in zip(sets, take) for e in T.oracle_expectation(oracle, oracle_gens_64_8, s)(bytes(64 * len(s["proofs"])))[:k])
    for r, w in ((rng, wts), (None, None)):
        verdict, ok, enc, ts = ctx64x8.rangeproof_verify_rlc_mixed_ts(groups, r, w, want_transcripts=True)
        assert ok and enc == bytes(32) and verdict == bytes(tot)
        assert ts == ends          # (the end state does not depend on the rng bytes)


def bad_call(oracle, gens):
    """the four sets with one bad member of each kind per group -> (call groups, kinds in call order, oracle expectation, rng, weights)"""
    sets = bound_sets(oracle, gens)
    where = [dict(zip(T.KINDS, (3, 17, 40, 65, 69)))] + [dict(zip(T.KINDS, (1, 2, 3, 4, 5)))] * 3
    bad = [T.with_bad_members(oracle, s, w) for s, w in zip(sets, where)]
    tot = sum(len(s["proofs"]) for s in sets)
    rng, wts = T.rand64(b"bad-r", tot), T.rand64(b"bad-w", tot)
    exps, kinds, gp = [], [], 0
    for g, k in bad:
        nb = len(g["proofs"])
        exps += T.oracle_expectation(oracle, gens, g)(rng[64 * gp:64 * (gp + nb)])
        kinds += k
        gp += nb
    return [T.as_call_group(g) for g, _ in bad], kinds, exps, rng, wts


def test_bad_members_of_every_kind_in_every_group(ctx64x8, oracle, oracle_gens_64_8):
    """per group a tampered t_x, a non-canonical scalar, an identity L_1, an undecodable A and a right proof on a wrong history: R is the
    oracle's combination of the good, the tampered and the wrong-history proofs; verdicts and states are the per-proof entry point's and
    the oracle's"""
    groups, kinds, exps, rng, wts = bad_call(oracle, oracle_gens_64_8)
    tot = len(kinds)
    verdict, ok, enc, ts = ctx64x8.rangeproof_verify_rlc_mixed_ts(groups, rng, wts, want_transcripts=True)
    want_r = T.combined_point(oracle, exps, kinds, wts)
    assert not ok and enc == want_r and enc != bytes(32)
    assert list(verdict) == [e[0] for e in exps]
    assert list(verdict) == [{"good": 0, "noncanonical": 2}.get(k, 1) for k in kinds]
    gp = 0
    for n, m, proofs, pl, coms, states in groups:
        nb = len(proofs) // pl
        v1, ts1 = ctx64x8.rangeproof_verify_batch_ts(n, m, proofs, pl, coms, states, rng[64 * gp:64 * (gp + nb)], want_transcripts=True)
        assert verdict[gp:gp + nb] == v1 and ts[208 * gp:208 * (gp + nb)] == ts1
        gp += nb
    for i, (e, k) in enumerate(zip(exps, kinds)):
        assert ts[208 * i:208 * (i + 1)] == e[2], (i, k)
    # the same call with the script switched off: the byte-wise replay in every group, the same answer
    ctx64x8.set_option("transcript_script", 0)
    try:
        assert ctx64x8.rangeproof_verify_rlc_mixed_ts(groups, rng, wts, want_transcripts=True) == (verdict, ok, enc, ts)
    finally:
        ctx64x8.set_option("transcript_script", 1)


def test_uniform_positions_take_the_script_and_shared_states_too(ctx64x8, oracle, oracle_gens_64_8):
    """a group whose per-proof states share one position (the scripted form with ts_in), a group on one shared bound state (stride 0)
    and a group at differing positions in one call, with a stopped and a rejected member: the same checks"""
    uni = T.proofs_on_states(oracle, oracle_gens_64_8, 8, 2, 70, "uniform", b"mu")
    sha = T.proofs_on_states(oracle, oracle_gens_64_8, 16, 1, 5, "shared", b"ms")
    dif = T.proofs_on_states(oracle, oracle_gens_64_8, 8, 1, 6, "differing", b"md")
    assert len({st[200:203] for st in uni["states"]}) == 1 and len(set(uni["states"])) == 70
    bad = [T.with_bad_members(oracle, uni, {"identity_L": 2, "noncanonical": 66, "tampered": 68}), T.with_bad_members(oracle, sha, {"undecodable_A": 1}),
           T.with_bad_members(oracle, dif, {"identity_L": 5})]
    groups = [T.as_call_group(bad[0][0]), T.as_call_group(bad[1][0], shared=True), T.as_call_group(bad[2][0])]
    tot = 81
    rng, wts = T.rand64(b"us-r", tot), T.rand64(b"us-w", tot)
    exps, kinds, gp = [], [], 0
    for g, k in bad:
        nb = len(g["proofs"])
        exps += T.oracle_expectation(oracle, oracle_gens_64_8, g)(rng[64 * gp:64 * (gp + nb)])
        kinds += k
        gp += nb
    verdict, ok, enc, ts = ctx64x8.rangeproof_verify_rlc_mixed_ts(groups, rng, wts, want_transcripts=True)
    assert not ok and enc == T.combined_point(oracle, exps, kinds, wts) and enc != bytes(32)
    assert list(verdict) == [e[0] for e in exps] and ts == b"".join(e[2] for e in exps)
    # the good members alone
    groups = [T.as_call_group(uni), T.as_call_group(sha, shared=True), T.as_call_group(dif)]
    verdict, ok, enc, ts = ctx64x8.rangeproof_verify_rlc_mixed_ts(groups, want_transcripts=True)
    assert ok and enc == bytes(32) and verdict == bytes(tot)
    assert ts == b"".join(e[2] for s in (uni, sha, dif) for e in T.oracle_expectation(oracle, oracle_gens_64_8, s)(bytes(64 * len(s["proofs"]))))


def test_weights_are_indexed_by_position_in_the_call(ctx64x8, oracle, oracle_gens_64_8):
    """the same proof bytes and state as the only member of two groups, weight rho in one and l - rho in the other: the two terms cancel
    exactly when each group reads ITS row.  Good proof: R is the identity.  Both copies tampered alike: rho M - rho M, still the identity
    (weights the prover could predict prove nothing -- which is why they must not be).  One copy tampered: R is not the identity."""
    s = T.proofs_on_states(oracle, oracle_gens_64_8, 8, 2, 7, "differing", b"mx8-2")
    one = T.as_call_group(s, 3, 4)
    bad = with_proof(one, 0, lambda pr: pr.__setitem__(130, pr[130] ^ 1))
    rho = int.from_bytes(T.rand64(b"neg", 1), "little") % T.L
    wts = rho.to_bytes(64, "little") + (T.L - rho).to_bytes(64, "little")
    rng = T.rand64(b"same-c", 1) * 2       # (the same batching challenge in both copies: the same mega-check)
    verdict, ok, enc = ctx64x8.rangeproof_verify_rlc_mixed_ts([one, one], rng, wts)
    assert ok and enc == bytes(32) and verdict == bytes(2)
    verdict, ok, enc = ctx64x8.rangeproof_verify_rlc_mixed_ts([bad, bad], rng, wts)
    assert ok and enc == bytes(32)
    verdict, ok, enc = ctx64x8.rangeproof_verify_rlc_mixed_ts([one, bad], rng, wts)
    assert not ok and enc != bytes(32) and list(verdict) == [0, 1]
    _, msm = ctx64x8.rangeproof_verify_batch_ts(bad[0], bad[1], bad[2], bad[3], bad[4], bad[5], rng[:64], want_msm=True)
    st, want = oracle.msm((T.L - rho).to_bytes(32, "little"), msm)
    assert st == 0 and enc == want


def test_malformed_states_and_strides_are_refused_before_anything_runs(ctx64x8, oracle, oracle_gens_64_8):
    import bulletproofs_amd as bp
    s = T.proofs_on_states(oracle, oracle_gens_64_8, 8, 2, 7, "differing", b"mx8-2")
    n, m, proofs, pl, coms, states = T.as_call_group(s, 0, 3)
    broken = bytearray(states)
    broken[208 + 200] = 200          # pos beyond the rate
    with pytest.raises(bp.BpgpuError):
        ctx64x8.rangeproof_verify_rlc_mixed_ts([(n, m, proofs, pl, coms, bytes(broken))])
    with pytest.raises(bp.BpgpuError):
        ctx64x8.rangeproof_verify_rlc_ts(n, m, proofs, pl, coms, bytes(broken))
    assert ctx64x8.rangeproof_verify_rlc_mixed_ts([]) == (b"", True, bytes(32))
    assert ctx64x8.rangeproof_verify_rlc_mixed_ts([(n, m, b"", pl, b"", states[:208])], want_transcripts=True) == (b"", True, bytes(32), b"")


def test_pool_form_and_the_python_api(ctx64x8, oracle, oracle_gens_64_8):
    """bpgpu_pool_rangeproof_verify_rlc_mixed_ts equals the context form on the bad-member call; RangeProof.verify_batch_combined and
    verify_mixed_combined on bound transcripts return verify_batch's verdicts"""
    import bulletproofs_amd as bp
    from bulletproofs_amd import BulletproofGens, RangeProof, Transcript
    groups, kinds, exps, rng, wts = bad_call(oracle, oracle_gens_64_8)
    want = ctx64x8.rangeproof_verify_rlc_mixed_ts(groups, rng, wts, want_transcripts=True)
    pool = bp.Pool((0,), 2)
    pool.gens_create(64, 8)
    assert pool.rangeproof_verify_rlc_mixed_ts(groups, rng, wts, want_transcripts=True) == want
    assert pool.rangeproof_verify_rlc_mixed_ts([]) == (b"", True, bytes(32))
    pool.close()
    bp_gens = BulletproofGens(64, 8)
    pc_gens = bp_gens.pedersen()
    bound = lambda st: Transcript(None, st)
    # one shape: a shared bound transcript, then one transcript per proof
    n, m, proofs, pl, coms, states = groups[1]
    nb = len(proofs) // pl
    prs = [proofs[pl * i:pl * (i + 1)] for i in range(nb)]
    cms = [[coms[32 * (m * i + j):32 * (m * i + j) + 32] for j in range(m)] for i in range(nb)]
    tss = [bound(states[208 * i:208 * (i + 1)]) for i in range(nb)]
    res = RangeProof.verify_batch_combined(bp_gens, pc_gens, tss, prs, cms, n)
    assert [0 if r is None else r.code for r in res] == list(want[0][70:70 + nb])
    assert all(t.state == states[208 * i:208 * (i + 1)] for i, t in enumerate(tss))           # the caller's transcripts are not advanced
    assert RangeProof.verify_batch_combined(bp_gens, pc_gens, tss[0], prs, cms, n) == RangeProof.verify_batch(bp_gens, pc_gens, tss[0], prs, cms, n)
    # mixed: every item of the call with its own bound transcript, in another order
    items = []
    for n, m, proofs, pl, coms, states in groups:
        for i in range(len(proofs) // pl):
            items.append((bound(states[208 * i:208 * (i + 1)]), proofs[pl * i:pl * (i + 1)], [coms[32 * (m * i + j):32 * (m * i + j) + 32] for j in range(m)], n))
    res = RangeProof.verify_mixed_combined(bp_gens, pc_gens, items[::-1], bound_transcripts=True)
    assert [0 if r is None else r.code for r in res] == list(want[0])[::-1]
    with pytest.raises(ValueError):
        RangeProof.verify_mixed_combined(bp_gens, pc_gens, items[:1])                         # (the default stays: fresh transcripts only)


def test_cpp_mirror_routes_bound_transcripts_to_the_new_call(tmp_path):
    """include/bulletproofs.hpp: RangeProof::verify_batch_combined with a bound Transcript, and its one-Transcript-per-proof overload"""
    exe = str(tmp_path / "range_proof_combined_ts_test")
    csrc = os.path.join(ROOT, "bulletproofs_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "range_proof_combined_ts_test.cpp"),
                           "-L", csrc, "-lbpgpu", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout
