"""GPU parity tests of the one-shape batch-combined check on the callers' own transcripts, bpgpu_rangeproof_verify_rlc_ts[_dev]
(include/bpgpu.h): the combination mode of the per-shape launch chain (weights, csrc/rlc.h) together with caller-supplied start states and
the states handed back, in all three forms of launch 1 -- k_rp_stage1_coop (up to 256 proofs, one position), k_rp_stage1<true> (more proofs,
one position) and k_rp_stage1<false> (positions that differ)."""
import pytest

import rlc_ts_cases as T

pytestmark = pytest.mark.gpu

N, M = 8, 2


@pytest.fixture(scope="module", params=["lookup", "bucket"])
def ctx64x8(request):
    import bulletproofs_amd as bp
    c = bp.Context(0)
    c.set_option("bucket_min_terms", 1 if request.param == "bucket" else 2**31 - 1)
    c.gens_create(64, 8)
    yield c
    c.close()


def check_good_and_bad(ctx, oracle, gens, group, nb, shared, where):
    """the first nb proofs of the group: all good -> one identity check and the oracle's end states, with explicit and with library-drawn
    randomness; with the bad members -> R is the oracle's combination, verdicts and states those of bpgpu_rangeproof_verify_batch_ts and of
    the oracle"""
    sub = dict(group, proofs=group["proofs"][:nb], coms=group["coms"][:nb], states=group["states"][:nb])
    n, m, proofs, pl, coms, states = T.as_call_group(sub, shared=shared)
    rng, wts = T.rand64(b"one-r", nb), T.rand64(b"one-w", nb)
    ends = b"".join(e[2] for e in T.oracle_expectation(oracle, gens, sub)(rng))
    for r, w in ((rng, wts), (None, None)):
        verdict, ok, enc, ts = ctx.rangeproof_verify_rlc_ts(n, m, proofs, pl, coms, states, r, w, want_transcripts=True)
        assert ok and enc == bytes(32) and verdict == bytes(nb) and ts == ends
    if shared:
        where = {k: i for k, i in where.items() if k != "wrong_history"}   # (one state for the batch: no member can have another history)
    bad, kinds = T.with_bad_members(oracle, sub, where)
    n, m, proofs, pl, coms, states = T.as_call_group(bad, shared=shared)
    exps = T.oracle_expectation(oracle, gens, bad)(rng)
    verdict, ok, enc, ts = ctx.rangeproof_verify_rlc_ts(n, m, proofs, pl, coms, states, rng, wts, want_transcripts=True)
    assert not ok and enc == T.combined_point(oracle, exps, kinds, wts) and enc != bytes(32)
    v1, ts1 = ctx.rangeproof_verify_batch_ts(n, m, proofs, pl, coms, states, rng, want_transcripts=True)
    assert verdict == v1 and ts == ts1
    assert list(verdict) == [e[0] for e in exps] and ts == b"".join(e[2] for e in exps)
    assert list(verdict) == [{"good": 0, "noncanonical": 2}.get(k, 1) for k in kinds]


WHERE = {5: dict(zip(T.KINDS, (0, 1, 2, 3, 4))), 300: dict(zip(T.KINDS, (7, 63, 64, 257, 299)))}


@pytest.mark.parametrize("nb", [5, 300])
@pytest.mark.parametrize("mode", ["shared", "uniform", "differing"])
def test_one_shape_on_caller_transcripts(ctx64x8, oracle, oracle_gens_64_8, nb, mode):
    """(8, 2), 5 proofs (below the 256-proof limit of the 32-lanes-per-proof replay) and 300 (above it); one shared state (stride 0), one
    state per proof at one position (the script with ts_in) and at differing positions (the byte-wise replay)"""
    group = T.proofs_on_states(oracle, oracle_gens_64_8, N, M, 300, mode, b"os-" + mode.encode())
    pos = {st[200:203] for st in group["states"][:nb]}
    assert (len(pos) > 1) == (mode == "differing")
    check_good_and_bad(ctx64x8, oracle, oracle_gens_64_8, group, nb, mode == "shared", WHERE[nb])


def test_device_pointer_form_leaves_combined_proofs_undecided(ctx64x8, oracle, oracle_gens_64_8):
    """bpgpu_rangeproof_verify_rlc_ts_dev on torch buffers, one state per proof: a good batch gives verdicts 0 and the oracle's end states;
    with one tampered and one malformed member the combined proofs are BPGPU_VERDICT_UNDECIDED and the malformed one keeps its code"""
    import torch
    import bulletproofs_amd as bp
    L_ = bp.lib()
    group = T.proofs_on_states(oracle, oracle_gens_64_8, N, M, 300, "differing", b"os-differing")
    dev = torch.device("cuda", 0)
    to_dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    nb = 6
    sub = dict(group, proofs=group["proofs"][:nb], coms=group["coms"][:nb], states=group["states"][:nb])
    bad, _ = T.with_bad_members(oracle, sub, {"tampered": 1, "noncanonical": 4})
    rng, wts = T.rand64(b"dev-r", nb), T.rand64(b"dev-w", nb)
    for g, want_v, want_b in ((sub, [0] * nb, 0), (bad, [5, 5, 5, 5, 2, 5], 1)):
        n, m, proofs, pl, coms, states = T.as_call_group(g)
        d_p, d_c, d_t, d_r, d_w = to_dev(proofs), to_dev(coms), to_dev(states), to_dev(rng), to_dev(wts)
        d_v = torch.full((nb,), 255, dtype=torch.uint8, device=dev)
        d_o = torch.full((36,), 255, dtype=torch.uint8, device=dev)
        d_to = torch.zeros((208 * nb,), dtype=torch.uint8, device=dev)
        rc = L_.bpgpu_rangeproof_verify_rlc_ts_dev(ctx64x8.h, n, m, nb, d_p.data_ptr(), pl, d_c.data_ptr(), None, d_t.data_ptr(), d_r.data_ptr(), d_w.data_ptr(),
                                                   d_v.data_ptr(), d_o.data_ptr(), d_to.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert d_v.cpu().tolist() == want_v and d_o.cpu().tolist()[0] == want_b
        exps = T.oracle_expectation(oracle, oracle_gens_64_8, g)(rng)
        assert bytes(d_to.cpu().numpy()) == b"".join(e[2] for e in exps)
    # both transcript arguments, or neither: refused
    assert L_.bpgpu_rangeproof_verify_rlc_ts_dev(ctx64x8.h, n, m, nb, d_p.data_ptr(), pl, d_c.data_ptr(), group["states"][0], d_t.data_ptr(),
                                                 d_r.data_ptr(), d_w.data_ptr(), d_v.data_ptr(), d_o.data_ptr(), None, None) == -1
    assert L_.bpgpu_rangeproof_verify_rlc_ts_dev(ctx64x8.h, n, m, nb, d_p.data_ptr(), pl, d_c.data_ptr(), None, None, d_r.data_ptr(), d_w.data_ptr(),
                                                 d_v.data_ptr(), d_o.data_ptr(), None, None) == -1
