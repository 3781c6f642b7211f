"""The launch chains of the seven combined-check host entry points, as bpgpu_profile_report counts them: for each entry point an all-valid
batch of 3 proofs (the combination decides) and the same batch with proof 1 tampered (the per-proof fallback runs behind it), on a context
with profiling on.  {label: launches} is compared with EXPECTED below -- tables recorded by running this module on the commit BEFORE the
host paths of these calls were folded into shared helpers (dev_call, comb_layout / comb_begin / comb_finish, host_call::deliver_combined), so a launch
that such a refactoring drops, doubles or renames shows here.  Shapes are the smallest the families' own modules build: n = 8, generators
(8, 1) -- (8, 2) for the mixed call with its groups m = 1 and m = 2, the R1CS module's own 128 for the k = 1 shuffle --, relation R1 of
sigma_cases.py.  Launch counts only: results are the other modules' business."""
import hashlib
import json

import pytest

import sigma_cases
from test_gpu_ipp_rlc import LABEL as IPP_LABEL, _args as ipp_args, _tamper as ipp_tamper
from test_gpu_r1cs import CAP, _record, _shuffle_gadget, _shuffle_proofs
from test_gpu_rlc_mixed import with_proof

pytestmark = pytest.mark.gpu

NB = 3
BAD = 1

# {case: {"valid": {label: launches}, "fallback": {label: launches}}}, recorded on the parent commit (see the module docstring)
EXPECTED = {
    "rangeproof_verify_rlc": {
        "valid": {"rlc_colsum": 1, "rlc_finish": 1, "rlc_stage3": 1, "rlc_stage4": 1, "rp_stage1": 1},
        "fallback": {"finish1": 1, "rlc_colsum": 1, "rlc_finish": 1, "rlc_stage3": 1, "rlc_stage4": 1, "rp_stage1": 2, "rp_stage3": 1, "rp_stage4": 1},
    },
    "rangeproof_verify_rlc_mixed": {
        "valid": {"fb_walk": 1, "msm_tail": 1, "rlc_mix_front": 2, "rlc_mix_reduce": 1, "rlc_mix_verdict": 1, "rlc_mix_weigh": 2, "vb_prepare": 1,
                  "vb_window": 1},
        "fallback": {"fb_walk": 1, "finish1": 2, "msm_tail": 1, "rlc_mix_front": 2, "rlc_mix_reduce": 1, "rlc_mix_verdict": 1, "rlc_mix_weigh": 2,
                     "rp_stage1": 2, "rp_stage3": 2, "rp_stage4": 2, "vb_prepare": 1, "vb_window": 1},
    },
    "r1cs_verify_rlc": {
        "valid": {"fb_walk": 1, "msm_tail": 1, "r1cs_finish": 1, "r1cs_flatten": 1, "r1cs_front": 1, "r1cs_rlc_reduce": 1, "r1cs_rlc_rho": 1,
                  "r1cs_rlc_sum": 1, "r1cs_rlc_verdict": 1, "r1cs_rlc_weigh": 1, "vb_prepare": 1, "vb_window": 1},
        "fallback": {"fb_walk": 2, "msm_tail": 2, "r1cs_finish": 2, "r1cs_flatten": 2, "r1cs_front": 2, "r1cs_rlc_reduce": 1, "r1cs_rlc_rho": 1,
                     "r1cs_rlc_sum": 1, "r1cs_rlc_verdict": 1, "r1cs_rlc_weigh": 1, "r1cs_verdict": 1, "vb_prepare": 2, "vb_window": 2},
    },
    "linear_verify_rlc": {
        "valid": {"fb_walk": 1, "lin_prepare": 1, "lin_rlc_reduce": 1, "lin_rlc_rho": 1, "lin_rlc_verdict": 1, "lin_rlc_weigh": 1, "msm_tail": 1,
                  "vb_prepare": 1, "vb_window": 1},
        "fallback": {"fb_walk": 2, "lin_prepare": 2, "lin_rlc_reduce": 1, "lin_rlc_rho": 1, "lin_rlc_verdict": 1, "lin_rlc_weigh": 1, "lin_verdict": 1,
                     "msm_tail": 2, "vb_prepare": 2, "vb_window": 2},
    },
    "ipp_verify_rlc": {
        "valid": {"fb_walk": 1, "ipp_rlc_front": 1, "ipp_rlc_reduce": 1, "ipp_rlc_rho": 1, "ipp_rlc_uniq": 1, "ipp_rlc_verdict": 1,
                  "ipp_rlc_weigh": 1, "msm_tail": 1, "vb_prepare": 1, "vb_window": 1},
        "fallback": {"fb_walk": 1, "gather32": 1, "ipp_prepare": 1, "ipp_rlc_front": 1, "ipp_rlc_reduce": 1, "ipp_rlc_rho": 1, "ipp_rlc_uniq": 1,
                     "ipp_rlc_verdict": 1, "ipp_rlc_weigh": 1, "ipp_verdict": 1, "msm_tail": 1, "vb_prepare": 2, "vb_tail": 1, "vb_window": 2},
    },
    "opening_verify_rlc_ts": {
        "valid": {"fb_walk": 1, "msm_tail": 1, "opn_front": 1, "opn_rlc_reduce": 1, "opn_rlc_rho": 1, "opn_rlc_verdict": 1, "opn_rlc_weigh": 1,
                  "vb_prepare": 1, "vb_window": 1},
        "fallback": {"fb_walk": 2, "msm_tail": 2, "opn_front": 2, "opn_rlc_reduce": 1, "opn_rlc_rho": 1, "opn_rlc_verdict": 1, "opn_rlc_weigh": 1,
                     "opn_verdict": 1, "vb_prepare": 2, "vb_window": 2},
    },
    "sigma_verify_rlc_ts": {
        "valid": {"fb_walk": 1, "msm_tail": 1, "sig_front": 1, "sig_rlc_reduce": 1, "sig_rlc_rho": 1, "sig_rlc_verdict": 1, "sig_rlc_weigh": 1,
                  "vb_prepare": 1, "vb_window": 1},
        "fallback": {"fb_walk": 2, "msm_tail": 2, "sig_front": 2, "sig_rlc_reduce": 1, "sig_rlc_rho": 1, "sig_rlc_verdict": 1, "sig_rlc_weigh": 1,
                     "sig_verdict": 1, "vb_prepare": 2, "vb_window": 2},
    },
}


def _flip(raw, plen, b, at, bit=1):
    """`raw` (proofs of plen bytes each) with one bit of proof b flipped at byte `at` (negative: from the proof's end)"""
    p = bytearray(raw)
    p[plen * b + (at % plen)] ^= bit
    return bytes(p)


def _w(tag, n=NB):
    return hashlib.shake_256(b"launch lists " + tag).digest(64 * n)


def _golden(golden, n, m):
    c = next(c for c in golden["cases"] if (c["n"], c["m"]) == (n, m))
    return bytes.fromhex(c["proof"]), golden["vc_bytes"][:32 * m]


@pytest.fixture(scope="module")
def profiled():
    """(gens_capacity, party_capacity) -> a context with profiling on, made once per module"""
    import bulletproofs_amd as bp
    made = {}

    def get(cap, parties):
        if (cap, parties) not in made:
            c = bp.Context(0)
            c.gens_create(cap, parties)
            c.profile_enable()
            made[(cap, parties)] = c
        return made[(cap, parties)]
    yield get
    for c in made.values():
        c.close()


def _launches(ctx, call):
    ctx.synchronize()
    ctx.profile_reset()
    out = call()
    ctx.synchronize()
    return out, {name: cnt for name, (cnt, _) in ctx.profile_report().items()}


def _compare(case, ctx, run):
    """run(tampered) -> batch_ok; both runs' launch tables against EXPECTED[case]"""
    got = {}
    for kind, tampered in (("valid", False), ("fallback", True)):
        ok, got[kind] = _launches(ctx, lambda: run(tampered))
        assert bool(ok) == (not tampered), (case, kind)         # the valid batch is decided by the combination, the other falls back
    print("LAUNCHES %s %s" % (case, json.dumps(got, sort_keys=True)))
    assert got == EXPECTED.get(case)


def test_rangeproof_verify_rlc(profiled, golden):
    ctx = profiled(8, 1)
    proof, com = _golden(golden, 8, 1)
    plen = len(proof)

    def run(tampered):
        proofs = _flip(proof * NB, plen, BAD, 4 * 32) if tampered else proof * NB       # t_x
        verdict, ok, _ = ctx.rangeproof_verify_rlc(8, 1, proofs, plen, com * NB, golden["label"], _w(b"rp rng"), _w(b"rp w"))
        assert verdict[0] == 0 == verdict[2] and (verdict[1] != 0) == tampered
        return ok
    _compare("rangeproof_verify_rlc", ctx, run)


def test_rangeproof_verify_rlc_mixed(profiled, golden):
    ctx = profiled(8, 2)
    p1, c1 = _golden(golden, 8, 1)
    p2, c2 = _golden(golden, 8, 2)
    groups = [(8, 1, p1 * 2, len(p1), c1 * 2, golden["label"]), (8, 2, p2, len(p2), c2, golden["label"])]

    def run(tampered):
        gr = [with_proof(groups[0], BAD, lambda pr: pr.__setitem__(4 * 32, pr[4 * 32] ^ 1)), groups[1]] if tampered else groups
        verdict, ok, _ = ctx.rangeproof_verify_rlc_mixed(gr, _w(b"mix rng"), _w(b"mix w"))
        assert verdict[0] == 0 == verdict[2] and (verdict[1] != 0) == tampered
        return ok
    _compare("rangeproof_verify_rlc_mixed", ctx, run)


def test_r1cs_verify_rlc(profiled, oracle):
    from bulletproofs_amd import r1cs
    ctx = profiled(CAP, 1)
    gens = oracle.Gens(CAP, 1).export()
    ps = _shuffle_proofs(gens, 1, NB)
    circuit = _record(_shuffle_gadget(1), 2, ps[0][2])
    proofs, coms, states = [p.to_bytes() for p, _, _ in ps], b"".join(c for _, c, _ in ps), b"".join(st for _, _, st in ps)
    rng = hashlib.shake_256(b"launch lists r1cs").digest(32 * NB)

    def run(tampered):
        pr = list(proofs)
        if tampered:
            pr[BAD] = _flip(pr[BAD], len(pr[BAD]), 0, 1 + 32 * 8 + 7, 0x10)               # t_x of a one-phase proof
        verdict, batch = r1cs.verify_batch_combined(ctx, [(circuit, pr, coms, states)], rng32=rng, weights64=_w(b"r1cs w"), want_batch=True)
        assert pr[BAD][0] == 0 and verdict[0] == 0 == verdict[2] and (verdict[1] != 0) == tampered, (bytes(verdict), bytes(batch))
        return batch[0] == 0
    _compare("r1cs_verify_rlc", ctx, run)


def test_linear_verify_rlc(profiled, oracle):
    ctx = profiled(8, 1)
    insts = [oracle.linear_test_instance(8, b"launch-lists-%d" % j) for j in range(NB)]
    cat = lambda key: b"".join(i[key] for i in insts)
    plen = len(insts[0]["proof"])

    def run(tampered):
        proofs = _flip(cat("proof"), plen, BAD, -32) if tampered else cat("proof")
        verdict, ok, _ = ctx.linear_verify_rlc(8, proofs, plen, cat("C"), None, None, None, cat("b"), label=insts[0]["label"], weights64=_w(b"lin w"))
        assert verdict[0] == 0 == verdict[2] and (verdict[1] != 0) == tampered
        return ok
    _compare("linear_verify_rlc", ctx, run)


def test_ipp_verify_rlc(profiled, oracle):
    ctx = profiled(8, 1)
    insts = [oracle.ipp_test_instance(8, IPP_LABEL, b"launch-lists-%d" % j) for j in range(NB)]

    def run(tampered):
        ins = [ipp_tamper(i) if tampered and j == BAD else i for j, i in enumerate(insts)]
        verdict, ok, _ = ctx.ipp_verify_rlc(*ipp_args(8, ins, True), label=IPP_LABEL, weights64=_w(b"ipp w"))
        assert verdict[0] == 0 == verdict[2] and (verdict[1] != 0) == tampered
        return ok
    _compare("ipp_verify_rlc", ctx, run)


def test_opening_verify_rlc_ts(profiled, oracle):
    import opening_twin as tw
    ctx = profiled(8, 1)
    B, Bb = tw.bases()
    rows = []
    for i in range(NB):
        v, r = tw.det_scalar(b"ll v", i) % 2**64, tw.det_scalar(b"ll r", i)
        state, Cc = tw.state_at(0, b"ll%d" % i), tw.commit(B, Bb, v, r)
        proof, st, _ = tw.create(state, 0, B, Bb, Cc, v, r, tw.det_seed(b"ll g", i))
        assert st == 0
        rows.append((proof, state, Cc))
    raw, states, Cs = (b"".join(r[k] for r in rows) for k in range(3))

    def run(tampered):
        proofs = _flip(raw, 96, BAD, 96 - 20, 2) if tampered else raw
        verdict, ok, _ = ctx.opening_verify_rlc_ts(0, proofs, 96, states, Cs, weights64=_w(b"opn w"))
        assert verdict[0] == 0 == verdict[2] and (verdict[1] != 0) == tampered
        return ok
    _compare("opening_verify_rlc_ts", ctx, run)


def test_sigma_verify_rlc_ts(profiled, oracle):
    import sigma_twin as tw
    ctx = profiled(8, 1)
    rel = sigma_cases.RELATIONS["R1"]
    rows = sigma_cases.rows(tw, tw.shared_bases(8), "R1", NB, tag=b"launch lists")
    h, S, P, E, _ = ctx.sigma_relation_create(tw.descriptor(rel))
    raw, states, pts = b"".join(r["proof"] for r in rows), b"".join(r["state"] for r in rows), b"".join(b"".join(r["points"]) for r in rows)
    plen = 32 * (E + S)

    def run(tampered):
        proofs = _flip(raw, plen, BAD, 32 * E + 5, 0x10) if tampered else raw             # s_0
        verdict, ok, _ = ctx.sigma_verify_rlc_ts(h, (S, P, E), proofs, states, pts, weights64=_w(b"sig w", NB * E))
        assert verdict[0] == 0 == verdict[2] and (verdict[1] != 0) == tampered
        return ok
    try:
        _compare("sigma_verify_rlc_ts", ctx, run)
    finally:
        ctx.sigma_relation_destroy(h)
