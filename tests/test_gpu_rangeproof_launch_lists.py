"""The launch chains of range-proof verification, as bpgpu_profile_report counts them: every row below is one call on a context with profiling
on, and its {label: launches} is compared with EXPECTED -- a table recorded by running this module on the commit BEFORE the one host function
behind all these calls (rp_verify_dev_locked) became a plan (rp_plan_chain) and one enqueue function per branch, so a launch that such a
refactoring drops, doubles or renames shows here.  The rows are chosen so that every launch site of that function is reached; the comment
beside a row names the sites it is there for.  Inputs are the smallest that reach them: the golden (8, 1) proof replicated (U = 11 points per
proof: one chunk), three proofs of bench_data/cfg3_n64_m16 (U = 40: two chunks per proof, 1024 generator pairs), window tables of 4 bits.
Launch counts only: verdicts are the business of the other modules (some rows verify proofs against transcripts they were not made on)."""
import hashlib
import json

import pytest

pytestmark = pytest.mark.gpu
W = 4
WIDE300 = {"split_stage3": 1}   # (a chain of 300 proofs in the wide forms, as tests/test_gpu_big_shapes.py::WIDE)

# {row: {label: launches}}, recorded on the parent commit (see the module docstring)
EXPECTED = {
    "w1": {"finish8": 1, "rp_stage1": 1, "rp_stage3": 1, "rp_stage4": 1},
    "w1_enc": {"finish8": 1, "rp_stage1": 1, "rp_stage3": 1, "rp_stage4": 1},
    "w7_splits64": {"finish1": 1, "rp_stage1": 1, "rp_stage3": 1, "rp_stage4": 1},
    "w7_splits64_enc": {"finish1": 1, "rp_stage1": 1, "rp_stage3": 1, "rp_stage4": 1},
    "wrong_bitsize": {"rp_stage1": 1, "rp_verdict": 1},
    "w256": {"rp_stage1": 1, "rp_stage3": 1, "rp_stage4": 1},
    "w257": {"fb_reduce": 1, "finish8": 1, "rp_stage1": 1, "rp_stage3": 1, "rp_stage4": 1},
    "w257_enc": {"fb_reduce": 1, "finish8": 1, "rp_stage1": 1, "rp_stage3": 1, "rp_stage4": 1},
    "w257_no_pairs": {"fb_reduce": 1, "finish8": 1, "rp_stage1": 1, "rp_stage3": 1, "rp_stage4": 1},
    "w257_splits65": {"fb_reduce": 1, "finish8": 1, "rp_stage1": 1, "rp_stage3": 1, "rp_stage4": 1},
    "w3_no_script": {"finish8": 1, "rp_stage1": 1, "rp_stage3": 1, "rp_stage4": 1},
    "w3_one_lane": {"fb_reduce": 1, "finish8": 1, "rp_stage1": 1, "rp_stage3": 1, "rp_stage4": 1},
    "w8": {"rp_stage1": 1, "rp_stage3": 1, "rp_stage4": 1},
    "w9_enc": {"finish8": 1, "rp_stage1": 1, "rp_stage3": 1, "rp_stage4": 1},
    "wide_aside": {"finish8": 1, "rp_horner1": 1, "rp_stage1": 1, "rp_stage3": 1, "rp_stage3w": 1, "rp_stage4": 1},
    "wide_aside_a_outside": {"finish8": 1, "rp_horner1": 1, "rp_stage1": 1, "rp_stage3": 1, "rp_stage3w": 1, "rp_stage4": 1},
    "wide_aside_no_pairs": {"finish8": 1, "rp_horner1": 1, "rp_stage1": 1, "rp_stage3": 1, "rp_stage3w": 1, "rp_stage4": 1},
    "wide_aside_radix32": {"finish8": 1, "rp_horner1": 1, "rp_stage1": 1, "rp_stage3": 1, "rp_stage3w": 1, "rp_stage4": 1},
    "wide_auto": {"fb_reduce": 1, "finish8": 1, "rp_stage1": 1, "rp_stage3": 1, "rp_stage3w": 1, "rp_stage4": 1},
    "wide_auto_no_pairs": {"fb_reduce": 1, "finish8": 1, "rp_stage1": 1, "rp_stage3": 1, "rp_stage3w": 1, "rp_stage4": 1},
    "wide_quads": {"fb_reduce": 1, "finish8": 1, "rp_stage1": 1, "rp_stage3": 1, "rp_stage3w": 1, "rp_stage4": 1},
    "wide_wave": {"fb_reduce": 1, "finish8": 1, "rp_stage1": 1, "rp_stage3": 1, "rp_stage3w": 1, "rp_stage4": 1},
    "malformed_length": {},
    "mixed_positions": {"finish8": 1, "rp_stage1": 1, "rp_stage3": 1, "rp_stage4": 1},
    "cfg3_narrow": {"finish8": 1, "rp_stage1": 1, "rp_stage3": 1, "rp_stage4": 1},
    "cfg3_quads": {"fb_reduce": 2, "finish8": 1, "rp_stage1": 1, "rp_stage3": 1, "rp_stage4": 1, "vb_colsum": 1},
    "cfg3_wide_aside": {"finish8": 1, "rp_horner1": 1, "rp_stage1": 1, "rp_stage3": 1, "rp_stage3w": 1, "rp_stage4": 1, "vb_colsum": 1},
    "rlc_bucket_w3": {"bk_heavy": 1, "bk_leaf": 1, "bk_sort": 1, "bk_tree": 1, "rlc_accum": 1, "rlc_finish": 1, "rlc_stage3": 1, "rlc_stage4": 1, "rp_stage1": 1},
    "rlc_bucket_w3_no_result": {"bk_heavy": 1, "bk_leaf": 1, "bk_sort": 1, "bk_tree": 1, "rlc_accum": 1, "rlc_finish": 1, "rlc_stage3": 1, "rlc_stage4": 1, "rp_stage1": 1},
    "rlc_w130": {"rlc_colsum": 2, "rlc_finish": 1, "rlc_stage3": 1, "rlc_stage4": 1, "rp_stage1": 1},
    "rlc_w3": {"rlc_colsum": 1, "rlc_finish": 1, "rlc_stage3": 1, "rlc_stage4": 1, "rp_stage1": 1},
    "rlc_w3_no_result": {"rlc_colsum": 1, "rlc_finish": 1, "rlc_stage3": 1, "rlc_stage4": 1, "rp_stage1": 1},
    "rlc_w9": {"rlc_colsum": 1, "rlc_finish": 1, "rlc_stage3": 1, "rlc_stage4": 1, "rp_stage1": 1},
    "pool_two_labels": {"finish8": 1, "rp_stage1": 1, "rp_stage3": 1, "rp_stage4": 1},
}


def _rng(tag, nb):
    return hashlib.shake_256(b"rp launch lists " + tag).digest(64 * nb)


@pytest.fixture(scope="module")
def contexts():
    """(capacity, options) -> a context with profiling on, made once per module"""
    import bulletproofs_amd as bp
    made = {}

    def get(capacity=(8, 1), **options):
        key = (capacity, tuple(sorted(options.items())))
        if key not in made:
            c = bp.Context(0, fixed_window_bits=W)
            for k, v in options.items():
                c.set_option(k, v)
            c.gens_create(*capacity)
            c.profile_enable()
            made[key] = c
        return made[key]
    yield get
    for c in made.values():
        c.close()


def _launches(ctx, call):
    ctx.synchronize()
    ctx.profile_reset()
    call()
    ctx.synchronize()
    return {name: cnt for name, (cnt, _) in ctx.profile_report().items()}


def _compare(row, got):
    print("LAUNCHES %s %s" % (row, json.dumps(got, sort_keys=True)))
    assert got == EXPECTED.get(row), row


@pytest.fixture(scope="module")
def small(golden):
    """the golden (8, 1) proof, its commitment, the label"""
    c = next(c for c in golden["cases"] if (c["n"], c["m"]) == (8, 1))
    return bytes.fromhex(c["proof"]), golden["vc_bytes"][:32], golden["label"]


@pytest.fixture(scope="module")
def cfg3():
    from bulletproofs_amd import workload as wl
    fx = wl.load_fixture("cfg3_n64_m16")
    return fx, wl.tile_batch(fx, 3)


def _batch(ctx, small, nb, want_msm=False, n=8, cut=0):
    proof, com, label = small
    proof = proof[:len(proof) - cut]
    return _launches(ctx, lambda: ctx.rangeproof_verify_batch(n, 1, proof * nb, len(proof), com * nb, label, _rng(b"batch", nb), want_msm=want_msm))


# ---- per-proof chains of the (8, 1) proof: (options, width, encodings wanted) ----------------------------------------------------------
PER_PROOF = {
    # k_rp_stage1_coop with second to fourth tables, k_rp_stage3<2>, k_rp_stage4<64> (narrow walk: four partial sums per proof), k_finish8<false>
    "w1": ({}, 1, False),
    # k_finish8<true>
    "w1_enc": ({}, 1, True),
    # two partial sums per proof: k_finish1<false>, k_finish1<true>
    "w7_splits64": ({"fixed_splits": 64}, 7, False),
    "w7_splits64_enc": ({"fixed_splits": 64}, 7, True),
    # the fused finish: no finish launch
    "w8": ({}, 8, False),
    # encodings wanted: no fused finish; two table levels
    "w9_enc": ({}, 9, True),
    # the last width of the narrow forms
    "w256": ({}, 256, False),
    # k_rp_stage1<true>, k_rp_stage3<1>, k_rp_stage4<4> with its Horner quads, a reduction launch in front of the finish (more than 64 partial sums)
    "w257": ({}, 257, False),
    "w257_enc": ({}, 257, True),
    # k_rp_stage3<0>
    "w257_no_pairs": ({"exponent_pairs": 0}, 257, False),
    # 65 partial sums per proof: the smallest count with a reduction launch
    "w257_splits65": ({"fixed_splits": 65}, 257, False),
    # k_rp_stage4<1>: quads' place taken by one lane per chain
    "w3_one_lane": ({"horner_lanes": 1}, 3, False),
    # k_rp_stage1<false>: byte-wise replay by option
    "w3_no_script": ({"transcript_script": 0}, 3, False),
    # wide: k_vb_window_colc, k_rp_exponents<true>, k_rp_stage4<4>
    "wide_auto": (dict(WIDE300, horner_lanes=0), 300, True),
    # wide, Horner chains aside: k_rp_horner1, k_rp_stage4<4> without a Horner role
    "wide_aside": (dict(WIDE300, horner_lanes=1, a_outside=0), 300, True),
    # ... with A outside: k_vb_window_wide<false>, k_rp_horner_wide<false>
    "wide_aside_a_outside": (dict(WIDE300, horner_lanes=1, a_outside=1), 300, True),
    "wide_quads": (dict(WIDE300, horner_lanes=4), 300, True),
    # wide with a wavefront per chain: the last k_rp_stage4<64> form (thread = proof walk)
    "wide_wave": (dict(WIDE300, horner_lanes=64), 300, True),
    # k_rp_exponents<false>
    "wide_auto_no_pairs": (dict(WIDE300, horner_lanes=0, exponent_pairs=0), 300, True),
    "wide_aside_no_pairs": (dict(WIDE300, horner_lanes=1, exponent_pairs=0), 300, True),
    # radix 32: k_vb_window_wide<true>, k_rp_horner_wide<true>
    "wide_aside_radix32": (dict(WIDE300, horner_lanes=1, per_proof_radix=32), 300, True),
}


@pytest.mark.parametrize("row", sorted(PER_PROOF))
def test_per_proof_chain(contexts, small, row):
    options, nb, want_msm = PER_PROOF[row]
    _compare(row, _batch(contexts(**options), small, nb, want_msm))


def test_malformed_length(contexts, small):
    """every proof 32 bytes short: memsets, no launch"""
    _compare("malformed_length", _batch(contexts(), small, 3, cut=32))


def test_wrong_bitsize(contexts, small):
    """the shape-verdict tail: k_rp_stage1<false> (transcripts only), k_rp_verdict"""
    _compare("wrong_bitsize", _batch(contexts(), small, 3, n=12))


def test_caller_transcripts_at_mixed_positions(contexts, small):
    """one state per proof, at differing STROBE positions: k_rp_stage1<false>"""
    from bulletproofs_amd._lib import transcript_new, transcript_append_message
    ctx = contexts()
    proof, com, _ = small
    nb = 3
    states = b"".join(transcript_append_message(transcript_new(b"launch lists"), b"pad", bytes(3 + 29 * i)) for i in range(nb))
    assert len({states[208 * i + 200] for i in range(nb)}) == nb
    _compare("mixed_positions", _launches(ctx, lambda: ctx.rangeproof_verify_batch_ts(8, 1, proof * nb, len(proof), com * nb, states, _rng(b"ts", nb))))


# ---- the proofs with two chunks of points and 1024 generator pairs ------------------------------------------------------------------------
CFG3 = {
    # Horner quads on more than one chunk per proof: k_vb_colsum in front of launch 4
    "cfg3_quads": {"horner_lanes": 4},
    # wide, chains aside, window sums through chunks: k_vb_colsum on the way to k_rp_horner1; k_rp_exponents_w3
    "cfg3_wide_aside": dict(WIDE300, horner_lanes=1, a_outside=0),
    # narrow chain of an aggregated shape
    "cfg3_narrow": {},
}


@pytest.mark.parametrize("row", sorted(CFG3))
def test_two_chunk_chain(contexts, cfg3, row):
    fx, (proofs, coms) = cfg3
    ctx = contexts(capacity=(64, 16), **CFG3[row])
    _compare(row, _launches(ctx, lambda: ctx.rangeproof_verify_batch(fx.n, fx.m, proofs, fx.proof_len, coms, fx.label, _rng(b"cfg3", 3), want_msm=True)))


# ---- the combined check -----------------------------------------------------------------------------------------------------------------
# (options, width, 33-byte result wanted); all proofs valid: the combination decides, nothing falls back
COMBINED = {
    # column-sum tree: <= 8 rows, the coefficient reduction alone in its launch; k_rp_stage4<64> for one MSM; k_rlc_finish<true>
    "rlc_w3": ({}, 3, True),
    # k_rlc_finish<false>
    "rlc_w3_no_result": ({}, 3, False),
    # 9 rows: the last tree level shares its launch with the coefficient reduction
    "rlc_w9": ({}, 9, True),
    # 130 rows: a 16-way level (k_fb_reduce) first
    "rlc_w130": ({}, 130, True),
    # 33 terms above bucket_min_terms = 16: the bucket form (sort, k_rlc_accum_scalars, k_bk_heavy, reduce, k_rlc_stage4b), k_rlc_finish<true> / <false>
    "rlc_bucket_w3": ({"bucket_min_terms": 16}, 3, True),
    "rlc_bucket_w3_no_result": ({"bucket_min_terms": 16}, 3, False),
}


@pytest.mark.parametrize("row", sorted(COMBINED))
def test_combined_check(contexts, small, row):
    import torch
    import bulletproofs_amd as bp
    options, nb, want_result = COMBINED[row]
    ctx = contexts(**options)
    proof, com, label = small
    if want_result:
        def call():
            verdict, ok, _ = ctx.rangeproof_verify_rlc(8, 1, proof * nb, len(proof), com * nb, label, _rng(b"rlc", nb), _rng(b"rlc w", nb))
            assert ok and verdict == bytes(nb)
    else:   # only the device-pointer call can do without the result
        dev = torch.device("cuda", 0)
        to_dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
        d_p, d_c, d_r, d_w = to_dev(proof * nb), to_dev(com * nb), to_dev(_rng(b"rlc", nb)), to_dev(_rng(b"rlc w", nb))
        d_v = torch.full((nb,), 255, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def call():
            assert bp.lib().bpgpu_rangeproof_verify_rlc_dev(ctx.h, 8, 1, nb, d_p.data_ptr(), len(proof), d_c.data_ptr(), label, len(label), d_r.data_ptr(),
                                                            d_w.data_ptr(), d_v.data_ptr(), None, None) == 0
            ctx.synchronize()
            assert d_v.cpu().tolist() == [0] * nb
    _compare(row, _launches(ctx, call))


# ---- one coalesced chain of the pool ------------------------------------------------------------------------------------------------------
def test_coalesced_chain_of_two_labels(small):
    """two submitted items whose labels differ, one chain: the start states of both labels staged ahead of launch 1"""
    import torch
    import bulletproofs_amd as bp
    proof, com, _ = small
    nb = 2
    dev = torch.device("cuda", 0)
    to_dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    pool = bp.Pool((0,), 2, fixed_window_bits=W)
    try:
        pool.gens_create(8, 1)
        pool.profile_enable()
        d_p, d_c, d_r = to_dev(proof * nb), to_dev(com * nb), to_dev(_rng(b"pool", nb))
        d_v = [torch.full((nb,), 255, dtype=torch.uint8, device=dev) for _ in range(2)]
        torch.cuda.synchronize()
        pool.set_option("stat_reset", 1)
        pool.profile_reset()
        for i, label in enumerate((b"launch lists A", b"launch lists B")):
            pool.submit_dev(0, 8, 1, nb, d_p.data_ptr(), len(proof), d_c.data_ptr(), label, d_r.data_ptr(), d_v[i].data_ptr())
        pool.wait()
        assert pool.get_option("stat_chains") == 1 and pool.get_option("stat_chain_proofs") == 2 * nb
        _compare("pool_two_labels", {name: cnt for name, (cnt, _) in pool.profile_report().items()})
    finally:
        pool.close()
