"""Range proofs of 32 to 1024 parties on the host (big_shapes.py): where each listed shape lies against the capacities of launch 1
(k_rp_stage1_coop), the scripted / 32-lane / byte-wise transcript replays against each other and the oracle, the verification pipeline lane
by lane in the narrow chain's forms, and the oracle's expected values against the Python twin (the C restatement is pinned on the
reference's own vectors only up to m = 8)."""
import ctypes as C
import hashlib

import pytest

import big_shapes as B
import bp_twin as T


@pytest.fixture(scope="module")
def H():
    import harness_lib
    return harness_lib.lib()


def _start_states(n, m):
    """every start state the GPU tests hand the shape: the label's (domain separator applied by the host), three shared padded states and,
    for the shapes of the callers'-transcripts test, the per-proof session states (domain separator applied on the device)"""
    out = [B.label_counts(n, m)]
    out += [B.counts(n, m, B.padded_state(pad)) for pad in ([], [60], [165])]
    if (n, m) in B.TS_SHAPES:
        out += [B.counts(n, m, B.session_state(0, ln)) for ln in B.session_lengths_32_32()]
    return out


def test_listed_shapes_lie_where_launch_1_branches():
    """If a capacity moves, this names the shape to swap: the GPU tests must not silently stop covering a branch.  (A capacity moved by one
    step is noticed where a shape sits on it: RP_COOP_MASKS_CAP at (16, 32) and (32, 32).  No admissible shape has
    8 (9 + 2k) + 8 m = RP_COOP_STAGE_WORDS or 4 + 2k + m = RP_DEFER_CAP, so those two are noticed once they pass a listed shape.)"""
    cap = B.caps()
    assert cap["max_k"] == B.lg(64 * 1024), "(64, 1024) is no longer the documented maximum"
    staged_script = lambda c: c[2] <= cap["ops"] and c[3] <= cap["masks"]
    staged_input = lambda c: c[1] <= cap["stage_words"]
    # the control: everything staged, coefficients parked, from every start state
    for c in _start_states(*B.CONTROL):
        assert staged_script(c) and c[3] < cap["masks"] and staged_input(c) and c[0] <= cap["defer"], ("control", c)
    # (16, 32): the script fills sops to its last mask from every start state
    for c in _start_states(16, 32):
        assert c[3] == cap["masks"] and c[2] <= cap["ops"] and staged_input(c) and c[0] <= cap["defer"], ((16, 32), c)
    # (32, 32): staged or not by the caller's position -- the two session states of the GPU test are one on each side
    lo, hi = (B.counts(32, 32, B.session_state(0, ln)) for ln in B.session_lengths_32_32())
    assert lo[3] == cap["masks"] and hi[3] == cap["masks"] + 1, (lo, hi)
    assert all(staged_input(c) and c[2] <= cap["ops"] and c[0] <= cap["defer"] and cap["masks"] <= c[3] <= cap["masks"] + 1 for c in _start_states(32, 32))
    assert not staged_script(B.label_counts(32, 32))   # (the label calls of the GPU tests take the unstaged script, the proof's bytes staged)
    # (8, 64): nothing staged, coefficients still parked; no smaller m has an unstaged proof
    for c in _start_states(8, 64):
        assert not staged_script(c) and not staged_input(c) and c[0] <= cap["defer"], ((8, 64), c)
    for n in (8, 16, 32, 64):
        assert staged_input(B.label_counts(n, 32)), n
    # (64, 64): the operations alone still fit (at the capacity or a few below, by the position), the masks do not; U below RP_DEFER_CAP
    for c in _start_states(64, 64):
        assert cap["ops"] - 4 <= c[2] <= cap["ops"] + 1 and c[3] > cap["masks"] and not staged_input(c) and c[0] <= cap["defer"], ((64, 64), c)
    assert B.label_counts(64, 64)[2] <= cap["ops"]
    # (8, 128) and up: U beyond RP_DEFER_CAP (the leader recodes), more per-proof points than one column chunk holds many times over
    for s in ((8, 128), (64, 128), (8, 1024), (64, 1024)):
        for c in _start_states(*s):
            assert c[0] > cap["defer"] and not staged_script(c) and not staged_input(c), (s, c)
    assert B.label_counts(8, 1024)[0] > 1000 > 31 * cap["vb_chunk"]
    assert set(B.SHAPES) == {(16, 32), (32, 32), (8, 64), (64, 64), (8, 128), (64, 128), (8, 1024), (64, 1024)}


def _transcript_batch(n, m):
    good, var = B.proofs(n, m), B.variants(n, m)
    items = [good[0], var["t_x"], var["L_last_identity"], var["t_x_blinding_noncanonical"]]
    return b"".join(i[0] for i in items), b"".join(i[1] for i in items)


@pytest.mark.parametrize("n,m", [s for s in B.SHAPES if s != (64, 1024)])
def test_scripted_transcript_equals_bytewise_replay_and_oracle(H, n, m):
    """test_device_code_on_cpu.py's comparison at the large shapes: scripted, 32-lane (with and without parked challenges) and byte-wise
    replay agree lane by lane from the ten paddings, with the domain separator applied on the device or not; the byte-wise path's final
    transcript is oracle.verify_ts's."""
    proofs, coms = _transcript_batch(n, m)
    pl, nb = B.O.proof_len(n, m), 4
    rng = B.rng64(b"ts%d-%d" % (n, m), nb)
    seen_masks = set()
    for pad in B.PADS:
        for domsep in (1, 0):
            st0 = B.padded_state(pad)
            st = st0 if domsep else B.with_domsep(st0, n, m)
            nperm = C.c_uint32(0)
            so, to = C.create_string_buffer(nb), C.create_string_buffer(208 * nb)
            rc = H.h_rp_transcript_compare(n, m, nb, proofs, pl, coms, rng, st, domsep, C.byref(nperm), so, to)
            assert rc == 0, (n, m, pad, domsep, rc)
            assert list(so.raw) == [0, 0, 1, 2]
            assert nperm.value == B.counts(n, m, st, bool(domsep))[3]
            seen_masks.add(nperm.value)
            if domsep:
                ev, _, ets = B.expected_ts(n, m, proofs, coms, st, rng)
                assert list(ev) == [0 if pad == [] else 1, 1, 1, 2]   # (valid on Transcript::new(LABEL) alone; the tampered t_x fails the mega-check only: its transcript runs to the end)
                assert ets == to.raw, (n, m, pad)     # valid, tampered scalar, stopped at the identity L, FormatError (untouched)
    assert len(seen_masks) >= (1 if (n, m) == (16, 32) else 2)


@pytest.mark.parametrize("n,m", [s for s in B.SHAPES if s != (64, 1024)])
def test_scripted_transcript_with_one_start_state_per_proof(H, n, m):
    proofs, coms = _transcript_batch(n, m)
    pl, nb = B.O.proof_len(n, m), 4
    rng = B.rng64(b"pp%d-%d" % (n, m), nb)
    for ln in (5, 41, 150) + B.session_lengths_32_32():
        states = b"".join(B.session_state(b_, ln) for b_ in range(nb))
        so, to = C.create_string_buffer(nb), C.create_string_buffer(208 * nb)
        rc = H.h_rp_transcript_compare_per_proof(n, m, nb, proofs, pl, coms, rng, states, so, to)
        assert rc == 0, (n, m, ln, rc)
        ev, _, ets = B.expected_ts(n, m, proofs, coms, states, rng)
        assert list(so.raw) == [0, 0, 1, 2] and list(ev) == [1, 1, 1, 2]   # (proofs made on another transcript: the replay runs to its end, the check fails)
        assert ets == to.raw and to.raw[208 * 3:] == states[208 * 3:], (n, m, ln)


# (all four forms on three shapes take more than two minutes of host time: all four at (8, 64), the first two at the other shapes)
FORMS = (4, "64+defer_emit+split+hi", "64+split", "a_outside")
PIPELINE = [((16, 32), f) for f in FORMS[:2]] + [((8, 64), f) for f in FORMS] + [((8, 128), f) for f in FORMS[:2]]


@pytest.mark.parametrize("shape,form", PIPELINE)
def test_full_verification_pipeline_lane_by_lane(H, shape, form):
    """rp_transcript -> rp_expand_a/b -> vb_* / fb_* -> finish, emulated lane by lane (test_device_code_on_cpu.py's forms): the quad
    chain; the narrow chain with parked coefficients, split scalar role and second tables; the split scalar role with the leader recoding
    (defer off -- at (8, 128) U > RP_DEFER_CAP turns it off in the first of the two as well); the one-lane chain with A outside.  One valid
    proof, one tampered, one with swapped commitments: verdicts and encodings are the oracle's."""
    n, m = shape
    s = isinstance(form, str)
    H.h_set_defer_emit(1 if s and "defer_emit" in form else 0)
    H.h_set_coop_split(1 if s and "split" in form else 0)
    H.h_set_narrow_hi(2 if s and "+hi" in form else 0)
    H.h_set_radix5(0)
    H.h_set_a_outside(1 if form == "a_outside" else 0)
    H.h_set_horner_lanes(1 if form == "a_outside" else (64 if s else form))
    try:
        good, var = B.proofs(n, m), B.variants(n, m)
        items = [good[1], var["t_x"], var["swapped_commitments"]]
        proofs, coms = b"".join(i[0] for i in items), b"".join(i[1] for i in items)
        rng = B.rng64(b"pipe%d-%d" % (n, m), 3)
        G2, H2, B2, Bb2 = B.gens(n, m).export()
        vd, mo = C.create_string_buffer(3), C.create_string_buffer(96)
        assert H.h_rp_verify(4, 3, n, m, Bb2 + B2 + G2 + H2, n, m, 3, proofs, B.O.proof_len(n, m), coms, B.LABEL, len(B.LABEL), rng, vd, mo) == 0
        ev, em = B.expected(n, m, proofs, coms, rng)
        assert vd.raw == ev and mo.raw == em, (shape, form)
        assert list(ev) == [0, 1, 1] and em[:32] == bytes(32) and em[32:64] != bytes(32) and em[64:] != bytes(32)
    finally:
        H.h_set_a_outside(0)
        H.h_set_defer_emit(0)
        H.h_set_coop_split(0)
        H.h_set_narrow_hi(0)
        H.h_set_horner_lanes(4)


def test_oracle_expected_values_at_64_parties_equal_the_python_twin():
    """bp_twin.verify_multiple (pure Python, written from the reference independently of the C restatement) accepts the C oracle's (8, 64)
    proof and rejects its t_x and swapped-commitment variants, with the encodings the C verifier reports; its multiscalar terms equal
    oracle.verify_terms term for term."""
    n, m = 8, 64
    rng = B.rng64(b"twin", 1)
    c = int.from_bytes(rng, "little") % T.L
    bg, pg = T.BulletproofGens(n, m), T.PedersenGens()
    var = B.variants(n, m)
    for name, (pr, cm) in [("valid", B.proofs(n, m)[0]), ("t_x", var["t_x"]), ("swapped_commitments", var["swapped_commitments"])]:
        vcs = [cm[32 * j:32 * j + 32] for j in range(m)]
        enc = T.verify_multiple(T.RangeProof.from_bytes(pr), bg, pg, T.Transcript(B.LABEL), vcs, n, c)
        erc, eenc = B.O.verify(B.gens_for(n, m), pr, cm, n, B.LABEL, rng)
        assert enc == eenc and (enc == bytes(32)) == (name == "valid") and erc == (0 if name == "valid" else 1), name
        ts, tp = T.verification_msm_terms(T.RangeProof.from_bytes(pr), bg, pg, T.Transcript(B.LABEL), vcs, n, c)
        rc, osc, opt = B.O.verify_terms(B.gens_for(n, m), pr, cm, n, B.LABEL, rng)
        assert rc == 0 and len(ts) == B.O.n_terms(n, m) == len(osc) // 32
        for i, (s_, p_) in enumerate(zip(ts, tp)):
            assert osc[32 * i:32 * i + 32] == s_.to_bytes(32, "little") and opt[32 * i:32 * i + 32] == (p_ if isinstance(p_, bytes) else T.compress(p_)), (name, i)
