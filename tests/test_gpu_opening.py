"""Proofs of knowledge of commitment openings on the GPU (bpgpu_opening_*, OpeningProof, BulletproofGens.prove_balance /
verify_balance_proved, bulletproofs.hpp) against tests/opening_twin.py.
CONTRACTS (include/bpgpu.h): (a) a row's msm_out equals bpgpu_msm_batch on (s_v, B), (s_r, B_blinding), (l - c, C), (l - 1, R) with c from
bpgpu_transcript_batch; (b) verdict and transcripts_out of the _rlc_ts call always equal those of _verify_batch_ts; (c) a created
proof verifies and both sides leave one state.  Batches have 1, 2, 63, 64, 65 and 130 proofs: lane 0 alone, the workgroup edge, and the
combined check's rounding of the batch to 64."""
import hashlib
import os
import subprocess

import pytest

import point_corpus as corpus

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1
SIZES = [1, 2, 63, 64, 65, 130]
NB = 130
TAMPERED = (0, 63, 64, NB - 1)
POSITIONS = (0, 100, 150, 165)
TS = 208
FIXED_W = 9


@pytest.fixture(scope="module")
def tw(oracle):
    import opening_twin
    return opening_twin


@pytest.fixture(scope="module")
def contexts():
    """(fixed_window_bits or None, prover_constant_time) -> a context with gens_create(8, 1), made once per module"""
    import bulletproofs_amd as bp
    made = {}

    def get(W=None, ct=0):
        if (W, ct) not in made:
            ctx = bp.Context(0, fixed_window_bits=W) if W else bp.Context(0)
            if ct:
                ctx.set_option("prover_constant_time", 1)
            ctx.gens_create(8, 1)
            made[(W, ct)] = ctx
        return made[(W, ct)]
    yield get
    for ctx in made.values():
        ctx.close()


@pytest.fixture(scope="module")
def ref(tw):
    """Per form: 130 statements (u64 values 0, 1, 2^64 - 1 and others, one state per proof over four STROBE positions), the twin's
    proofs and end states, computed once and left unchanged; `shared`: the twin's proofs when every row starts from rows[0]'s state"""
    B, Bb = tw.bases()
    special = [0, 1, 2**64 - 1]
    out = {"B": B, "Bb": Bb}
    for form in (0, 1):
        rows, shared = [], []
        for i in range(NB):
            v = special[i] if i < 3 else tw.det_scalar(b"v", i) % 2**64
            r = tw.L - 1 if i == 3 else tw.det_scalar(b"r%d" % form, i)
            state = tw.state_at(POSITIONS[i % 4], b"s%d" % (i % 7))
            Cc = tw.commit(B, Bb, v, r)
            seed = tw.det_seed(b"g%d" % form, i)
            proof, st, so = tw.create(state, form, B, Bb, Cc, v, r, seed)
            assert st == 0
            rows.append(dict(state=state, v=v, r=r, C=Cc, seed=seed, proof=proof, out=so))
        for i in range(NB):
            r = rows[i]
            shared.append(tw.create(rows[0]["state"], form, B, Bb, r["C"], r["v"], r["r"], r["seed"]))
        out[form] = dict(rows=rows, shared=shared)
    return out


def _col(rows, key, n=None):
    rows = rows if n is None else rows[:n]
    return b"".join(r[key] for r in rows)


def _vals(rows, vb, n=None):
    rows = rows if n is None else rows[:n]
    return b"".join(r["v"].to_bytes(vb, "little") for r in rows)


def _bl(rows, n=None):
    rows = rows if n is None else rows[:n]
    return b"".join(r["r"].to_bytes(32, "little") for r in rows)


def _split(b, n):
    return [b[n * i:n * i + n] for i in range(len(b) // n)]


# ---- creation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", SIZES)
@pytest.mark.parametrize("form", [0, 1])
def test_created_proofs_are_the_twins_bytes(contexts, ref, form, nb):
    """u64 and 32-byte values, one state per proof; default W, one fixed_window_bits value, prover_constant_time on: the same bytes,
    status OK, the twin's end states.  A shared state (stride 0) on the default context."""
    rows = ref[form]["rows"]
    pl = 96 if form == 0 else 64
    want_p, want_t = _col(rows, "proof", nb), _col(rows, "out", nb)
    for key in ((None, 0), (None, 1), (FIXED_W, 0)):
        ctx = contexts(*key)
        for vb in (8, 32):
            proofs, st, ts = ctx.opening_create_batch_ts(form, _col(rows, "state", nb), _col(rows, "C", nb), _vals(rows, vb, nb), vb, _bl(rows, nb),
                                                         rng32=_col(rows, "seed", nb), want_transcripts=True)
            assert st == bytes(nb), (key, vb)
            assert _split(proofs, pl) == _split(want_p, pl), (key, vb)
            assert ts == want_t, (key, vb)
    sh = ref[form]["shared"][:nb]
    proofs, st, ts = contexts().opening_create_batch_ts(form, rows[0]["state"], _col(rows, "C", nb), _vals(rows, 8, nb), 8, _bl(rows, nb),
                                                        rng32=_col(rows, "seed", nb), want_transcripts=True)
    assert (proofs, st, ts) == (b"".join(s[0] for s in sh), bytes(nb), b"".join(s[2] for s in sh))


@pytest.mark.parametrize("form", [0, 1])
def test_scalar_values_and_rejected_rows(contexts, tw, ref, form):
    """32-byte values 0, 1, 2^64 - 1, l - 1; a value of l or 2^256 - 1, a blinding of l: status 2, zero bytes, the input state, the
    neighbours untouched -- in a batch of 66 that puts rejected rows at the workgroup edge (63, 64)"""
    B, Bb = ref["B"], ref["Bb"]
    nb = 66
    base = ref[form]["rows"][:nb]
    vals = [r["v"] for r in base]
    rs = [r["r"] for r in base]
    vals[0:4] = [0, 1, 2**64 - 1, tw.L - 1]
    vals[5], vals[63] = tw.L, 2**256 - 1
    rs[64], rs[7] = tw.L, 2**256 - 1
    rows = [dict(state=b["state"], seed=b["seed"], v=v, r=r, C=(tw.commit(B, Bb, v % tw.L, r % tw.L) if i < 4 else b["C"])) for i, (b, v, r) in enumerate(zip(base, vals, rs))]
    want = [tw.create(r["state"], form, B, Bb, r["C"], r["v"], r["r"], r["seed"]) for r in rows]
    pl = 96 if form == 0 else 64
    for key in ((None, 0), (None, 1)):
        proofs, st, ts = contexts(*key).opening_create_batch_ts(form, _col(rows, "state"), _col(rows, "C"), b"".join(v.to_bytes(32, "little") for v in vals), 32,
                                                                b"".join(r.to_bytes(32, "little") for r in rs), rng32=_col(rows, "seed"), want_transcripts=True)
        assert _split(proofs, pl) == [w[0] for w in want] and list(st) == [w[1] for w in want] and _split(ts, TS) == [w[2] for w in want]
        for i in (5, 7, 63, 64):
            assert st[i] == tw.BAD_SCALAR and proofs[pl * i:pl * i + pl] == bytes(pl) and ts[TS * i:TS * i + TS] == rows[i]["state"]
        assert sum(st) == 4 * tw.BAD_SCALAR
    if form == 1:   # no value buffer: every value is 0
        zero = [dict(r, v=0, C=tw.commit(B, Bb, 0, r["r"])) for r in base[:3]]
        proofs, st, ts = contexts().opening_create_batch_ts(1, _col(zero, "state"), _col(zero, "C"), None, 8, _bl(zero), rng32=_col(zero, "seed"), want_transcripts=True)
        want = [tw.create(r["state"], 1, B, Bb, r["C"], 0, r["r"], r["seed"]) for r in zero]
        assert (proofs, st, ts) == (b"".join(w[0] for w in want), bytes(3), b"".join(w[2] for w in want))


def test_library_drawn_seeds_give_proofs_that_verify(contexts, ref):
    """rng32 = NULL: the seeds come from the OS; the proofs differ from the seeded ones and verify (contract c without a fixed seed)"""
    rows = ref[0]["rows"][:5]
    ctx = contexts()
    proofs, st, ts = ctx.opening_create_batch_ts(0, _col(rows, "state"), _col(rows, "C"), _vals(rows, 8), 8, _bl(rows), want_transcripts=True)
    assert st == bytes(5) and proofs != _col(rows, "proof")
    v, ts2 = ctx.opening_verify_batch_ts(0, proofs, 96, _col(rows, "state"), _col(rows, "C"), want_transcripts=True)
    assert v == bytes(5) and ts2 == ts


# ---- verification -----------------------------------------------------------------------------------------------------------------
def _verify_both(ctx, form, proofs, states, Cs, values, vb=8, weights64=None):
    """the per-proof and the combined call on the same inputs -> ((verdict, msm_out, transcripts), (verdict, batch_ok, batch point, transcripts))"""
    pl = 96 if form == 0 else 64
    a = ctx.opening_verify_batch_ts(form, proofs, pl, states, Cs, values, vb, want_msm=True, want_transcripts=True)
    b = ctx.opening_verify_rlc_ts(form, proofs, pl, states, Cs, values, vb, weights64=weights64, want_transcripts=True)
    return a, b


@pytest.mark.parametrize("nb", SIZES)
@pytest.mark.parametrize("form", [0, 1])
def test_created_proofs_verify_and_both_sides_end_in_one_state(contexts, ref, form, nb):
    """contract (c) through both verifiers, at every batch size; msm_out of a proof that verifies is the identity's encoding"""
    rows = ref[form]["rows"]
    ctx = contexts()
    values = _vals(rows, 8, nb) if form == 1 else None
    a, b = _verify_both(ctx, form, _col(rows, "proof", nb), _col(rows, "state", nb), _col(rows, "C", nb), values)
    assert a == (bytes(nb), bytes(32 * nb), _col(rows, "out", nb))
    assert b == (bytes(nb), True, bytes(32), _col(rows, "out", nb))
    if nb > 1:   # ... and from one shared state
        sh = ref[form]["shared"][:nb]
        a, b = _verify_both(ctx, form, b"".join(s[0] for s in sh), rows[0]["state"], _col(rows, "C", nb), values)
        assert a[0] == b[0] == bytes(nb) and a[2] == b[3] == b"".join(s[2] for s in sh)


@pytest.mark.parametrize("form", [0, 1])
def test_msm_out_is_the_four_term_msm_with_the_challenge_of_the_transcript_script(contexts, tw, ref, form):
    """contract (a) on every row of the 130-row batch, a third of them with one bit of a response flipped so that the check is not the
    identity: c from bpgpu_transcript_batch running the header's script, then bpgpu_msm_batch on (s_v, B), (s_r, B~), (l - c, C), (l - 1, R)"""
    from bulletproofs_amd.api import TranscriptBatch
    rows = ref[form]["rows"]
    ctx = contexts()
    B, Bb = ref["B"], ref["Bb"]
    pl = 96 if form == 0 else 64
    proofs = []
    for i, r in enumerate(rows):
        p = bytearray(r["proof"])
        if i % 3 == 0:
            p[pl - 32 + (i % 31)] ^= 1 << (i % 8)      # (a byte below the top one: the response stays canonical)
        proofs.append(bytes(p))
    verdict, msm_out, _ = ctx.opening_verify_batch_ts(form, b"".join(proofs), pl, _col(rows, "state"), _col(rows, "C"), _vals(rows, 8) if form == 1 else None, 8,
                                                      want_msm=True, want_transcripts=True)
    tb = TranscriptBatch.from_states(ctx, _col(rows, "state"))
    tb.append_message(b"dom-sep", b"openingproof v1")
    tb.append_u64(b"form", form)
    tb.append_message(b"C", [r["C"] for r in rows])
    if form == 1:
        tb.append_message(b"v", [r["v"].to_bytes(32, "little") for r in rows])
    tb.append_message(b"R", [p[:32] for p in proofs])
    cs = [int.from_bytes(c, "little") for c in tb.challenge_scalars(b"c")]
    sc, pt = b"", b""
    for r, p, c in zip(rows, proofs, cs):
        s_r = int.from_bytes(p[-32:], "little")
        s_v = int.from_bytes(p[32:64], "little") if form == 0 else c * r["v"] % tw.L
        sc += b"".join(tw.le32(x) for x in (s_v, s_r, (tw.L - c) % tw.L, tw.L - 1))
        pt += B + Bb + r["C"] + p[:32]
    out, st = ctx.msm_batch([4] * NB, sc, pt)
    assert st == bytes(NB)
    assert _split(msm_out, 32) == _split(out, 32)
    assert [v for v in verdict] == [1 if (i % 3 == 0) else 0 for i in range(NB)]
    assert all((out[32 * i:32 * i + 32] == bytes(32)) == (i % 3 != 0) for i in range(NB))


def _reject_members():
    return corpus.one_per_class()


def _tampers(tw, form):
    """name -> f(row dict copy, its proof as a bytearray, a neighbour row): one tamper class each"""
    def bit(lo):
        def f(row, p, other):
            p[lo + 5] ^= 0x08
        return f

    def c_bit(row, p, other):
        row["C"] = row["C"][:9] + bytes([row["C"][9] ^ 0x10]) + row["C"][10:]

    def v_plus_one(row, p, other):
        row["v"] += 1

    def session(row, p, other):
        row["state"] = other["state"]

    def s_r_is_l(row, p, other):
        p[-32:] = tw.le32(tw.L)

    def r_zero(row, p, other):
        p[:32] = bytes(32)

    t = {"R bit": bit(0), "s_r bit": bit(64 if form == 0 else 32), "C bit": c_bit, "wrong session": session, "s_r = l": s_r_is_l, "R zero": r_zero}
    if form == 0:
        t["s_v bit"] = bit(32)
    else:
        t["v + 1"] = v_plus_one
    for cls, enc in _reject_members():
        def in_r(row, p, other, enc=enc):
            p[:32] = enc

        def in_c(row, p, other, enc=enc):
            row["C"] = enc
        t["R fails " + cls] = in_r
        t["C fails " + cls] = in_c
    return t


TAMPER_NAMES = {0: ["R bit", "s_v bit", "s_r bit", "C bit", "wrong session", "s_r = l", "R zero"] + [w + c for c in "CNQTY" for w in ("R fails ", "C fails ")],
                1: ["R bit", "s_r bit", "C bit", "v + 1", "wrong session", "s_r = l", "R zero"] + [w + c for c in "CNQTY" for w in ("R fails ", "C fails ")]}


@pytest.mark.parametrize("form,name", [(f, n) for f in (0, 1) for n in TAMPER_NAMES[f]])
def test_each_tamper_class_alone_through_both_verifiers(contexts, tw, ref, form, name):
    """rows 0, 63, 64 and 129 of an otherwise valid batch: the exact verdict and transcripts_out of the twin from the per-proof call and
    from the combined call, the other rows untouched"""
    B, Bb = ref["B"], ref["Bb"]
    rows = [dict(r) for r in ref[form]["rows"]]
    proofs = [bytearray(r["proof"]) for r in rows]
    f = _tampers(tw, form)[name]
    for i in TAMPERED:
        f(rows[i], proofs[i], ref[form]["rows"][(i + 1) % NB if i + 1 < NB else 1])
    proofs = [bytes(p) for p in proofs]
    want_v, want_t = bytearray(NB), [r["out"] for r in rows]
    for i in TAMPERED:
        want_v[i], want_t[i], _ = tw.verify(rows[i]["state"], form, B, Bb, proofs[i], rows[i]["C"], rows[i]["v"])
    assert all(want_v[i] != 0 for i in TAMPERED), name
    if name in ("s_r = l",):
        assert all(want_v[i] == tw.FORMAT_ERROR and want_t[i] == rows[i]["state"] for i in TAMPERED)
    if name == "R zero":
        assert all(want_v[i] == tw.VERIFICATION_ERROR and want_t[i] not in (rows[i]["state"], rows[i]["out"]) for i in TAMPERED)
    a, b = _verify_both(contexts(), form, b"".join(proofs), _col(rows, "state"), _col(rows, "C"), _vals(rows, 32) if form == 1 else None, 32)
    assert a[0] == bytes(want_v) and _split(a[2], TS) == want_t
    assert b[0] == bytes(want_v) and _split(b[3], TS) == want_t
    assert b[1] == (name in ("s_r = l", "R zero"))      # rows that stopped in the front end do not enter the combination: it is the identity


def test_a_public_value_that_is_not_canonical_is_a_format_error(contexts, tw, ref):
    rows = ref[1]["rows"][:3]
    vals = [rows[0]["v"], tw.L, rows[2]["v"]]
    a, b = _verify_both(contexts(), 1, _col(rows, "proof"), _col(rows, "state"), _col(rows, "C"), b"".join(v.to_bytes(32, "little") for v in vals), 32)
    want_t = rows[0]["out"] + rows[1]["state"] + rows[2]["out"]
    assert a[0] == b[0] == bytes([0, tw.FORMAT_ERROR, 0]) and a[2] == b[3] == want_t


# ---- the combined check ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("failing", ["none", "all", "row 0", "row 64", "last row"])
def test_combined_check_equals_the_per_proof_check(contexts, tw, ref, form, failing):
    """contract (b); batch_out[0] is 0 exactly when every combined row verifies; the _dev form marks UNDECIDED where the host form falls
    back to the per-proof path"""
    import torch
    rows = ref[form]["rows"]
    pl = 96 if form == 0 else 64
    bad = {"none": [], "all": list(range(NB)), "row 0": [0], "row 64": [64], "last row": [NB - 1]}[failing]
    proofs = [bytearray(r["proof"]) for r in rows]
    for i in bad:
        proofs[i][pl - 20] ^= 2
    proofs = b"".join(bytes(p) for p in proofs)
    values = _vals(rows, 8) if form == 1 else None
    ctx = contexts()
    w64 = hashlib.shake_256(b"opening weights " + failing.encode()).digest(64 * NB)
    a, b = _verify_both(ctx, form, proofs, _col(rows, "state"), _col(rows, "C"), values, weights64=w64)
    want = bytes(1 if i in bad else 0 for i in range(NB))
    assert a[0] == b[0] == want and a[2] == b[3] == _col(rows, "out")
    assert b[1] == (not bad) and (b[2] == bytes(32)) == (not bad)
    # the _dev form: the same batch point for the same weights, UNDECIDED where R is not the identity
    dev = torch.device("cuda:0")
    up = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)
    d_pr, d_ts, d_c, d_w = up(proofs), up(_col(rows, "state")), up(_col(rows, "C")), up(w64)
    d_val = up(values) if values is not None else None
    d_v, d_bo, d_to = (torch.full((n,), 255, dtype=torch.uint8, device=dev) for n in (NB, 33, TS * NB))
    torch.cuda.synchronize()
    ctx.opening_verify_rlc_ts_dev(form, NB, d_pr.data_ptr(), pl, None, d_ts.data_ptr(), d_c.data_ptr(), d_val.data_ptr() if d_val is not None else None, 8,
                                  d_w.data_ptr(), d_v.data_ptr(), d_bo.data_ptr(), d_to.data_ptr())
    ctx.synchronize()
    bo = bytes(d_bo.cpu().numpy())
    assert bytes(d_v.cpu().numpy()) == (bytes(NB) if not bad else bytes([tw.UNDECIDED]) * NB)
    assert bo[0] == (1 if bad else 0) and bo[1:33] == b[2] and bytes(d_to.cpu().numpy()) == _col(rows, "out")
    # ... and the per-proof _dev form agrees with the host form
    d_v2, d_m = torch.full((NB,), 255, dtype=torch.uint8, device=dev), torch.full((32 * NB,), 255, dtype=torch.uint8, device=dev)
    ctx.opening_verify_batch_ts_dev(form, NB, d_pr.data_ptr(), pl, None, d_ts.data_ptr(), d_c.data_ptr(), d_val.data_ptr() if d_val is not None else None, 8,
                                    d_v2.data_ptr(), d_m.data_ptr(), None)
    ctx.synchronize()
    assert bytes(d_v2.cpu().numpy()) == want and bytes(d_m.cpu().numpy()) == a[1]


@pytest.mark.parametrize("form", [0, 1])
def test_equal_weights_give_one_batch_point_for_a_shared_state_and_for_its_copies(contexts, ref, form):
    """a batch with one failing proof, so that the batch point is not the identity: stride 0 and nbatch copies of the state agree byte
    for byte; without weights64 the library draws them and two calls differ"""
    rows = ref[form]["rows"]
    sh = ref[form]["shared"]
    nb, pl = 65, 96 if form == 0 else 64
    proofs = bytearray(b"".join(s[0] for s in sh[:nb]))
    proofs[pl * 64 + pl - 9] ^= 1
    proofs = bytes(proofs)
    ctx = contexts()
    w64 = hashlib.shake_256(b"equal weights").digest(64 * nb)
    values = _vals(rows, 8, nb) if form == 1 else None
    one = ctx.opening_verify_rlc_ts(form, proofs, pl, rows[0]["state"], _col(rows, "C", nb), values, 8, weights64=w64, want_transcripts=True)
    many = ctx.opening_verify_rlc_ts(form, proofs, pl, rows[0]["state"] * nb, _col(rows, "C", nb), values, 8, weights64=w64, want_transcripts=True)
    assert one == many and one[1] is False and one[2] != bytes(32) and one[0] == bytes(64) + b"\x01"
    d1 = ctx.opening_verify_rlc_ts(form, proofs, pl, rows[0]["state"], _col(rows, "C", nb), values, 8)
    d2 = ctx.opening_verify_rlc_ts(form, proofs, pl, rows[0]["state"], _col(rows, "C", nb), values, 8)
    assert d1[0] == d2[0] == one[0] and d1[2] != d2[2]


def test_argument_checks_on_a_real_context(contexts, ref):
    """a form other than 0 or 1, a proof_len that is not the form's, a value_bytes other than 8 or 32, values in form 0: INVALID_ARG,
    the outputs untouched; the empty batch is OK"""
    import ctypes as C
    ctx = contexts()
    L = ctx._L
    rows = ref[0]["rows"][:1]
    pr, ts, cm = rows[0]["proof"], rows[0]["state"], rows[0]["C"]
    vd = C.create_string_buffer(b"\x5a", 1)
    for form, pl in ((2, 96), (-1, 64), (0, 64), (1, 96), (0, 95), (0, 0)):
        assert L.bpgpu_opening_verify_batch_ts(ctx.h, form, 1, pr, pl, ts, 0, cm, None, 8, vd, None, None) == INVALID_ARG, (form, pl)
        assert L.bpgpu_opening_verify_rlc_ts(ctx.h, form, 1, pr, pl, ts, 0, cm, None, 8, None, vd, None, None) == INVALID_ARG, (form, pl)
        assert L.bpgpu_opening_verify_rlc_ts_dev(ctx.h, form, 1, 256, pl, ts, None, 512, None, 8, None, 768, None, None, None) == INVALID_ARG, (form, pl)
    out, st = C.create_string_buffer(b"\x5a" * 96, 96), C.create_string_buffer(b"\x5a", 1)
    assert L.bpgpu_opening_create_batch_ts(ctx.h, 2, 1, ts, 0, None, cm, bytes(8), 8, bytes(32), out, st, None) == INVALID_ARG
    assert L.bpgpu_opening_create_batch_ts(ctx.h, 0, 1, ts, 0, None, cm, bytes(8), 16, bytes(32), out, st, None) == INVALID_ARG
    assert L.bpgpu_opening_create_batch_ts(ctx.h, 0, 1, ts, 0, None, cm, None, 8, bytes(32), out, st, None) == INVALID_ARG
    assert L.bpgpu_opening_create_batch_ts(ctx.h, 0, 1, ts, 100, None, cm, bytes(8), 8, bytes(32), out, st, None) == INVALID_ARG
    assert L.bpgpu_opening_verify_batch_ts(ctx.h, 0, 1, pr, 96, ts, 0, cm, bytes(8), 8, vd, None, None) == INVALID_ARG
    bad_state = ts[:200] + bytes([200]) + ts[201:]
    assert L.bpgpu_opening_verify_batch_ts(ctx.h, 0, 1, pr, 96, bad_state, 0, cm, None, 8, vd, None, None) == INVALID_ARG
    assert vd.raw == b"\x5a" and out.raw == b"\x5a" * 96 and st.raw == b"\x5a"
    bo = C.create_string_buffer(b"\x5a" * 33, 33)
    assert L.bpgpu_opening_verify_rlc_ts(ctx.h, 0, 0, None, 96, ts, 0, None, None, 8, None, None, bo, None) == 0 and bo.raw == bytes(33)
    assert L.bpgpu_opening_create_batch_ts(ctx.h, 1, 0, ts, 0, None, None, None, 8, None, None, None, None) == 0


# ---- composition ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gens():
    import bulletproofs_amd as bp
    g = bp.BulletproofGens(8, 1)
    yield g
    g.ctx.close()


def _block(gens, tw, fees):
    """rows of 2 inputs and 2 outputs whose values differ by the row's fee -> (inputs, outputs, excess blindings)"""
    inputs, outputs, excess = [], [], []
    for i, fee in enumerate(fees):
        v_out = [5 + i, 7]
        v_in = [fee // 2 + 5 + i + fee % 2, fee // 2 + 7]
        bl = [tw.det_scalar(b"block", 4 * i + k) for k in range(4)]
        coms, _ = gens.commit_batch(v_in + v_out, [tw.le32(b) for b in bl])
        inputs.append(coms[:2])
        outputs.append(coms[2:])
        excess.append(tw.le32((bl[0] + bl[1] - bl[2] - bl[3]) % tw.L))
    return inputs, outputs, excess


def test_prove_balance_then_verify_balance_proved(gens, tw):
    """fees 0 and 2^64 - 1 (and two more rows); the verifier sees commitments, fees and proofs only.  A fee off by one is rejected, alone.
    The twin verifies the same proofs against E_r = sum(in) - sum(out) - fee B."""
    import bulletproofs_amd as bp
    fees = [0, 2**64 - 1, 3, 1000]
    inputs, outputs, excess = _block(gens, tw, fees)
    mk = lambda: [_session(bp, i) for i in range(len(fees))]
    tp, tv, tx = mk(), mk(), mk()
    proofs = gens.prove_balance(fees, excess, tp, inputs, outputs, rng_seed32=b"".join(tw.det_seed(b"bal", i) for i in range(len(fees))))
    assert all(p.serialized_size() == 64 for p in proofs)
    assert gens.verify_balance_proved(inputs, outputs, fees, proofs, tv) == [None] * len(fees)
    assert [t.state for t in tv] == [t.state for t in tp]
    B, Bb = tw.bases()
    for i, fee in enumerate(fees):
        E = tw.msm([1, 1, tw.L - 1, tw.L - 1, tw.L - fee], inputs[i] + outputs[i] + [B])
        assert E == tw.commit(B, Bb, 0, int.from_bytes(excess[i], "little"))
        assert tw.verify(_session(bp, i).state, 1, B, Bb, proofs[i].to_bytes(), E, 0)[0] == 0
    wrong = list(fees)
    wrong[1] -= 1
    res = gens.verify_balance_proved(inputs, outputs, wrong, proofs, tx)
    assert res[0] is None and res[2] is None and res[3] is None and res[1] == bp.VerificationError()
    # a TranscriptBatch in place of the list; a shared transcript for every row
    tb = bp.TranscriptBatch.from_states(gens, mk())
    assert gens.verify_balance_proved(inputs, outputs, fees, proofs, tb) == [None] * len(fees) and tb.states() == b"".join(t.state for t in tp)
    one = _session(bp, 99)
    shared = gens.prove_balance(fees, excess, one, inputs, outputs)
    assert gens.verify_balance_proved(inputs, outputs, fees, shared, one) == [None] * len(fees)
    # a row with an input that does not decode has no key: never verified
    broken = [list(r) for r in inputs]
    broken[2][0] = b"\xff" * 32
    res = gens.verify_balance_proved(broken, outputs, fees, proofs, mk())
    assert res[2] == bp.VerificationError() and res[0] is None and res[1] is None and res[3] is None


def _session(bp, i):
    t = bp.Transcript(b"opening proofs")
    t.append_u64(b"session", i)
    return t


@pytest.mark.parametrize("public", [False, True])
def test_opening_proof_class(gens, tw, public):
    """create_batch with commitments=None makes them with commit_batch; verify_batch and verify_batch_combined give None per proof and
    leave lists and a TranscriptBatch advanced alike; one-proof create / verify raise ProofError"""
    import bulletproofs_amd as bp
    n = 5
    values = [0, 1, 2**64 - 1, 77, 12345]
    blindings = [tw.le32(tw.det_scalar(b"cls", i)) for i in range(n)]
    seeds = b"".join(tw.det_seed(b"cls", i) for i in range(n))
    mk = lambda: [_session(bp, i) for i in range(n)]
    tp, tv, tc = mk(), mk(), mk()
    proofs, coms = bp.OpeningProof.create_batch(gens, tp, values, blindings, public_values=public, rng_seed32=seeds)
    B, Bb = tw.bases()
    for i in range(n):
        want = tw.create(_session(bp, i).state, int(public), B, Bb, coms[i], values[i], int.from_bytes(blindings[i], "little"), seeds[32 * i:32 * i + 32])
        assert (proofs[i].to_bytes(), tp[i].state) == (want[0], want[2])
    pv = values if public else None
    assert bp.OpeningProof.verify_batch(gens, tv, proofs, coms, pv) == [None] * n
    assert bp.OpeningProof.verify_batch_combined(gens, tc, proofs, coms, pv) == [None] * n
    assert [t.state for t in tv] == [t.state for t in tc] == [t.state for t in tp]
    tb = bp.TranscriptBatch(gens, b"opening proofs", n)
    tb.append_u64(b"session", list(range(n)))
    assert bp.OpeningProof.verify_batch_combined(gens, tb, proofs, coms, pv) == [None] * n and tb.states() == b"".join(t.state for t in tp)
    # the wrong public value / the wrong commitment: rejected alone
    swapped = list(coms)
    swapped[1], swapped[2] = swapped[2], swapped[1]
    res = bp.OpeningProof.verify_batch_combined(gens, mk(), proofs, swapped, pv)
    assert res == [None, bp.VerificationError(), bp.VerificationError(), None, None]
    # one proof
    t1, t2 = _session(bp, 3), _session(bp, 3)
    p = bp.OpeningProof.create(gens, t1, values[3], blindings[3], coms[3], public_value=public, rng_seed32=seeds[96:128])
    assert p.to_bytes() == proofs[3].to_bytes()
    p.verify(gens, t2, coms[3], values[3] if public else None)
    assert t1.state == t2.state
    with pytest.raises(bp.ProofError):
        p.verify(gens, _session(bp, 4), coms[3], values[3] if public else None)
    with pytest.raises(bp.FormatError):
        bp.OpeningProof.from_bytes(p.to_bytes()[:-32] + tw.le32(tw.L))
    with pytest.raises(ValueError):
        bp.OpeningProof.create_batch(gens, mk()[:1], [1], [tw.le32(tw.L)], commitments=coms[:1])


def test_cpp_mirror_has_the_class(tmp_path):
    """include/bulletproofs.hpp: OpeningProof, BulletproofGens::prove_balance / verify_balance_proved"""
    exe, csrc = str(tmp_path / "opening_proof_test"), os.path.join(ROOT, "bulletproofs_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "opening_proof_test.cpp"),
                           "-L", csrc, "-lbpgpu", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout
