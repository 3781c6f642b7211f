"""Inner-product and linear proofs on the callers' own transcripts (bpgpu_ipp_*_ts, bpgpu_linear_*_ts): every proof of a batch starts from
its own Merlin state, before innerproduct_domain_sep(n), at whatever STROBE position its session left it.  The contracts (include/bpgpu.h):
  C1  row p of a _ts call == the existing entry point with nbatch = 1 and shared_transcript = transcripts[p];
  C2  transcript_stride = 0 == the existing entry point on the whole batch with that shared_transcript, byte for byte;
  C3  verdict and transcripts_out of an _rlc_ts call == those of the _verify_batch_ts call;
  C4  the inner-product transcripts_out is what verification_scalars leaves in the reference's `&mut Transcript` (oracle twin).
Proofs come from the existing create calls with nbatch = 1 on each state."""
import ctypes as C
import hashlib
import os
import random
import subprocess

import pytest

from test_ipp_linear_ts_on_cpu import ELL, _bound, _le, _starts, _state_of, _wrap_item

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS = 208
INVALID_ARG = -1
OK, VERIFICATION, FORMAT, UNDECIDED = 0, 1, 2, 5
NB = 65                                       # one full workgroup of RP_BLOCK = 64 lanes plus one more
DAMAGED = {5: "noncanonical", 17: "identity", 40: "flip", 64: "undecodable"}
BOTH = pytest.mark.parametrize("fixed", [False, True], ids=["explicit", "table"])
SHAPES = pytest.mark.parametrize("n,nb", [(n, nb) for n in (2, 8, 64) for nb in (1, 3, NB)])


@pytest.fixture(scope="module")
def ctx():
    import bulletproofs_amd as bp
    c = bp.Context(0)
    c.gens_create(64, 1)
    yield c
    c.close()


def _four_starts(n):
    """fresh, bound, and two bound ones whose separator wraps the 166-byte rate inside `dom-sep` resp. inside `n` (oracle-twin transcripts)"""
    fresh, wrap1, wrap2 = _starts(n)
    plain = next(t for t in (_bound(length) for length in range(3, 400)) if _wrap_item(t, n) == 0)
    return [fresh, plain, wrap1, wrap2]


def _keystream(seed, nblocks):
    from chacha_rng import ChaChaRng
    return ChaChaRng(seed).fill_bytes(64 * nblocks)


def _rand_scalars(rnd, count):
    return [rnd.randrange(ELL) for _ in range(count)]


def _damage(proof, kind, k, a_off):
    pr = bytearray(proof)
    if kind == "noncanonical":
        pr[a_off:a_off + 32] = b"\xff" * 32
    elif kind == "identity":
        j = min(1, k - 1)
        pr[64 * j:64 * j + 32] = bytes(32)                      # L_1 (L_0 where there is one round only)
    elif kind == "flip":
        pr[a_off + 3] ^= 0x10
    elif kind == "undecodable":
        pr[32:64] = b"\xff" * 32                                # R_0: no Ristretto encoding
    return bytes(pr)


# ---- the rows: 65 statements per size, each with its own start state, seed and proof -------------------------------------------------------
_cache = {}


def _lin_rows(ctx, oracle, n):
    key = ("lin", n)
    if key in _cache:
        return _cache[key]
    k = n.bit_length() - 1
    Gall, _, Bp, Bb = ctx.gens_export()
    G, F, B = Gall[:32 * n], Bp, Bb                              # linear_proof.rs:405-411
    starts = _four_starts(n)
    rows = []
    for j in range(NB):
        rnd = random.Random("lin-%d-%d" % (n, j))
        a, b, r = _rand_scalars(rnd, n), _rand_scalars(rnd, n), rnd.randrange(ELL)
        c = sum(x * y for x, y in zip(a, b)) % ELL
        rcm, Cc = oracle.msm(b"".join(_le(x) for x in a) + _le(r) + _le(c), G + B + F)
        assert rcm == 0
        seed = hashlib.shake_256(b"lin-seed-%d-%d" % (n, j)).digest(32)
        t0 = starts[j % 4]
        row = dict(a=b"".join(_le(x) for x in a), b=b"".join(_le(x) for x in b), r=_le(r), C=Cc, seed=seed, rng=_keystream(seed, 2 * k + 2), t0=t0,
                   st=_state_of(t0), a_int=a, b_int=b, r_int=r)
        proofs, status, ts = ctx.linear_create_batch(n, Cc, row["r"], row["a"], row["b"], G, F, B, transcript=row["st"], rng=row["rng"], want_transcripts=True)
        assert status == bytes(1)
        row.update(proof=proofs, ts_created=ts)
        rows.append(row)
    _cache[key] = dict(n=n, k=k, G=G, F=F, B=B, rows=rows, pl=32 * (2 * k + 3), a_off=64 * k + 32)
    return _cache[key]


def _ipp_rows(ctx, oracle, n):
    key = ("ipp", n)
    if key in _cache:
        return _cache[key]
    k = n.bit_length() - 1
    Gall, Hall, _, _ = ctx.gens_export()
    G, H = Gall[:32 * n], Hall[:32 * n]
    starts = _four_starts(n)
    rows = []
    for j in range(NB):
        rnd = random.Random("ipp-%d-%d" % (n, j))
        a, b, gf, hf = (_rand_scalars(rnd, n) for _ in range(4))
        c = sum(x * y for x, y in zip(a, b)) % ELL
        Q = oracle.ipp_test_instance(2, b"q", b"ipp-q-%d-%d" % (n, j))["Q"]
        rcm, P = oracle.msm(b"".join(_le(x * g) for x, g in zip(a, gf)) + b"".join(_le(y * h) for y, h in zip(b, hf)) + _le(c), G + H + Q)
        assert rcm == 0
        t0 = starts[j % 4]
        row = dict(a=b"".join(_le(x) for x in a), b=b"".join(_le(x) for x in b), Gf=b"".join(_le(x) for x in gf), Hf=b"".join(_le(x) for x in hf), Q=Q, P=P,
                   t0=t0, st=_state_of(t0), gf_int=gf, hf_int=hf)
        proofs, status = ctx.ipp_create_batch(n, Q, row["Gf"], row["Hf"], G, H, row["a"], row["b"], transcript=row["st"])
        assert status == bytes(1)
        row["proof"] = proofs
        rows.append(row)
    _cache[key] = dict(n=n, k=k, G=G, H=H, rows=rows, pl=32 * (2 * k + 2), a_off=64 * k)
    return _cache[key]


def _batch(d, nb, damaged=None):
    """the first nb rows; `damaged`: {row: kind} (default: one row of each kind in a batch of 65, none in smaller ones)"""
    if damaged is None:
        damaged = DAMAGED if nb == NB else {}
    rows = []
    for j, row in enumerate(d["rows"][:nb]):
        if j in damaged:
            row = dict(row, proof=_damage(row["proof"], damaged[j], d["k"], d["a_off"]))
        rows.append(row)
    return rows


def _cat(rows, key):
    return b"".join(r[key] for r in rows)


# ---- what the reference leaves in each transcript (oracle twin, transcript operations only) -------------------------------------------------
def _lin_ts_want(d, row):
    key = ("lin-ts", d["n"], row["st"], row["proof"], row["C"], row["b"])
    if key not in _cache:
        _cache[key] = _lin_ts_twin(d, row)
    return _cache[key]


def _lin_ts_twin(d, row):
    """bpgpu_linear_verify_batch's documented transcripts_out for shared_transcript = the row's own state: after x_star for a proof that
    reaches the final check, the state right behind innerproduct_domain_sep(n) otherwise"""
    n, k, pr = d["n"], d["k"], row["proof"]
    t = row["t0"].clone()
    t.innerproduct_domain_sep(n)
    behind = _state_of(t)
    if any(int.from_bytes(pr[o:o + 32], "little") >= ELL for o in (64 * k + 32, 64 * k + 64)):
        return behind
    t.append_message(b"C", row["C"])
    for i in range(n):
        t.append_message(b"b_i", row["b"][32 * i:32 * i + 32])
    for i in range(n):
        t.append_message(b"G_i", d["G"][32 * i:32 * i + 32])
    t.append_message(b"F", d["F"])
    t.append_message(b"B", d["B"])
    for j in range(k):
        if pr[64 * j:64 * j + 32] == bytes(32) or pr[64 * j + 32:64 * j + 64] == bytes(32):
            return behind
        t.append_message(b"L", pr[64 * j:64 * j + 32])
        t.append_message(b"R", pr[64 * j + 32:64 * j + 64])
        t.challenge_bytes(b"x_j", 64)
    t.append_message(b"S", pr[64 * k:64 * k + 32])
    t.challenge_bytes(b"x_star", 64)
    return _state_of(t)


def _ipp_ts_want(d, row):
    """C4: the transcript after InnerProductProof::from_bytes(proof)?.verification_scalars(n, &mut transcript) (ipp.rs:203-222)"""
    import bp_twin as T
    n, k, pr = d["n"], d["k"], row["proof"]
    t = row["t0"].clone()
    p = T.RangeProof()
    p.L_vec = [pr[64 * i:64 * i + 32] for i in range(k)]
    p.R_vec = [pr[64 * i + 32:64 * i + 64] for i in range(k)]
    try:
        p.a, p.b = T._canonical_scalar(pr[64 * k:64 * k + 32]), T._canonical_scalar(pr[64 * k + 32:])
        T.verification_scalars(p, n, t)
    except T.ProofError:
        pass
    return _state_of(t)


def _ipp_twin_verify(d, row):
    """(code, compress(expect_P - P) or None) of the twin's InnerProductProof::verify on the row's own transcript"""
    import bp_twin as T
    n = d["n"]
    dec = lambda b: [T.decompress(b[32 * i:32 * i + 32]) for i in range(len(b) // 32)]
    try:
        em = T.ipp_verify(row["proof"], n, row["t0"].clone(), row["gf_int"], row["hf_int"], T.decompress(row["P"]), T.decompress(row["Q"]), dec(d["G"]), dec(d["H"]))
    except T.FormatError:
        return FORMAT, None
    except T.VerificationError:
        return VERIFICATION, None
    return (OK if em == bytes(32) else VERIFICATION), em


# ---- device-pointer helpers ---------------------------------------------------------------------------------------------------------------
def _dev():
    import torch
    return torch.device("cuda", 0)


def _to_dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(_dev())


def _filled(nbytes):
    import torch
    return torch.full((max(nbytes, 1),), 0x5a, dtype=torch.uint8, device=_dev())


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _raw(t, nbytes):
    return bytes(t.cpu().numpy())[:nbytes]


def _ipp_existing(ctx, d, rows, state):
    """bpgpu_ipp_verify_batch_dev (the existing call that takes a shared_transcript) on `rows` with bases given once: (verdict, msm_out)"""
    import bulletproofs_amd as bp
    import torch
    L = bp.lib()
    nb = len(rows)
    bufs = [_to_dev(_cat(rows, key)) for key in ("proof", "Gf", "Hf", "P", "Q")]
    d_g, d_h = _to_dev(d["G"]), _to_dev(d["H"])
    d_v, d_o = _filled(nb), _filled(32 * nb)
    torch.cuda.synchronize()
    rc = L.bpgpu_ipp_verify_batch_dev(ctx.h, d["n"], nb, bufs[0].data_ptr(), d["pl"], None, 0, state, bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(),
                                      bufs[4].data_ptr(), d_g.data_ptr(), d_h.data_ptr(), 1, d_v.data_ptr(), d_o.data_ptr(), None)
    assert rc == 0
    ctx.synchronize()
    return _raw(d_v, nb), _raw(d_o, 32 * nb)


def _weights(tag, nb):
    return hashlib.shake_256(b"ipl-ts-weights-" + tag).digest(64 * nb)


def _expected_batch_ok(verdict):
    """the combination holds every proof that reaches the final check: it is the identity iff none of them fails there (a proof stopped in the
    front end -- FormatError, an identity L_j / R_j -- is left out)"""
    return all(v in (OK, FORMAT) or kind == "identity" for v, kind in verdict)


# ============================================================================================================================================
# C1, C3, C4: one state per proof
# ============================================================================================================================================
@BOTH
@SHAPES
def test_linear_verify_on_one_transcript_per_proof(ctx, oracle, n, nb, fixed):
    d = _lin_rows(ctx, oracle, n)
    rows = _batch(d, nb)
    bases = (None, None, None) if fixed else (d["G"], d["F"], d["B"])
    states, w = _cat(rows, "st"), _weights(b"lin-%d-%d" % (n, nb), nb)
    args = (n, _cat(rows, "proof"), d["pl"], states, _cat(rows, "C")) + bases + (_cat(rows, "b"),)
    verdict, msm, ts = ctx.linear_verify_batch_ts(*args, want_msm=True, want_transcripts=True)
    v2, ok, enc, ts2 = ctx.linear_verify_rlc_ts(*args, weights64=w, want_transcripts=True)
    assert v2 == verdict and ts2 == ts                                                             # C3
    for p, row in enumerate(rows):
        one = ctx.linear_verify_batch(n, row["proof"], d["pl"], row["C"], *bases, row["b"], transcript=row["st"], want_msm=True, want_transcripts=True)
        assert one == (verdict[p:p + 1], msm[32 * p:32 * p + 32], ts[TS * p:TS * (p + 1)]), p      # C1
        code, em = oracle.linear_verify(n, row["proof"], row["st"], row["C"], d["G"], d["F"], d["B"], row["b"])
        assert verdict[p] == code, p
        if em != b"\xff" * 32 and code != FORMAT:
            assert msm[32 * p:32 * p + 32] == em, p
        assert ts[TS * p:TS * (p + 1)] == _lin_ts_want(d, row), p
    kinds = DAMAGED if nb == NB else {}
    assert list(verdict) == [{"noncanonical": FORMAT, "identity": VERIFICATION, "flip": VERIFICATION, "undecodable": VERIFICATION}.get(kinds.get(p), OK) for p in range(nb)]
    assert ok == _expected_batch_ok([(verdict[p], kinds.get(p)) for p in range(nb)])
    # the prover left each transcript where the verifier leaves it
    assert all(ts[TS * p:TS * (p + 1)] == rows[p]["ts_created"] for p in range(nb) if p not in kinds)
    # one public vector for all: b_shared
    if nb == 3:
        shared = dict(rows[0])
        got = ctx.linear_verify_batch_ts(n, _cat(rows, "proof"), d["pl"], states, _cat(rows, "C"), *bases, shared["b"], want_transcripts=True)
        assert got[0][0] == OK and got[0][1] == VERIFICATION and got[0][2] == VERIFICATION
        for p, row in enumerate(rows):
            one = ctx.linear_verify_batch(n, row["proof"], d["pl"], row["C"], *bases, shared["b"], transcript=row["st"], want_transcripts=True)
            assert one == (got[0][p:p + 1], got[1][TS * p:TS * (p + 1)]), p


@BOTH
@SHAPES
def test_inner_product_verify_on_one_transcript_per_proof(ctx, oracle, n, nb, fixed):
    d = _ipp_rows(ctx, oracle, n)
    rows = _batch(d, nb)
    states, w = _cat(rows, "st"), _weights(b"ipp-%d-%d" % (n, nb), nb)
    cat = lambda key: _cat(rows, key)
    verdict, msm, ts = ctx.ipp_verify_batch_ts(n, cat("proof"), d["pl"], states, cat("Gf"), cat("Hf"), cat("P"), cat("Q"), d["G"], d["H"], want_msm=True,
                                               want_transcripts=True)
    v2, ok, enc, ts2 = ctx.ipp_verify_rlc_ts(n, cat("proof"), d["pl"], states, cat("Gf"), cat("Hf"), cat("P"), cat("Q"), None if fixed else d["G"],
                                             None if fixed else d["H"], gens_m=1, weights64=w, want_transcripts=True)
    assert v2 == verdict and ts2 == ts                                                             # C3
    kinds = DAMAGED if nb == NB else {}
    twin_rows = set(range(nb)) if n < 64 or nb < NB else set(kinds) | {0, 1, 2, 3}
    for p, row in enumerate(rows):
        one = _ipp_existing(ctx, d, [row], row["st"])
        assert one == (verdict[p:p + 1], msm[32 * p:32 * p + 32]), p                               # C1
        assert ts[TS * p:TS * (p + 1)] == _ipp_ts_want(d, row), p                                  # C4
        if p in twin_rows:
            code, em = _ipp_twin_verify(d, row)
            assert verdict[p] == code, p
            if em is not None:
                assert msm[32 * p:32 * p + 32] == em, p
    assert list(verdict) == [{"noncanonical": FORMAT, "identity": VERIFICATION, "flip": VERIFICATION, "undecodable": VERIFICATION}.get(kinds.get(p), OK) for p in range(nb)]
    assert ok == _expected_batch_ok([(verdict[p], kinds.get(p)) for p in range(nb)])
    # C4 spelled out for the damaged rows
    if nb == NB:
        by = {kind: p for p, kind in kinds.items()}
        p = by["noncanonical"]
        assert ts[TS * p:TS * (p + 1)] == rows[p]["st"]                                            # from_bytes: the input state
        p = by["identity"]
        t = rows[p]["t0"].clone()
        t.innerproduct_domain_sep(n)
        for j in range(min(1, d["k"] - 1)):
            t.append_message(b"L", rows[p]["proof"][64 * j:64 * j + 32])
            t.append_message(b"R", rows[p]["proof"][64 * j + 32:64 * j + 64])
            t.challenge_bytes(b"u", 64)
        assert ts[TS * p:TS * (p + 1)] == _state_of(t)                                             # as of the identity point, nothing of it in
    # n != 2^lg_n: VerificationError, every state handed back as it came (the reference returns before the separator)
    if nb == 3:
        bad = ctx.ipp_verify_batch_ts(2 * n, cat("proof"), d["pl"], states, cat("Gf") * 2, cat("Hf") * 2, cat("P"), cat("Q"), d["G"] * 2, d["H"] * 2,
                                      want_transcripts=True)
        assert bad == (bytes([VERIFICATION]) * nb, states)
        bad = ctx.ipp_verify_rlc_ts(2 * n, cat("proof"), d["pl"], states, cat("Gf") * 2, cat("Hf") * 2, cat("P"), cat("Q"), d["G"] * 2, d["H"] * 2,
                                    weights64=w, want_transcripts=True)
        assert (bad[0], bad[3]) == (bytes([VERIFICATION]) * nb, states)
        # bases per proof (bases_shared = 0): the same rows
        got = ctx.ipp_verify_batch_ts(n, cat("proof"), d["pl"], states, cat("Gf"), cat("Hf"), cat("P"), cat("Q"), d["G"] * nb, d["H"] * nb, want_msm=True,
                                      want_transcripts=True)
        assert got == (verdict, msm, ts)


# ============================================================================================================================================
# C3: the three batches the combined checks meet
# ============================================================================================================================================
@BOTH
@pytest.mark.parametrize("case", ["all-valid", "one-bad", "one-front-end-reject"])
def test_combined_checks_agree_with_the_per_proof_calls(ctx, oracle, case, fixed):
    n, nb = 8, NB
    damaged = {"all-valid": {}, "one-bad": {33: "flip"}, "one-front-end-reject": {64: "noncanonical"}}[case]
    want_ok = case != "one-bad"
    w = _weights(case.encode(), nb)
    d = _lin_rows(ctx, oracle, n)
    rows = _batch(d, nb, damaged)
    bases = (None, None, None) if fixed else (d["G"], d["F"], d["B"])
    args = (n, _cat(rows, "proof"), d["pl"], _cat(rows, "st"), _cat(rows, "C")) + bases + (_cat(rows, "b"),)
    verdict, ts = ctx.linear_verify_batch_ts(*args, want_transcripts=True)
    v2, ok, enc, ts2 = ctx.linear_verify_rlc_ts(*args, weights64=w, want_transcripts=True)
    assert (v2, ts2) == (verdict, ts) and ok is want_ok and (enc == bytes(32)) is want_ok
    assert [p for p in range(nb) if verdict[p]] == sorted(damaged)
    d = _ipp_rows(ctx, oracle, n)
    rows = _batch(d, nb, damaged)
    cat = lambda key: _cat(rows, key)
    verdict, ts = ctx.ipp_verify_batch_ts(n, cat("proof"), d["pl"], cat("st"), cat("Gf"), cat("Hf"), cat("P"), cat("Q"), d["G"], d["H"], want_transcripts=True)
    v2, ok, enc, ts2 = ctx.ipp_verify_rlc_ts(n, cat("proof"), d["pl"], cat("st"), cat("Gf"), cat("Hf"), cat("P"), cat("Q"), None if fixed else d["G"],
                                             None if fixed else d["H"], weights64=w, want_transcripts=True)
    assert (v2, ts2) == (verdict, ts) and ok is want_ok and (enc == bytes(32)) is want_ok
    assert [p for p in range(nb) if verdict[p]] == sorted(damaged)


# ============================================================================================================================================
# C2: one state for every proof
# ============================================================================================================================================
@pytest.fixture(scope="module")
def shared8(ctx, oracle):
    """65 statements at n = 8 proved on ONE bound state (its separator wraps the rate inside `n`) by the existing calls on the whole batch"""
    n = 8
    lin, ipp = _lin_rows(ctx, oracle, n), _ipp_rows(ctx, oracle, n)
    st = _state_of(_four_starts(n)[3])
    lr, ir = lin["rows"], ipp["rows"]
    lp = ctx.linear_create_batch(n, _cat(lr, "C"), _cat(lr, "r"), _cat(lr, "a"), _cat(lr, "b"), lin["G"], lin["F"], lin["B"], transcript=st, rng=_cat(lr, "rng"),
                                 want_transcripts=True)
    ip = ctx.ipp_create_batch(n, _cat(ir, "Q"), _cat(ir, "Gf"), _cat(ir, "Hf"), ipp["G"], ipp["H"], _cat(ir, "a"), _cat(ir, "b"), transcript=st)
    assert lp[1] == bytes(NB) and ip[1] == bytes(NB)
    return dict(n=n, st=st, lin=lin, ipp=ipp, lin_created=lp, ipp_created=ip)


@pytest.mark.parametrize("nb", [3, NB])
def test_stride_0_equals_the_existing_calls_on_the_shared_state(ctx, shared8, nb):
    s = shared8
    n, st, lin, ipp = s["n"], s["st"], s["lin"], s["ipp"]
    # the two provers
    lr, ir = lin["rows"][:nb], ipp["rows"][:nb]
    got = ctx.linear_create_batch_ts(n, st, _cat(lr, "C"), _cat(lr, "r"), _cat(lr, "a"), _cat(lr, "b"), lin["G"], lin["F"], lin["B"], rng32=_cat(lr, "seed"),
                                     want_transcripts=True)
    assert ctx.get_option("staging_residue") == 0
    assert got == (s["lin_created"][0][:lin["pl"] * nb], bytes(nb), s["lin_created"][2][:TS * nb])
    got = ctx.ipp_create_batch_ts(n, st, _cat(ir, "Q"), _cat(ir, "Gf"), _cat(ir, "Hf"), ipp["G"], ipp["H"], _cat(ir, "a"), _cat(ir, "b"), want_transcripts=True)
    assert got[:2] == (s["ipp_created"][0][:ipp["pl"] * nb], bytes(nb))
    # the verifiers, with one damaged row of each kind in the batch of 65
    kinds = DAMAGED if nb == NB else {}
    w = _weights(b"shared-%d" % nb, nb)
    lproofs = b"".join(_damage(s["lin_created"][0][lin["pl"] * p:lin["pl"] * (p + 1)], kinds.get(p), lin["k"], lin["a_off"]) for p in range(nb))
    iproofs = b"".join(_damage(s["ipp_created"][0][ipp["pl"] * p:ipp["pl"] * (p + 1)], kinds.get(p), ipp["k"], ipp["a_off"]) for p in range(nb))
    for bases in ((lin["G"], lin["F"], lin["B"]), (None, None, None)):
        a = ctx.linear_verify_batch_ts(n, lproofs, lin["pl"], st, _cat(lr, "C"), *bases, _cat(lr, "b"), want_msm=True, want_transcripts=True)
        b = ctx.linear_verify_batch(n, lproofs, lin["pl"], _cat(lr, "C"), *bases, _cat(lr, "b"), transcript=st, want_msm=True, want_transcripts=True)
        assert a == b and [p for p in range(nb) if a[0][p]] == sorted(kinds)
        a = ctx.linear_verify_rlc_ts(n, lproofs, lin["pl"], st, _cat(lr, "C"), *bases, _cat(lr, "b"), weights64=w, want_transcripts=True)
        b = ctx.linear_verify_rlc(n, lproofs, lin["pl"], _cat(lr, "C"), *bases, _cat(lr, "b"), transcript=st, weights64=w, want_transcripts=True)
        assert a == b and a[1] is (nb != NB)
    rows = [dict(r, proof=iproofs[ipp["pl"] * p:ipp["pl"] * (p + 1)]) for p, r in enumerate(ir)]
    cat = lambda key: _cat(rows, key)
    a = ctx.ipp_verify_batch_ts(n, iproofs, ipp["pl"], st, cat("Gf"), cat("Hf"), cat("P"), cat("Q"), ipp["G"], ipp["H"], want_msm=True, want_transcripts=True)
    assert a[:2] == _ipp_existing(ctx, ipp, rows, st) and [p for p in range(nb) if a[0][p]] == sorted(kinds)
    for G, H in ((ipp["G"], ipp["H"]), (None, None)):
        c = ctx.ipp_verify_rlc_ts(n, iproofs, ipp["pl"], st, cat("Gf"), cat("Hf"), cat("P"), cat("Q"), G, H, weights64=w, want_transcripts=True)
        b = ctx.ipp_verify_rlc(n, iproofs, ipp["pl"], cat("Gf"), cat("Hf"), cat("P"), cat("Q"), G, H, transcript=st, weights64=w)
        assert c[:3] == b and c[3] == a[2] and c[1] is (nb != NB)
    # what the inner-product prover leaves is what the verifier leaves
    if nb == 3:
        assert got[2] == a[2]


# ============================================================================================================================================
# creation
# ============================================================================================================================================
class _ChaChaScalars:
    """the rng handed to the twin's create(): Scalar::random of ChaChaRng::from_seed(seed)"""

    def __init__(self, seed):
        from chacha_rng import ChaChaRng
        self.rng = ChaChaRng(seed)

    def scalar(self):
        from chacha_rng import scalar_random
        return int.from_bytes(scalar_random(self.rng), "little")


@BOTH
@SHAPES
def test_linear_create_on_one_transcript_per_proof(ctx, oracle, n, nb, fixed):
    import bp_twin as T
    d = _lin_rows(ctx, oracle, n)
    rows = d["rows"][:nb]
    bases = (None, None, None) if fixed else (d["G"], d["F"], d["B"])
    states = _cat(rows, "st")
    proofs, status, ts = ctx.linear_create_batch_ts(n, states, _cat(rows, "C"), _cat(rows, "r"), _cat(rows, "a"), _cat(rows, "b"), *bases,
                                                    rng32=_cat(rows, "seed"), want_transcripts=True)
    assert ctx.get_option("staging_residue") == 0
    # C1: the existing call, one proof at a time, on the expanded keystream
    assert status == bytes(nb) and proofs == _cat(rows, "proof") and ts == _cat(rows, "ts_created")
    # the reference's create() with ChaChaRng::from_seed(seed) (oracle twin), a few rows
    dec = lambda b: [T.decompress(b[32 * i:32 * i + 32]) for i in range(len(b) // 32)]
    for p in sorted({0, 1, 2, nb - 1} & set(range(nb))) if n < 64 else [nb - 1]:
        row = rows[p]
        t = row["t0"].clone()
        want = T.linear_create(t, _ChaChaScalars(row["seed"]), row["C"], row["r_int"], row["a_int"], row["b_int"], dec(d["G"]), T.decompress(d["F"]), T.decompress(d["B"]))
        assert proofs[d["pl"] * p:d["pl"] * (p + 1)] == want and ts[TS * p:TS * (p + 1)] == _state_of(t), p
    # prover and verifier leave equal transcripts
    verdict, vts = ctx.linear_verify_batch_ts(n, proofs, d["pl"], states, _cat(rows, "C"), *bases, _cat(rows, "b"), want_transcripts=True)
    assert verdict == bytes(nb) and vts == ts
    # the library's own seeds: other proofs each time, and they verify
    if nb == 3:
        x = ctx.linear_create_batch_ts(n, states, _cat(rows, "C"), _cat(rows, "r"), _cat(rows, "a"), _cat(rows, "b"), *bases, want_transcripts=True)
        y = ctx.linear_create_batch_ts(n, states, _cat(rows, "C"), _cat(rows, "r"), _cat(rows, "a"), _cat(rows, "b"), *bases)
        assert ctx.get_option("staging_residue") == 0
        pl = d["pl"]
        assert all(len({x[0][pl * p:pl * (p + 1)], y[0][pl * p:pl * (p + 1)], proofs[pl * p:pl * (p + 1)]}) == 3 for p in range(nb))
        for out in (x, y):
            assert ctx.linear_verify_batch_ts(n, out[0], pl, states, _cat(rows, "C"), *bases, _cat(rows, "b")) == bytes(nb)
        assert ctx.linear_verify_batch_ts(n, x[0], pl, states, _cat(rows, "C"), *bases, _cat(rows, "b"), want_transcripts=True)[1] == x[2]


@SHAPES
def test_inner_product_create_on_one_transcript_per_proof(ctx, oracle, n, nb):
    d = _ipp_rows(ctx, oracle, n)
    rows = d["rows"][:nb]
    cat = lambda key: _cat(rows, key)
    proofs, status, ts = ctx.ipp_create_batch_ts(n, cat("st"), cat("Q"), cat("Gf"), cat("Hf"), d["G"], d["H"], cat("a"), cat("b"), want_transcripts=True)
    assert status == bytes(nb) and proofs == cat("proof")                                          # C1
    verdict, vts = ctx.ipp_verify_batch_ts(n, proofs, d["pl"], cat("st"), cat("Gf"), cat("Hf"), cat("P"), cat("Q"), d["G"], d["H"], want_transcripts=True)
    assert verdict == bytes(nb) and vts == ts
    if nb == 3:                                                                                    # bases per proof
        again = ctx.ipp_create_batch_ts(n, cat("st"), cat("Q"), cat("Gf"), cat("Hf"), d["G"] * nb, d["H"] * nb, cat("a"), cat("b"), want_transcripts=True)
        assert again == (proofs, status, ts)


# ============================================================================================================================================
# the device-pointer forms
# ============================================================================================================================================
def _undecided(verdict, ok, kinds):
    """what a _dev combined check reports where the host form has fallen back: front-end codes kept, the rest undecided"""
    if ok:
        return verdict
    return bytes(v if (v == FORMAT or kinds.get(p) == "identity") else UNDECIDED for p, v in enumerate(verdict))


@pytest.mark.parametrize("n,nb", [(8, 3), (64, NB)])
def test_device_pointer_forms_on_a_side_stream_give_the_host_forms_bytes(ctx, oracle, n, nb):
    import bulletproofs_amd as bp
    import torch
    L = bp.lib()
    kinds = DAMAGED if nb == NB else {}
    w = _weights(b"dev-%d" % n, nb)
    side = torch.cuda.Stream(device=_dev())
    d_w = _to_dev(w)
    # ---- linear, explicit bases and generator tables
    d = _lin_rows(ctx, oracle, n)
    rows = _batch(d, nb)
    states = _cat(rows, "st")
    d_pr, d_c, d_b, d_t = _to_dev(_cat(rows, "proof")), _to_dev(_cat(rows, "C")), _to_dev(_cat(rows, "b")), _to_dev(states)
    d_g, d_f, d_bb = _to_dev(d["G"]), _to_dev(d["F"]), _to_dev(d["B"])
    for fixed in (False, True):
        bases = (None, None, None) if fixed else (d["G"], d["F"], d["B"])
        dbase = (None, None, None) if fixed else (d_g, d_f, d_bb)
        want = ctx.linear_verify_batch_ts(n, _cat(rows, "proof"), d["pl"], states, _cat(rows, "C"), *bases, _cat(rows, "b"), want_msm=True, want_transcripts=True)
        wrlc = ctx.linear_verify_rlc_ts(n, _cat(rows, "proof"), d["pl"], states, _cat(rows, "C"), *bases, _cat(rows, "b"), weights64=w, want_transcripts=True)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            d_v, d_o, d_to = _filled(nb), _filled(32 * nb), _filled(TS * nb)
            assert L.bpgpu_linear_verify_batch_ts_dev(ctx.h, n, nb, d_pr.data_ptr(), d["pl"], None, d_t.data_ptr(), d_c.data_ptr(), *[_ptr(x) for x in dbase],
                                                      d_b.data_ptr(), 0, d_v.data_ptr(), d_o.data_ptr(), d_to.data_ptr(), side.cuda_stream) == 0
            d_v2, d_bo, d_to2 = _filled(nb), _filled(64), _filled(TS * nb)
            assert L.bpgpu_linear_verify_rlc_ts_dev(ctx.h, n, nb, d_pr.data_ptr(), d["pl"], None, d_t.data_ptr(), d_c.data_ptr(), *[_ptr(x) for x in dbase],
                                                    d_b.data_ptr(), 0, d_w.data_ptr(), d_v2.data_ptr(), d_bo.data_ptr(), d_to2.data_ptr(), side.cuda_stream) == 0
        side.synchronize()
        assert (_raw(d_v, nb), _raw(d_o, 32 * nb), _raw(d_to, TS * nb)) == want
        bo = _raw(d_bo, 33)
        assert (bo[0] == 0, bo[1:33], _raw(d_to2, TS * nb)) == wrlc[1:] and _raw(d_v2, nb) == _undecided(wrlc[0], wrlc[1], kinds)
    # ---- inner product, bases given once; the combined check with explicit bases and generator tables
    d = _ipp_rows(ctx, oracle, n)
    rows = _batch(d, nb)
    cat = lambda key: _cat(rows, key)
    bufs = [_to_dev(cat(key)) for key in ("proof", "Gf", "Hf", "P", "Q")]
    d_g, d_h = _to_dev(d["G"]), _to_dev(d["H"])
    want = ctx.ipp_verify_batch_ts(n, cat("proof"), d["pl"], states, cat("Gf"), cat("Hf"), cat("P"), cat("Q"), d["G"], d["H"], want_msm=True, want_transcripts=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d_v, d_o, d_to = _filled(nb), _filled(32 * nb), _filled(TS * nb)
        assert L.bpgpu_ipp_verify_batch_ts_dev(ctx.h, n, nb, bufs[0].data_ptr(), d["pl"], None, d_t.data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                                               bufs[3].data_ptr(), bufs[4].data_ptr(), d_g.data_ptr(), d_h.data_ptr(), 1, d_v.data_ptr(), d_o.data_ptr(),
                                               d_to.data_ptr(), side.cuda_stream) == 0
    side.synchronize()
    assert (_raw(d_v, nb), _raw(d_o, 32 * nb), _raw(d_to, TS * nb)) == want
    for fixed in (False, True):
        wrlc = ctx.ipp_verify_rlc_ts(n, cat("proof"), d["pl"], states, cat("Gf"), cat("Hf"), cat("P"), cat("Q"), None if fixed else d["G"], None if fixed else d["H"],
                                     weights64=w, want_transcripts=True)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            d_v2, d_bo, d_to2 = _filled(nb), _filled(64), _filled(TS * nb)
            assert L.bpgpu_ipp_verify_rlc_ts_dev(ctx.h, n, nb, bufs[0].data_ptr(), d["pl"], None, d_t.data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                                                 bufs[3].data_ptr(), bufs[4].data_ptr(), None if fixed else d_g.data_ptr(), None if fixed else d_h.data_ptr(), 1,
                                                 d_w.data_ptr(), d_v2.data_ptr(), d_bo.data_ptr(), d_to2.data_ptr(), side.cuda_stream) == 0
        side.synchronize()
        bo = _raw(d_bo, 33)
        assert (bo[0] == 0, bo[1:33], _raw(d_to2, TS * nb)) == wrlc[1:] and _raw(d_v2, nb) == _undecided(wrlc[0], wrlc[1], kinds)


def test_device_pointer_forms_with_one_host_state_and_with_position_bytes_out_of_range(ctx, shared8):
    """shared_transcript (a host pointer, handed to the kernels by value) == the host forms with transcript_stride = 0; a device state whose
    position byte is 200 -- past the sponge's rate, and unseen by the host -- is started at position 0"""
    import bulletproofs_amd as bp
    import torch
    L = bp.lib()
    s = shared8
    n, st, lin, ipp, nb = s["n"], s["st"], s["lin"], s["ipp"], 3
    lr, ir = lin["rows"][:nb], ipp["rows"][:nb]
    lproofs, iproofs = s["lin_created"][0][:lin["pl"] * nb], s["ipp_created"][0][:ipp["pl"] * nb]
    cat = lambda key: _cat(ir, key)
    d_pr, d_c, d_b = _to_dev(lproofs), _to_dev(_cat(lr, "C")), _to_dev(_cat(lr, "b"))
    bufs = [_to_dev(iproofs)] + [_to_dev(cat(key)) for key in ("Gf", "Hf", "P", "Q")]
    d_g, d_h = _to_dev(ipp["G"]), _to_dev(ipp["H"])
    want_l = ctx.linear_verify_batch_ts(n, lproofs, lin["pl"], st, _cat(lr, "C"), None, None, None, _cat(lr, "b"), want_msm=True, want_transcripts=True)
    want_i = ctx.ipp_verify_batch_ts(n, iproofs, ipp["pl"], st, cat("Gf"), cat("Hf"), cat("P"), cat("Q"), ipp["G"], ipp["H"], want_msm=True, want_transcripts=True)
    assert want_l[0] == want_i[0] == bytes(nb)
    d_v, d_o, d_to = _filled(nb), _filled(32 * nb), _filled(TS * nb)
    d_v2, d_o2, d_to2 = _filled(nb), _filled(32 * nb), _filled(TS * nb)
    d_v3, d_bo3, d_to3 = _filled(nb), _filled(64), _filled(TS * nb)
    d_v4, d_bo4, d_to4 = _filled(nb), _filled(64), _filled(TS * nb)
    torch.cuda.synchronize()
    assert L.bpgpu_linear_verify_batch_ts_dev(ctx.h, n, nb, d_pr.data_ptr(), lin["pl"], st, None, d_c.data_ptr(), None, None, None, d_b.data_ptr(), 0,
                                              d_v.data_ptr(), d_o.data_ptr(), d_to.data_ptr(), None) == 0
    assert L.bpgpu_ipp_verify_batch_ts_dev(ctx.h, n, nb, bufs[0].data_ptr(), ipp["pl"], st, None, bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(),
                                           bufs[4].data_ptr(), d_g.data_ptr(), d_h.data_ptr(), 1, d_v2.data_ptr(), d_o2.data_ptr(), d_to2.data_ptr(), None) == 0
    assert L.bpgpu_linear_verify_rlc_ts_dev(ctx.h, n, nb, d_pr.data_ptr(), lin["pl"], st, None, d_c.data_ptr(), None, None, None, d_b.data_ptr(), 0, None,
                                            d_v3.data_ptr(), d_bo3.data_ptr(), d_to3.data_ptr(), None) == 0
    assert L.bpgpu_ipp_verify_rlc_ts_dev(ctx.h, n, nb, bufs[0].data_ptr(), ipp["pl"], st, None, bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(),
                                         bufs[4].data_ptr(), None, None, 1, None, d_v4.data_ptr(), d_bo4.data_ptr(), d_to4.data_ptr(), None) == 0
    ctx.synchronize()
    assert (_raw(d_v, nb), _raw(d_o, 32 * nb), _raw(d_to, TS * nb)) == want_l
    assert (_raw(d_v2, nb), _raw(d_o2, 32 * nb), _raw(d_to2, TS * nb)) == want_i
    assert (_raw(d_v3, nb), _raw(d_bo3, 33), _raw(d_to3, TS * nb)) == (bytes(nb), bytes(33), want_l[2])
    assert (_raw(d_v4, nb), _raw(d_bo4, 33), _raw(d_to4, TS * nb)) == (bytes(nb), bytes(33), want_i[2])
    # exactly one of the two sources, aligned
    assert L.bpgpu_linear_verify_batch_ts_dev(ctx.h, n, nb, d_pr.data_ptr(), lin["pl"], None, None, d_c.data_ptr(), None, None, None, d_b.data_ptr(), 0,
                                              d_v.data_ptr(), None, None, None) == INVALID_ARG
    assert L.bpgpu_ipp_verify_rlc_ts_dev(ctx.h, n, nb, bufs[0].data_ptr(), ipp["pl"], st, d_to.data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(),
                                         bufs[4].data_ptr(), None, None, 1, None, d_v4.data_ptr(), None, None, None) == INVALID_ARG
    assert L.bpgpu_ipp_verify_batch_ts_dev(ctx.h, n, nb, bufs[0].data_ptr(), ipp["pl"], None, d_to.data_ptr() + 2, bufs[1].data_ptr(), bufs[2].data_ptr(),
                                           bufs[3].data_ptr(), bufs[4].data_ptr(), d_g.data_ptr(), d_h.data_ptr(), 1, d_v2.data_ptr(), None, None, None) == INVALID_ARG
    # position byte 200: the lanes start such a state at position 0 -- the outputs of the same sponge words at pos = pos_begin = 0
    odd = bytearray(st)
    odd[200], odd[201] = 200, 7
    zero = bytearray(st)
    zero[200], zero[201] = 0, 0
    want_l = ctx.linear_verify_batch_ts(n, lproofs, lin["pl"], bytes(zero), _cat(lr, "C"), None, None, None, _cat(lr, "b"), want_msm=True, want_transcripts=True)
    want_i = ctx.ipp_verify_batch_ts(n, iproofs, ipp["pl"], bytes(zero), cat("Gf"), cat("Hf"), cat("P"), cat("Q"), ipp["G"], ipp["H"], want_msm=True,
                                     want_transcripts=True)
    assert want_l[0] == want_i[0] == bytes([VERIFICATION]) * nb
    d_t = _to_dev(bytes(odd) * nb)
    d_v, d_o, d_to = _filled(nb), _filled(32 * nb), _filled(TS * nb)
    d_v2, d_o2, d_to2 = _filled(nb), _filled(32 * nb), _filled(TS * nb)
    d_v4, d_bo4, d_to4 = _filled(nb), _filled(64), _filled(TS * nb)
    torch.cuda.synchronize()
    assert L.bpgpu_linear_verify_batch_ts_dev(ctx.h, n, nb, d_pr.data_ptr(), lin["pl"], None, d_t.data_ptr(), d_c.data_ptr(), None, None, None, d_b.data_ptr(), 0,
                                              d_v.data_ptr(), d_o.data_ptr(), d_to.data_ptr(), None) == 0
    assert L.bpgpu_ipp_verify_batch_ts_dev(ctx.h, n, nb, bufs[0].data_ptr(), ipp["pl"], None, d_t.data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                                           bufs[3].data_ptr(), bufs[4].data_ptr(), d_g.data_ptr(), d_h.data_ptr(), 1, d_v2.data_ptr(), d_o2.data_ptr(),
                                           d_to2.data_ptr(), None) == 0
    assert L.bpgpu_ipp_verify_rlc_ts_dev(ctx.h, n, nb, bufs[0].data_ptr(), ipp["pl"], None, d_t.data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(),
                                         bufs[4].data_ptr(), d_g.data_ptr(), d_h.data_ptr(), 1, None, d_v4.data_ptr(), d_bo4.data_ptr(), d_to4.data_ptr(), None) == 0
    ctx.synchronize()
    assert (_raw(d_v, nb), _raw(d_o, 32 * nb), _raw(d_to, TS * nb)) == want_l
    assert (_raw(d_v2, nb), _raw(d_o2, 32 * nb), _raw(d_to2, TS * nb)) == want_i
    assert _raw(d_v4, nb) == bytes([UNDECIDED]) * nb and _raw(d_to4, TS * nb) == want_i[2]


# ============================================================================================================================================
# errors
# ============================================================================================================================================
def test_bad_transcript_arguments_are_refused_and_leave_the_outputs_untouched(ctx, oracle):
    import bulletproofs_amd as bp
    L = bp.lib()
    n, nb = 8, 3
    lin, ipp = _lin_rows(ctx, oracle, n), _ipp_rows(ctx, oracle, n)
    lr, ir = lin["rows"][:nb], ipp["rows"][:nb]
    states = _cat(lr, "st")
    assert states == _cat(ir, "st")
    cat = lambda key: _cat(ir, key)
    pat = lambda nbytes: C.create_string_buffer(b"\x5a" * nbytes, nbytes)
    outs = dict(v=pat(nb), o=pat(32 * nb), t=pat(TS * nb), bo=pat(33), pr=pat(lin["pl"] * nb), st=pat(nb))

    def calls(ts, stride, nb_=nb):
        """the six host-pointer entry points' return codes for one (transcripts, stride)"""
        o = outs
        return [
            L.bpgpu_ipp_verify_batch_ts(ctx.h, n, nb_, cat("proof"), ipp["pl"], ts, stride, cat("Gf"), cat("Hf"), cat("P"), cat("Q"), ipp["G"], ipp["H"], 1, o["v"], o["o"], o["t"]),
            L.bpgpu_ipp_verify_rlc_ts(ctx.h, n, nb_, cat("proof"), ipp["pl"], ts, stride, cat("Gf"), cat("Hf"), cat("P"), cat("Q"), ipp["G"], ipp["H"], 1, None, o["v"], o["bo"],
                                      o["t"]),
            L.bpgpu_linear_verify_batch_ts(ctx.h, n, nb_, _cat(lr, "proof"), lin["pl"], ts, stride, _cat(lr, "C"), lin["G"], lin["F"], lin["B"], _cat(lr, "b"), 0, o["v"],
                                           o["o"], o["t"]),
            L.bpgpu_linear_verify_rlc_ts(ctx.h, n, nb_, _cat(lr, "proof"), lin["pl"], ts, stride, _cat(lr, "C"), None, None, None, _cat(lr, "b"), 0, None, o["v"], o["bo"],
                                         o["t"]),
            L.bpgpu_ipp_create_batch_ts(ctx.h, n, nb_, ts, stride, cat("Q"), cat("Gf"), cat("Hf"), ipp["G"], ipp["H"], 1, cat("a"), cat("b"), o["pr"], o["st"], o["t"]),
            L.bpgpu_linear_create_batch_ts(ctx.h, n, nb_, ts, stride, _cat(lr, "seed"), _cat(lr, "C"), _cat(lr, "r"), _cat(lr, "a"), _cat(lr, "b"), 0, lin["G"], lin["F"],
                                           lin["B"], o["pr"], o["st"], o["t"]),
        ]

    untouched = lambda: all(buf.raw == b"\x5a" * len(buf.raw) for buf in outs.values())
    malformed = bytearray(states)
    malformed[TS * (nb - 1) + 200] = 166                                                           # the LAST state: every one is checked
    begin = bytearray(states)
    begin[TS + 201] = 167
    refused = ((states, 17), (states, TS - 1), (states, 2 * TS), (None, TS), (None, 0), (bytes(malformed), TS), (bytes(begin), TS),
               (bytes(malformed[TS * (nb - 1):]), 0))
    # the seeds are secrets: after a successful and after a failed bpgpu_linear_create_batch_ts nothing is left in the secret part of the
    # staging block nor in the working sets (the probe of test_gpu_prover_seeded.py; it is read before a verifier stages public inputs again)
    scratch = dict(pr=pat(lin["pl"] * nb), st=pat(nb), t=pat(TS * nb))

    def lin_create(ts, stride):
        rc = L.bpgpu_linear_create_batch_ts(ctx.h, n, nb, ts, stride, _cat(lr, "seed"), _cat(lr, "C"), _cat(lr, "r"), _cat(lr, "a"), _cat(lr, "b"), 0, lin["G"], lin["F"],
                                            lin["B"], scratch["pr"], scratch["st"], scratch["t"])
        assert ctx.get_option("staging_residue") == 0
        return rc
    assert lin_create(states, TS) == 0 and scratch["pr"].raw == _cat(lr, "proof")
    for ts, stride in refused:
        assert lin_create(ts, stride) == INVALID_ARG, (stride, ts is None)
    for ts, stride in refused:
        assert calls(ts, stride) == [INVALID_ARG] * 6, (stride, ts is None)
        assert untouched()
    assert calls(None, 17, nb_=0) == [INVALID_ARG] * 6 and untouched()
    assert calls(states, TS, nb_=0) == [0] * 6                                                      # an empty batch: BPGPU_OK ...
    assert outs["bo"].raw == bytes(33)                                                             # ... and the empty sum
    outs["bo"].raw = b"\x5a" * 33
    assert untouched()
    assert L.bpgpu_linear_verify_batch_ts(None, n, nb, _cat(lr, "proof"), lin["pl"], states, TS, _cat(lr, "C"), None, None, None, _cat(lr, "b"), 0, outs["v"], None,
                                          None) == INVALID_ARG
    # a failure behind the transcript checks: generators too small for the table mode
    big = L.bpgpu_linear_create_batch_ts(ctx.h, 128, 1, states, 0, _cat(lr, "seed"), lr[0]["C"], lr[0]["r"], bytes(32 * 128), bytes(32 * 128), 0, None, None, None,
                                         C.create_string_buffer(32 * 17), outs["st"], None)
    assert big not in (0, INVALID_ARG)
    assert calls(states, TS) == [0] * 6 and not untouched()
    assert ctx.get_option("staging_residue") == 0                                                  # (the last of the six is the linear prover)


# ============================================================================================================================================
# the Python and C++ mirrors
# ============================================================================================================================================
def test_python_api_on_a_list_of_transcripts(ctx, oracle):
    from bulletproofs_amd import api
    n, nb = 8, 4
    d = _lin_rows(ctx, oracle, n)
    rows = d["rows"][:nb]
    split = lambda b: [b[32 * i:32 * i + 32] for i in range(len(b) // 32)]
    G, F, B = split(d["G"]), d["F"], d["B"]

    def sessions():
        out = []
        for row in rows:
            t = api.Transcript(b"unused")
            t.state, t.fresh_label = row["st"], None
            out.append(t)
        return out
    provers, v1, v2 = sessions(), sessions(), sessions()
    proofs = api.LinearProof.create_batch(ctx, provers, [r["C"] for r in rows], [r["r"] for r in rows], [split(r["a"]) for r in rows], [split(r["b"]) for r in rows],
                                          G, F, B, rng_seed32=_cat(rows, "seed"))
    assert [p.to_bytes() for p in proofs] == [r["proof"] for r in rows]
    Cs, bvs = [r["C"] for r in rows], [split(r["b"]) for r in rows]
    assert api.LinearProof.verify_batch(ctx, v1, proofs, Cs, G, F, B, bvs) == [None] * nb
    assert api.LinearProof.verify_batch_combined(ctx, v2, proofs, Cs, G, F, B, bvs) == [None] * nb
    # the lists come back advanced to the twin's states
    for lst in (provers, v1, v2):
        assert [t.state for t in lst] == [_lin_ts_want(d, r) for r in rows] and all(t.fresh_label is None for t in lst)
    # the single-proof call with the keyword takes the same path
    t = sessions()[1]
    one = api.LinearProof.create(t, None, rows[1]["C"], rows[1]["r"], split(rows[1]["a"]), split(rows[1]["b"]), G, F, B, ctx, rng_seed32=rows[1]["seed"])
    assert one.to_bytes() == rows[1]["proof"] and t.state == provers[1].state
    # a proof on another session's transcript fails on both paths; its transcript is left behind the separator
    w1, w2 = sessions(), sessions()
    for lst in (w1, w2):
        lst[0], lst[2] = lst[2], lst[0]
    r1 = api.LinearProof.verify_batch(ctx, w1, proofs, Cs, G, F, B, bvs)
    r2 = api.LinearProof.verify_batch_combined(ctx, w2, proofs, Cs, G, F, B, bvs)
    assert [type(x) for x in r1] == [type(x) for x in r2] == [api.VerificationError, type(None), api.VerificationError, type(None)]
    assert [t.state for t in w1] == [t.state for t in w2]
    # one bound transcript for all: not advanced (the existing behaviour)
    shared = sessions()[3]
    before = shared.state
    made = api.LinearProof.create_batch(ctx, shared, Cs, [r["r"] for r in rows], [split(r["a"]) for r in rows], bvs, G, F, B)
    assert shared.state == before and api.LinearProof.verify_batch(ctx, shared, made, Cs, G, F, B, bvs) == [None] * nb and shared.state == before


def test_cpp_mirror_takes_one_transcript_per_proof(tmp_path):
    """include/bulletproofs.hpp: LinearProof::create_batch and the std::vector<Transcript>& overloads of verify_batch / verify_batch_combined"""
    exe = str(tmp_path / "linear_proof_ts_test")
    csrc = os.path.join(ROOT, "bulletproofs_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "linear_proof_ts_test.cpp"),
                           "-L", csrc, "-lbpgpu", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout
