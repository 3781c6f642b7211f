"""Test-side statement of the opening proofs (include/bpgpu.h, bpgpu_opening_*): the sigma protocol for C = v B + r B_blinding on
oracle/py/bp_twin.py's Merlin transcript and oracle/py/chacha_rng.py's ChaChaRng.  Nothing in the reference defines this protocol; the
issue that introduced it does, and this file restates it from there.  Group arithmetic goes through the C oracle's oracle_msm on
compressed encodings (as tests/r1cs_twin.py does), so that batches of 130 proofs take well under a second.
TEST INFRASTRUCTURE ONLY: the product never imports this file."""
import hashlib

import bp_twin as T
import pyoracle as O
from chacha_rng import ChaChaRng, scalar_random
from r1cs_twin import transcript_from_state, transcript_state

L = T.L
FULL, BLINDING = 0, 1
OK, VERIFICATION_ERROR, FORMAT_ERROR, UNDECIDED = 0, 1, 2, 5
BAD_SCALAR = 2
PROOF_LEN = {FULL: 96, BLINDING: 64}
RATE = 166          # STROBE-128's rate as Merlin uses it


def le32(x):
    return int(x).to_bytes(32, "little")


def msm(scalars, points):
    """sum scalars[i] points[i] over compressed encodings; None when a point does not decode"""
    st, out = O.msm(b"".join(le32(s % L) for s in scalars), b"".join(points))
    return None if st else out


def bases():
    """(B, B_blinding) of PedersenGens::default(), compressed"""
    _, _, B, Bb = O.Gens(1, 1).export()
    return B, Bb


def commit(B, Bb, v, r):
    return msm([v, r], [B, Bb])


def bind(t, form, C, v):
    """the statement: separator, form, C and (form 1) the public value"""
    t.append_message(b"dom-sep", b"openingproof v1")
    t.append_u64(b"form", form)
    t.append_point(b"C", C)
    if form == BLINDING:
        t.append_scalar(b"v", v)


def nonces(form, seed32):
    rng = ChaChaRng(seed32)
    draw = lambda: int.from_bytes(scalar_random(rng), "little")
    k_v = draw() if form == FULL else 0
    return k_v, draw()


def create(state, form, B, Bb, C, v, r, seed32):
    """-> (proof bytes, status, state out).  v, r: ints below 2^256; one that is not canonical voids the row"""
    if v >= L or r >= L:
        return bytes(PROOF_LEN[form]), BAD_SCALAR, state
    t = transcript_from_state(state)
    k_v, k_r = nonces(form, seed32)
    R = msm([k_v, k_r], [B, Bb])
    bind(t, form, C, v)
    t.validate_and_append_point(b"R", R)       # (R = identity has probability 2^-252: not a case of the tests)
    c = t.challenge_scalar(b"c")
    proof = R + (le32((k_v + c * v) % L) if form == FULL else b"") + le32((k_r + c * r) % L)
    return proof, OK, transcript_state(t)


def front(state, form, proof, C, v=0):
    """The verifier up to the multiscalar multiplication -> (status, state out, c, s_v, s_r); c, s_v, s_r are None where the row stopped.
    v: the public value of form 1 as an int below 2^256."""
    assert len(proof) == PROOF_LEN[form]
    R = proof[:32]
    s_r = int.from_bytes(proof[-32:], "little")
    s_v = int.from_bytes(proof[32:64], "little") if form == FULL else None
    if s_r >= L or (form == FULL and s_v >= L) or (form == BLINDING and v >= L):
        return FORMAT_ERROR, state, None, None, None
    t = transcript_from_state(state)
    bind(t, form, C, v)
    try:
        t.validate_and_append_point(b"R", R)
    except T.VerificationError:
        return VERIFICATION_ERROR, transcript_state(t), None, None, None
    c = t.challenge_scalar(b"c")
    if form == BLINDING:
        s_v = c * v % L
    return OK, transcript_state(t), c, s_v, s_r


def check_terms(B, Bb, proof, C, c, s_v, s_r):
    """the four terms of contract (a): (s_v, B), (s_r, B_blinding), (l - c, C), (l - 1, R)"""
    return [s_v, s_r, (L - c) % L, L - 1], [B, Bb, C, proof[:32]]


def verify(state, form, B, Bb, proof, C, v=0):
    """-> (verdict, state out, msm_out): msm_out is the compressed check, 32 zero bytes where the row stopped before it or a point
    did not decode"""
    st, out, c, s_v, s_r = front(state, form, proof, C, v)
    if st:
        return st, out, bytes(32)
    res = msm(*check_terms(B, Bb, proof, C, c, s_v, s_r))
    if res is None:
        return VERIFICATION_ERROR, out, bytes(32)
    return (OK if res == bytes(32) else VERIFICATION_ERROR), out, res


# ---- start states at chosen STROBE positions ----------------------------------------------------------------------------
def state_at(pos, tag=b""):
    """A bound transcript (label, a session message) whose STROBE position is `pos`: the padding message's length is found by search"""
    for k in range(2 * RATE):
        t = T.Transcript(b"opening proof test")
        t.append_message(b"session", tag + bytes(k))
        if t.strobe.pos == pos:
            return transcript_state(t)
    raise AssertionError("no padding length reaches position %d" % pos)


def positions(state, form, C, v, R):
    """STROBE positions before the separator, before C's message, before R's message and after it (for the tests' boundary claims)"""
    t = transcript_from_state(state)
    out = [t.strobe.pos]
    t.append_message(b"dom-sep", b"openingproof v1")
    t.append_u64(b"form", form)
    out.append(t.strobe.pos)
    t.append_point(b"C", C)
    if form == BLINDING:
        t.append_scalar(b"v", v)
    out.append(t.strobe.pos)
    t.append_point(b"R", R)
    out.append(t.strobe.pos)
    return out


def det_scalar(tag, i):
    return int.from_bytes(hashlib.sha512(b"opening-twin" + tag + i.to_bytes(4, "little")).digest(), "little") % L


def det_seed(tag, i):
    return hashlib.sha256(b"opening-seed" + tag + i.to_bytes(4, "little")).digest()
