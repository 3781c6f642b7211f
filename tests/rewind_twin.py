"""Test-side statement of rewindable range proofs (include/bpgpu.h, bpgpu_rangeproof_prove_batch_rw / _rewind_batch): a draw wrapper round
oracle/py/bp_twin.py's prove_multiple -- an rng whose first scalar() is d_0 - e and whose later ones are oracle/py/chacha_rng.py's
ChaCha draws -- and the rewind in integers.  Nothing in the reference defines this protocol; the issue that introduced it does, and this
file restates it from there.  TEST INFRASTRUCTURE ONLY: the product never imports this file."""
import hashlib

import bp_twin as T
from chacha_rng import ChaChaRng, scalar_random
from r1cs_twin import transcript_from_state, transcript_state

L = T.L
OK, NOT_FOUND, FORMAT = 0, 1, 2
RATE = 166
SEED_LABEL = b"bpgpu rewind seed v1"


def draws(seed32, count):
    """d_0 .. d_{count-1}: the Scalar::random draws of ChaChaRng::from_seed(seed32)"""
    rng = ChaChaRng(seed32)
    return [int.from_bytes(scalar_random(rng), "little") for _ in range(count)]


def payload(v, msg16=None):
    """e = v + 2^64 msg, msg the 16-byte message as a little-endian integer"""
    return v + (int.from_bytes(msg16 or bytes(16), "little") << 64)


class RewindRng:
    """bp_twin's rng interface: scalar() number 0 is d_0 - e, every later one the seed's own draw"""

    def __init__(self, seed32, e):
        self.rng, self.e, self.k = ChaChaRng(seed32), e, 0

    def scalar(self):
        d = int.from_bytes(scalar_random(self.rng), "little")
        if self.k == 0:
            d = (d - self.e) % L
        self.k += 1
        return d


def contract_rng(n, seed32, e):
    """the `rng` buffer of the contract call: keystream blocks 0 .. 2n+3 of the seed, block 0 replaced by the 32 canonical bytes of
    (d_0 - e) mod l, zero-extended to 64"""
    rng = ChaChaRng(seed32)
    blocks = [rng.fill_bytes(64) for _ in range(2 * n + 4)]
    d0 = int.from_bytes(blocks[0], "little") % L
    blocks[0] = ((d0 - e) % L).to_bytes(32, "little") + bytes(32)
    return b"".join(blocks)


def prove(bp_gens, pc_gens, state, v, blinding, n, seed32, msg16=None):
    """-> (proof bytes, V, state out): bp_twin.prove_multiple (m = 1) under RewindRng"""
    t = transcript_from_state(state)
    pr, Vs = T.prove_multiple(bp_gens, pc_gens, t, [v], [blinding], n, RewindRng(seed32, payload(v, msg16)))
    return pr.to_bytes(), Vs[0], transcript_state(t)


def rewind(pc_gens, state, proof, V, n, seed32, commit=None):
    """-> (status, value, 16-byte message, blinding as an int); the three are zero unless the status is OK.  commit(v, gamma) -> 32
    bytes replaces the pure-Python Pedersen commitment where a faster one is at hand."""
    none = (0, bytes(16), 0)
    assert len(proof) == 32 * (9 + 2 * (n.bit_length() - 1))
    try:
        pr = T.RangeProof.from_bytes(proof)
    except T.FormatError:
        return (FORMAT,) + none
    t = transcript_from_state(state)
    t.rangeproof_domain_sep(n, 1)
    t.append_point(b"V", V)
    try:
        t.validate_and_append_point(b"A", pr.A)
        t.validate_and_append_point(b"S", pr.S)
        t.challenge_scalar(b"y")
        z = t.challenge_scalar(b"z")
        t.validate_and_append_point(b"T_1", pr.T_1)
        t.validate_and_append_point(b"T_2", pr.T_2)
    except T.VerificationError:
        return (NOT_FOUND,) + none
    x = t.challenge_scalar(b"x")
    d = draws(seed32, 2 * n + 4)
    e = (d[0] + d[1] * x - pr.e_blinding) % L
    if e >> 192:
        return (NOT_FOUND,) + none
    gamma = (pr.t_x_blinding - x * (d[2 * n + 2] + x * d[2 * n + 3])) * T.sc_inv(z * z % L) % L
    v, msg = e & (2**64 - 1), e >> 64
    got = commit(v, gamma) if commit else T.compress(pc_gens.commit(v, gamma))
    if got != V:
        return (NOT_FOUND,) + none
    return OK, v, msg.to_bytes(16, "little"), gamma


def seed_for(key32, commitment):
    """the seed derivation fixed in include/bpgpu.h"""
    t = T.Transcript(SEED_LABEL)
    t.append_message(b"key", key32)
    t.append_message(b"C", commitment)
    return t.challenge_bytes(b"seed", 32)


# ---- start states at chosen STROBE positions ----------------------------------------------------------------------------
def state_at(pos, tag=b""):
    """A bound transcript (label, a session message) whose STROBE position is `pos`: the padding message's length is found by search"""
    for k in range(2 * RATE):
        t = T.Transcript(b"rewind test")
        t.append_message(b"session", tag + bytes(k))
        if t.strobe.pos == pos:
            return transcript_state(t)
    raise AssertionError("no padding length reaches position %d" % pos)


def positions(state, n, V, proof):
    """STROBE positions before V, A, S, T_1 and after T_2 (for the tests' boundary claims); proof: its bytes"""
    t = transcript_from_state(state)
    t.rangeproof_domain_sep(n, 1)
    out = [t.strobe.pos]
    t.append_point(b"V", V)
    out.append(t.strobe.pos)
    t.append_point(b"A", proof[0:32])
    out.append(t.strobe.pos)
    t.append_point(b"S", proof[32:64])
    t.challenge_scalar(b"y")
    t.challenge_scalar(b"z")
    out.append(t.strobe.pos)
    t.append_point(b"T_1", proof[64:96])
    out.append(t.strobe.pos)
    t.append_point(b"T_2", proof[96:128])
    out.append(t.strobe.pos)
    return out


def det_scalar(tag, i):
    return int.from_bytes(hashlib.sha512(b"rewind-twin" + tag + i.to_bytes(4, "little")).digest(), "little") % L


def det_seed(tag, i):
    return hashlib.sha256(b"rewind-seed" + tag + i.to_bytes(4, "little")).digest()
