"""Test-side statement of the sigma proofs of recorded linear relations (include/bpgpu.h, bpgpu_sigma_*) on oracle/py/bp_twin.py's Merlin
transcript and oracle/py/chacha_rng.py's ChaChaRng, built as tests/opening_twin.py is.  Nothing in the reference defines this protocol;
the issue that introduced it does, and this file restates it from there.  Group arithmetic goes through the C oracle's oracle_msm on
compressed encodings.  A relation here is (S, P, [(lhs, [(secret, base), ...]), ...]) with the base ids of the header: 0 B_blinding, 1 B,
2 + i G_i, 16 + p instance slot p; lhs is 16 + p.
TEST INFRASTRUCTURE ONLY: the product never imports this file."""
import bp_twin as T
import pyoracle as O
from chacha_rng import ChaChaRng, scalar_random
from opening_twin import RATE, det_scalar, det_seed, le32, msm          # noqa: F401  (re-exported for the tests)
from r1cs_twin import transcript_from_state, transcript_state

L = T.L
OK, VERIFICATION_ERROR, FORMAT_ERROR, UNDECIDED = 0, 1, 2, 5
BAD_POINT, BAD_SCALAR = 1, 2
SLOT = 16


def descriptor(rel):
    S, P, eqs = rel
    out = bytearray([S, P, len(eqs)])
    for lhs, terms in eqs:
        out += bytes([lhs, len(terms)])
        for s, b in terms:
            out += bytes([s, b])
    return bytes(out)


def digest(desc):
    t = T.Transcript(b"sigma statement")
    t.append_message(b"desc", desc)
    return t.challenge_bytes(b"digest", 32)


def shared_bases(ngens=8):
    """{base id: encoding} for B_blinding, B and G_0 .. G_{ngens-1} of party 0"""
    G, _, B, Bb = O.Gens(ngens, 1).export()
    out = {0: Bb, 1: B}
    for i in range(ngens):
        out[2 + i] = G[32 * i:32 * i + 32]
    return out


def base_of(bases, points, b):
    return points[b - SLOT] if b >= SLOT else bases[b]


def instance(rel, bases, secrets, free):
    """The P instance points of a TRUE statement: `free` maps the slots that are nobody's lhs to encodings; the lhs slots follow from
    the equations in order (an equation may use the lhs of an earlier one as a base)."""
    S, P, eqs = rel
    pts = [free.get(i) for i in range(P)]
    for lhs, terms in eqs:
        pts[lhs - SLOT] = msm([secrets[s] for s, _ in terms], [base_of(bases, pts, b) for _, b in terms])
    assert all(p is not None for p in pts)
    return pts


def bind(t, rel, points):
    t.append_message(b"dom-sep", b"sigmaproof v1")
    t.append_message(b"stmt", digest(descriptor(rel)))
    for p in points:
        t.append_point(b"P", p)


def nonces(S, seed32):
    rng = ChaChaRng(seed32)
    return [int.from_bytes(scalar_random(rng), "little") for _ in range(S)]


def create(state, rel, bases, points, secrets, seed32):
    """-> (proof bytes, status, state out).  A secret that is not canonical or an instance BASE that does not decode voids the row."""
    S, P, eqs = rel
    plen = 32 * (len(eqs) + S)
    if any(x >= L for x in secrets):
        return bytes(plen), BAD_SCALAR, state
    k = nonces(S, seed32)
    Ts = [msm([k[s] for s, _ in terms], [base_of(bases, points, b) for _, b in terms]) for _, terms in eqs]
    if any(x is None for x in Ts):
        return bytes(plen), BAD_POINT, state
    t = transcript_from_state(state)
    bind(t, rel, points)
    for x in Ts:
        t.validate_and_append_point(b"T", x)
    c = t.challenge_scalar(b"c")
    return b"".join(Ts) + b"".join(le32((k[j] + c * secrets[j]) % L) for j in range(S)), OK, transcript_state(t)


def front(state, rel, proof, points):
    """The verifier up to the multiscalar multiplications -> (status, state out, c, [s_j]); c and s are None where the row stopped."""
    S, P, eqs = rel
    E = len(eqs)
    assert len(proof) == 32 * (E + S)
    s = [int.from_bytes(proof[32 * (E + j):32 * (E + j) + 32], "little") for j in range(S)]
    if any(x >= L for x in s):
        return FORMAT_ERROR, state, None, None
    t = transcript_from_state(state)
    bind(t, rel, points)
    for k in range(E):
        try:
            t.validate_and_append_point(b"T", proof[32 * k:32 * k + 32])
        except T.VerificationError:
            return VERIFICATION_ERROR, transcript_state(t), None, None
    c = t.challenge_scalar(b"c")
    return OK, transcript_state(t), c, s


def check_terms(rel, bases, proof, points, c, s, k):
    """the terms of equation k's check: (s[sec], Base) per term, (l - c, slot[lhs]), (l - 1, T_k)"""
    lhs, terms = rel[2][k]
    return ([s[j] for j, _ in terms] + [(L - c) % L, L - 1],
            [base_of(bases, points, b) for _, b in terms] + [points[lhs - SLOT], proof[32 * k:32 * k + 32]])


def staged(rel, c, s, k):
    """what the front end stages for equation k: ({slot: coefficient} over the slots it touches, {shared base id: coefficient})"""
    lhs, terms = rel[2][k]
    slots, gens = {}, {}
    for j, b in terms:
        d = slots if b >= SLOT else gens
        key = b - SLOT if b >= SLOT else b
        d[key] = (d.get(key, 0) + s[j]) % L
    slots[lhs - SLOT] = (slots.get(lhs - SLOT, 0) - c) % L
    return slots, gens


def verify(state, rel, bases, proof, points):
    """-> (verdict, state out, [msm_out per equation]): an msm_out is 32 zero bytes where the row stopped before it or a point of that
    equation did not decode"""
    E = len(rel[2])
    st, out, c, s = front(state, rel, proof, points)
    if st:
        return st, out, [bytes(32)] * E
    res = [msm(*check_terms(rel, bases, proof, points, c, s, k)) for k in range(E)]
    ok = all(r == bytes(32) for r in res)
    return (OK if ok else VERIFICATION_ERROR), out, [r if r is not None else bytes(32) for r in res]


def state_at(pos, tag=b""):
    """A bound transcript whose STROBE position is `pos`: the padding message's length is found by search"""
    for k in range(2 * RATE):
        t = T.Transcript(b"sigma proof test")
        t.append_message(b"session", tag + bytes(k))
        if t.strobe.pos == pos:
            return transcript_state(t)
    raise AssertionError("no padding length reaches position %d" % pos)


def positions(state, rel, points, Ts):
    """STROBE positions before each message of the script, in order: separator, digest, the P points, the E commitments, and after the
    last one -- as [(name, before, after)]"""
    t = transcript_from_state(state)
    out = []

    def step(name, label, msg):
        before = t.strobe.pos
        t.append_message(label, msg)
        out.append((name, before, t.strobe.pos))
    step("sep", b"dom-sep", b"sigmaproof v1")
    step("digest", b"stmt", digest(descriptor(rel)))
    for p in points:
        step("P", b"P", p)
    for x in Ts:
        step("T", b"T", x)
    return out
