"""Test-side statement of scanning under many keys (include/bpgpu.h, bpgpu_rangeproof_scan_batch), in integers: the replay to x once, the
candidate e_j of every key, the LOWEST j with e_j < 2^192, then tests/rewind_twin.py's rewind under that key's seed.  It also traces the
seed derivation: the STROBE position after the key (the prefix the library stores per key) and every position at which Keccak-f runs
between the key and the seed -- the claim that a candidate costs one permutation.  TEST INFRASTRUCTURE ONLY: the product never imports
this file."""
import bp_twin as T
from r1cs_twin import transcript_from_state

import rewind_twin as R
from rewind_twin import FORMAT, NOT_FOUND, OK, L, seed_for  # noqa: F401

NONE = 0xFFFFFFFF
RATE = R.RATE
PREFIX_POS, PRF_POS = 91, 144   # what the header states; seed_traced measures them


def seed_traced(key32, commitment):
    """-> (seed, position after the key, [positions at which Keccak-f ran after the key]); the seed equals seed_for's"""
    t = T.Transcript(R.SEED_LABEL)
    t.append_message(b"key", key32)
    prefix_pos, ran = t.strobe.pos, []
    run_f = t.strobe._run_f

    def traced():
        ran.append(t.strobe.pos)
        run_f()

    t.strobe._run_f = traced
    t.append_message(b"C", commitment)
    seed = t.challenge_bytes(b"seed", 32)
    assert seed == seed_for(key32, commitment)
    return seed, prefix_pos, ran


def replay(state, proof, V, n):
    """steps 1 and 2 -> (status, proof object, x): the parse and the transcript up to x, as rewind_twin.rewind makes them"""
    assert len(proof) == 32 * (9 + 2 * (n.bit_length() - 1))
    try:
        pr = T.RangeProof.from_bytes(proof)
    except T.FormatError:
        return FORMAT, None, None
    t = transcript_from_state(state)
    t.rangeproof_domain_sep(n, 1)
    t.append_point(b"V", V)
    try:
        t.validate_and_append_point(b"A", pr.A)
        t.validate_and_append_point(b"S", pr.S)
        t.challenge_scalar(b"y")
        t.challenge_scalar(b"z")
        t.validate_and_append_point(b"T_1", pr.T_1)
        t.validate_and_append_point(b"T_2", pr.T_2)
    except T.VerificationError:
        return NOT_FOUND, None, None
    return OK, pr, t.challenge_scalar(b"x")


def candidate(key32, V, x, e_blinding):
    """e_j of one key, and the trace of its seed derivation"""
    seed, prefix_pos, ran = seed_traced(key32, V)
    # the one-permutation claim: the key leaves the state at 91, and the only Keccak-f up to the seed is the PRF's own, below the rate
    assert prefix_pos == PREFIX_POS and len(ran) == 1 and ran[0] == PRF_POS and ran[0] < RATE, (prefix_pos, ran)
    d = R.draws(seed, 2)
    return (d[0] + d[1] * x - e_blinding) % L, seed, ran[0]


def scan(pc_gens, state, proof, V, n, keys, commit=None):
    """-> (status, key index, value, 16-byte message, blinding as an int, PRF position); the key index is NONE and the three data outputs
    are zero unless the status is OK.  keys: a list of 32-byte keys."""
    none = (NONE, 0, bytes(16), 0)
    st, pr, x = replay(state, proof, V, n)
    if st != OK:
        return (st,) + none + (None,)
    jstar, seed, pos = NONE, None, None
    for j, key in enumerate(keys):
        e, s, pos = candidate(key, V, x, pr.e_blinding)
        if jstar == NONE and e >> 192 == 0:
            jstar, seed = j, s
    if jstar == NONE:
        return (NOT_FOUND,) + none + (pos,)
    st, v, msg, gamma = R.rewind(pc_gens, state, proof, V, n, seed, commit)
    if st != OK:
        return (NOT_FOUND,) + none + (pos,)
    return OK, jstar, v, msg, gamma, pos


def forge_e_blinding(state, proof, V, n, key32, e=0):
    """The proof's bytes with e_blinding rewritten so that `key32` passes the 2^192 test with candidate e (e_blinding is absorbed after
    x, so x does not move): what an adversary who knows a key's seed can write."""
    st, pr, x = replay(state, proof, V, n)
    assert st == OK and e >> 192 == 0
    d = R.draws(seed_for(key32, V), 2)
    eb = (d[0] + d[1] * x - e) % L
    return proof[:128 + 64] + eb.to_bytes(32, "little") + proof[128 + 96:]
