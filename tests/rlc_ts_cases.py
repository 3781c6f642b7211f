"""Inputs shared by tests/test_gpu_rlc_ts.py and tests/test_gpu_rlc_mixed_ts.py: range proofs the oracle makes on PRE-BOUND transcripts
(oracle.prove_ts), the five kinds of bad member, and what the oracle expects of each proof (oracle.verify_ts).  Every set is made once
per session and never modified: the tests build their calls from copies."""
import hashlib

L = 2**252 + 27742317777372353535851937790883648493
KINDS = ("tampered", "noncanonical", "identity_L", "undecodable_A", "wrong_history")
CONTRIBUTES = ("good", "tampered", "wrong_history")   # reach the final check with every point decoding: they are in R

_cache = {}


def bound_state(oracle, i, differing=True, shared=False):
    """A transcript the application bound before the proof is checked, as _bound_state of tests/test_gpu_transcripts.py: protocol label,
    session id, an earlier challenge -- then a message whose length moves the STROBE position (a challenge resets it, so the message follows
    the challenge).  differing: the length depends on i; else every i sits at one position with its own sponge words; shared: one state."""
    j = 0 if shared else i
    st = oracle.transcript_new(b"payment-protocol v3")
    st = oracle.transcript_append_message(st, b"session", hashlib.shake_256(b"sess%d" % j).digest(40 + j % 7))
    st, _ = oracle.transcript_challenge_bytes(st, b"binding", 16)
    ln = (13 * j + 5) % 166 if differing and not shared else 21
    return oracle.transcript_append_message(st, b"amount-commitment-context", hashlib.shake_256(b"ctx%d" % j).digest(ln))


def proofs_on_states(oracle, gens, n, m, count, mode, tag):
    """count good proofs of shape (n, m), proof i made on its own bound state; mode: "differing" / "uniform" positions, or "shared"
    (one state).  Returns {"n", "m", "pl", "proofs": [..], "coms": [..], "states": [..]} (cached)."""
    key = (n, m, count, mode, tag)
    if key not in _cache:
        proofs, coms, states = [], [], []
        for i in range(count):
            st = bound_state(oracle, i + 1000 * len(tag), differing=mode == "differing", shared=mode == "shared")
            vals = [int.from_bytes(hashlib.shake_256(b"%sv%d-%d" % (tag, i, j)).digest(8), "little") % (1 << n) for j in range(m)]
            bl = b"".join(hashlib.shake_256(b"%sb%d-%d" % (tag, i, j)).digest(31) + b"\x00" for j in range(m))
            pr, cm, _ = oracle.prove_ts(gens, vals, bl, n, st, b"%ss%d" % (tag, i))
            proofs.append(pr), coms.append(cm), states.append(st)
        _cache[key] = {"n": n, "m": m, "pl": oracle.proof_len(n, m), "proofs": tuple(proofs), "coms": tuple(coms), "states": tuple(states)}
    return _cache[key]


def with_bad_members(oracle, group, where):
    """a copy of the group with the bad member `kind` at index where[kind]; returns (group, kinds) with kinds[i] = "good" or the kind"""
    proofs, states, kinds = list(group["proofs"]), list(group["states"]), ["good"] * len(group["proofs"])
    for kind, i in where.items():
        pr = bytearray(proofs[i])
        if kind == "tampered":
            pr[130] ^= 1                                   # t_x
        elif kind == "noncanonical":
            pr[128:160] = b"\xff" * 32                     # t_x >= l: FormatError, the transcript is never touched
        elif kind == "identity_L":
            pr[224 + 64:224 + 96] = bytes(32)              # L_1 = the identity encoding: the replay stops at that message
        elif kind == "undecodable_A":
            pr[0] |= 1                                     # a negative s: no Ristretto point
        elif kind == "wrong_history":
            states[i] = bound_state(oracle, 777000 + i)    # the right proof on another transcript
        proofs[i] = bytes(pr)
        kinds[i] = kind
    g = dict(group)
    g["proofs"], g["states"] = tuple(proofs), tuple(states)
    return g, kinds


def as_call_group(group, lo=0, hi=None, shared=False):
    """(n, m, proofs, proof_len, commitments, states) as Context.rangeproof_verify_rlc_mixed_ts takes it"""
    sl = slice(lo, hi)
    return (group["n"], group["m"], b"".join(group["proofs"][sl]), group["pl"], b"".join(group["coms"][sl]),
            group["states"][lo] if shared else b"".join(group["states"][sl]))


def oracle_expectation(oracle, gens, group):
    """[(rc, mega-check encoding, end state)] per proof of the group, rng bytes from the caller"""
    def run(rng):
        return [oracle.verify_ts(gens, pr, cm, group["n"], st, rng[64 * i:64 * i + 64])
                for i, (pr, cm, st) in enumerate(zip(group["proofs"], group["coms"], group["states"]))]
    return run


def combined_point(oracle, exps, kinds, wts):
    """R = sum rho_i MegaCheck_i as ONE oracle MSM over the mega-check encodings oracle.verify_ts returned, rho_i = weights64[i] mod l, over
    the proofs that contribute"""
    sc, pt = b"", b""
    for i, ((rc, enc, _), kind) in enumerate(zip(exps, kinds)):
        if kind in CONTRIBUTES:
            assert rc in (0, 1)
            sc += (int.from_bytes(wts[64 * i:64 * i + 64], "little") % L).to_bytes(32, "little")
            pt += enc
    st, out = oracle.msm(sc, pt)
    assert st == 0
    return out


def rand64(tag, total):
    return hashlib.shake_256(tag).digest(64 * total)
