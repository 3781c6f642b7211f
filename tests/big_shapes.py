"""Range proofs of 32 to 1024 parties for the tests of the large shapes (test_big_shapes_on_cpu.py, test_gpu_big_shapes.py).  Test-only.

The front end takes n in {8, 16, 32, 64}, m a power of two, lg(n m) <= BP_RP_MAX_K = 16.  Launch 1 of a narrow chain (k_rp_stage1_coop,
csrc/k_rp1.hip) stages the script and the proof's bytes in LDS when they fit four capacities; SHAPES lists, per capacity, a shape on
each side of it.  Every proof comes from the oracle's prover on seeded values and is made once per session (functools.lru_cache);
every expected verdict comes from the oracle's verifier, never from this file."""
import ctypes as C
import functools
import hashlib

import pyoracle as O

LABEL = b"big shapes"

# (n, m): the branch of launch 1 the shape is here for (U = 4 + 2k + m; stage = 8 (9 + 2k) + 8 m words; test_big_shapes_on_cpu.py
# asserts every claim from the compiled capacities)
SHAPES = {
    (16, 32): "the script has exactly RP_COOP_MASKS_CAP masks: staged, sops filled to its last word",
    (32, 32): "RP_COOP_MASKS_CAP masks or one more, by the caller's STROBE position: staged or not",
    (8, 64): "smallest shape with nothing staged (proof + commitments > RP_COOP_STAGE_WORDS, masks > RP_COOP_MASKS_CAP)",
    (64, 64): "operations at RP_COOP_OPS_CAP with U <= RP_DEFER_CAP",
    (8, 128): "U > RP_DEFER_CAP: the coefficients are recoded by the leader, not parked",
    (64, 128): "k = 13, U > RP_DEFER_CAP",
    (8, 1024): "U > 1000",
    (64, 1024): "the documented maximum, k = BP_RP_MAX_K",
}
CONTROL = (64, 16)   # everything staged
TS_SHAPES = ((32, 32), (8, 64), (8, 128))   # the shapes verified on callers' own transcripts
N_PROOFS = {s: (1 if s == (64, 1024) else 3) for s in list(SHAPES) + [CONTROL, (64, 1)]}


def lg(x):
    return x.bit_length() - 1


@functools.lru_cache(maxsize=None)
def gens(gens_capacity, party_capacity):
    return O.Gens(gens_capacity, party_capacity)


def gens_for(n, m):
    """the oracle's generators the shape is checked on: one (64, 128) set for everything it holds (share j's chain does not depend on the
    capacities), a set of its own for the 1024-party shapes"""
    return gens(64, 128) if m <= 128 else gens(n, m)


def _values(n, m, p):
    """seeded values of proof p; 0 and 2^n - 1 at party 0, at party m - 1 and at a party >= 64"""
    top = (1 << n) - 1
    v = [int.from_bytes(hashlib.shake_256(b"bigv-%d-%d-%d-%d" % (n, m, p, j)).digest(8), "little") & top for j in range(m)]
    edge = [(0, top), (top, 0), (top, top)][p % 3]
    v[0], v[m - 1] = edge
    if m > 64:
        v[64], v[m - 2] = edge[1], edge[0]
        v[m // 2 + 3] = top if p == 0 else 0
    return v


def _blindings(n, m, p):
    return b"".join(hashlib.shake_256(b"bigb-%d-%d-%d-%d" % (n, m, p, j)).digest(31) + b"\x00" for j in range(m))


@functools.lru_cache(maxsize=None)
def proofs(n, m):
    """[(proof, commitments)] * N_PROOFS on Transcript::new(LABEL), distinct values, blindings and prover randomness"""
    cnt = N_PROOFS[(n, m)]
    vals = [x for p in range(cnt) for x in _values(n, m, p)]
    bl = b"".join(_blindings(n, m, p) for p in range(cnt))
    pr, cm = O.prove_batch(gens_for(n, m), vals, bl, m, n, LABEL, b"big-%d-%d" % (n, m), threads=min(cnt, 4))
    pl = O.proof_len(n, m)
    return [(pr[pl * p:pl * (p + 1)], cm[32 * m * p:32 * m * (p + 1)]) for p in range(cnt)]


@functools.lru_cache(maxsize=None)
def proof_on(n, m, p, state):
    """(proof, commitments, advanced state) of proof p's values made on the caller's transcript `state` (208 bytes)"""
    return O.prove_ts(gens_for(n, m), _values(n, m, p), _blindings(n, m, p), n, state, b"bigts-%d-%d-%d" % (n, m, p))


def tamper(n, m, proof, coms):
    """the tampered variants of one proof: name -> (proof, commitments).  Offsets: A S T_1 T_2 t_x t_x_blinding e_blinding, then L_i R_i
    at 224 + 64 i, then a, b."""
    k = lg(n * m)
    out = {}

    def var(name, po=None, co=None):
        p, c = bytearray(proof), bytearray(coms)
        if po:
            po(p)
        if co:
            co(c)
        out[name] = (bytes(p), bytes(c))

    def flip(off, bit=1):
        def f(b):
            b[off] ^= bit
        return f

    def ident_l_last(b):
        b[224 + 64 * (k - 1):224 + 64 * (k - 1) + 32] = bytes(32)

    def swap(c):
        c[:32], c[32 * (m - 1):32 * m] = c[32 * (m - 1):32 * m], c[:32]

    def noncanonical(b):
        b[160:192] = b"\xff" * 32

    var("t_x", flip(128))
    var("a", flip(224 + 64 * k))
    var("A", flip(1, 4))
    var("L_last_identity", ident_l_last)
    var("last_commitment", None, flip(32 * (m - 1) + 1, 4))
    var("swapped_commitments", None, swap)
    if m > 64:
        var("commitment_64_undecodable", None, flip(32 * 64, 1))   # an odd (negative) field element: no canonical encoding
    var("t_x_blinding_noncanonical", noncanonical)
    return out


@functools.lru_cache(maxsize=None)
def variants(n, m):
    """tamper() of the shape's first proof"""
    return tamper(n, m, *proofs(n, m)[0])


def batch(n, m, nb, bad=("t_x", "swapped_commitments", "t_x_blinding_noncanonical", "last_commitment", "L_last_identity", "a", "A", "commitment_64_undecodable")):
    """nb proofs tiled from the cached ones, every fifth place (and the last) a tampered variant in turn: (proofs, commitments)"""
    good, var = proofs(n, m), variants(n, m)
    names = [b for b in bad if b in var]
    pr, cm, nbad = [], [], 0
    for i in range(nb):
        if names and (i % 5 == 2 or (i == nb - 1 and nb > 1)):
            q = var[names[nbad % len(names)]]
            nbad += 1
        else:
            q = good[i % len(good)]
        pr.append(q[0])
        cm.append(q[1])
    return b"".join(pr), b"".join(cm)


def rng64(tag, nb):
    return hashlib.shake_256(b"bigrng-" + tag).digest(64 * nb)


def expected(n, m, prfs, coms, rng, label=LABEL, threads=8):
    """the oracle's verdict bytes and mega-check encodings for a batch"""
    _, ev, em = O.verify_batch(gens_for(n, m), prfs, coms, m, n, label, rng, threads=threads)
    return ev, em


def expected_ts(n, m, prfs, coms, states, rng):
    """oracle.verify_ts per proof: verdict bytes, encodings, advanced states; states: one 208-byte state or one per proof"""
    pl = O.proof_len(n, m)
    nb = len(prfs) // pl
    v, e, t = [], [], []
    for i in range(nb):
        st = states if len(states) == 208 else states[208 * i:208 * (i + 1)]
        rc, enc, ts = O.verify_ts(gens_for(n, m), prfs[pl * i:pl * (i + 1)], coms[32 * m * i:32 * m * (i + 1)], n, st, rng[64 * i:64 * i + 64])
        v.append(rc)
        e.append(enc)
        t.append(ts)
    return bytes(v), b"".join(e), b"".join(t)


# ---- start states ---------------------------------------------------------------------------------------------------------------
def padded_state(pad, label=LABEL):
    """Transcript::new(label) with one message of every length in `pad` appended (the paddings of the golden-shape transcript test)"""
    st = O.transcript_new(label)
    for j, ln in enumerate(pad):
        st = O.transcript_append_message(st, b"pad%d" % j, bytes((ln + q) & 0xff for q in range(ln)))
    return st


def with_domsep(st, n, m):
    st = O.transcript_append_message(st, b"dom-sep", b"rangeproof v1")
    st = O.transcript_append_message(st, b"n", n.to_bytes(8, "little"))
    return O.transcript_append_message(st, b"m", m.to_bytes(8, "little"))


def session_state(who, ln):
    """a caller's transcript with a `ln`-byte message of its own: states of one `ln` share their STROBE position, not their words"""
    return O.transcript_append_message(O.transcript_new(b"big app"), b"session", hashlib.shake_256(b"sess-%d" % who).digest(ln))


PADS = ([], [0], [1], [7], [60], [100, 3], [165], [166], [167, 9], [40, 40, 40])


def counts(n, m, state, domsep=True):
    """(U, stage words, n_ops, n_masks) of launch 1 for the shape, from the position of a 208-byte start state; domsep: the state does
    not hold rangeproof_domain_sep(n, m) yet (callers' transcripts), else it does (label calls)"""
    import harness_lib
    out = (C.c_uint32 * 4)()
    assert harness_lib.lib().h_rp_script_counts(n, m, state[200], state[201], state[202], 1 if domsep else 0, out) == 0
    return tuple(out)


def label_counts(n, m, label=LABEL):
    """... for a call that brings a label: the host applies the domain separator, the script starts behind it"""
    return counts(n, m, with_domsep(O.transcript_new(label), n, m), domsep=False)


def caps():
    import harness_lib
    f = harness_lib.lib().h_rp_coop_cap
    f.restype = C.c_uint32
    return dict(stage_words=f(0), ops=f(1), masks=f(2), defer=f(3), max_k=f(4), vb_chunk=f(5))


@functools.lru_cache(maxsize=None)
def session_lengths_32_32():
    """two session-message lengths at which a (32, 32) script has RP_COOP_MASKS_CAP masks (staged) and one more (not staged)"""
    cap = caps()["masks"]
    at = {}
    for ln in range(1, 166):
        at.setdefault(counts(32, 32, session_state(0, ln))[3], ln)
    assert cap in at and cap + 1 in at, at
    return at[cap], at[cap + 1]
