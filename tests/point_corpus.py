"""ristretto255 encodings sorted by WHICH of RFC 9496's five decoding checks they fail, for every test that feeds a decoder.

A decode is the conjunction  canonical && !s_negative && was_square && !t_negative && y != 0.  `failed_checks` carries the RFC's
formulas to the end on Python big ints and reports each check on its own (C, N, Q, T, Y), where bp_twin.decompress (and every
decoder under test) may stop at the first one.  REJECT holds, for each check, encodings that fail that check AND NO OTHER, found by
search from both ends of the range, so that a decoder which lost one term of the conjunction accepts a member; ACCEPT holds the
valid ends of the range and hashed points whose from_uniform_bytes representative takes each branch of the encoder (the
representative a decoder makes of ANY encoding takes neither: coset() gives the others).  Constants and point arithmetic come from bp_twin;
the decision does not.  (tests/test_point_corpus.py proves every claim made here.)"""
import hashlib

import bp_twin as T

P = T.P
CLASSES = "CNQTY"
MASK255 = (1 << 255) - 1


def enc(v):
    return v.to_bytes(32, "little")


def decode_full(b):
    """RFC 9496 section 4.3.1 carried to the end: (failed checks, (x, y, 1, t)).

    s is the low 255 bits reduced mod p (what the kernels' fe_from_words and dalek's from_bytes form).  C: the 32 bytes are not
    the canonical encoding of s (bit 255 set, or the low 255 bits >= p).  N uses the RAW bit 0 of the encoding, as the kernels
    do; dalek takes the sign of the reduced value -- the two differ only where C fails already, so the verdict is the same.
    Q: v u2^2 is not a non-zero square (SQRT_RATIO_M1's was_square; 0 counts as not square, its inverse root does not exist).
    T: t = x y is negative.  Y: y = 0."""
    raw = int.from_bytes(b, "little")
    assert len(b) == 32
    s = (raw & MASK255) % P
    failed = set()
    if raw != s:
        failed.add("C")
    if raw & 1:
        failed.add("N")
    ss = s * s % P
    u1, u2 = (1 - ss) % P, (1 + ss) % P
    u2s = u2 * u2 % P
    v = (-(T.D * u1 % P * u1) - u2s) % P
    ok, inv = T.invsqrt(v * u2s % P)
    dx = inv * u2 % P
    dy = inv * dx % P * v % P
    x = T.fabs(2 * s * dx % P)
    y = u1 * dy % P
    t = x * y % P
    if not ok:
        failed.add("Q")
    if t & 1:
        failed.add("T")
    if y == 0:
        failed.add("Y")
    return frozenset(failed), (x, y, 1, t)


def failed_checks(b):
    """The subset of "CNQTY" that the 32 bytes fail; empty = a valid encoding.  (Sign convention of N: see decode_full.)"""
    return decode_full(b)[0]


def compress_steps(p):
    """RFC 9496 section 4.3.2 step by step: (encoding, rotate, negate_y) -- the encoder's two data-dependent decisions."""
    X, Y, Z, Tt = p
    u1 = (Z + Y) * (Z - Y) % P
    u2 = X * Y % P
    _, inv = T.invsqrt(u1 * u2 % P * u2 % P)
    i1, i2 = inv * u1 % P, inv * u2 % P
    zinv = i1 * i2 % P * Tt % P
    rotate = bool(Tt * zinv % P & 1)
    den = i2
    if rotate:
        X, Y = Y * T.SQRT_M1 % P, X * T.SQRT_M1 % P
        den = i1 * T.INVSQRT_A_MINUS_D % P
    negate = bool(X * zinv % P & 1)
    if negate:
        Y = (-Y) % P
    return enc(T.fabs(den * (Z - Y) % P)), rotate, negate


# E[4], the kernel of the map onto the ristretto group: (0, 1), (0, -1), (i, 0), (-i, 0) in extended coordinates
E4 = [(0, 1, 1, 0), (0, P - 1, 1, 0), (T.SQRT_M1, 0, 1, 0), (P - T.SQRT_M1, 0, 1, 0)]


def coset(p):
    """The four Edwards representatives p + T, T in E[4], of one ristretto element; extended coordinates, each with its own Z != 1."""
    out = []
    for k, t4 in enumerate(E4):
        q = T.pt_add(p, t4)
        z = int.from_bytes(hashlib.shake_256(b"coset-z%d" % k + enc(q[0])).digest(32), "little") % (P - 2) + 2
        q = tuple(c * z % P for c in q)
        assert q[2] != 1 and q[0] * q[1] % P == q[2] * q[3] % P
        out.append(q)
    return out


def _search(want, values, count):
    found = []
    for v in values:
        if failed_checks(enc(v)) == want:
            found.append(v)
            if len(found) == count:
                break
    return found


SEARCH = 400   # how far from each end of the range the search looks


def _build():
    accept, reject = [], []
    # ---- valid: the identity, the smallest and the largest valid s
    ident = bytes(32)
    assert not failed_checks(ident)
    small = _search(frozenset(), range(1, SEARCH), 5)
    large = _search(frozenset(), range(P - 1, P - SEARCH, -1), 3)
    assert len(small) == 5 and len(large) == 3
    accept.append(("identity", ident))
    accept += [("s=%d" % v, enc(v)) for v in small] + [("s=p-%d" % (P - v), enc(v)) for v in large]
    # hashed points: each of the encoder's decisions taken and not taken on the hashed representative, two points per combination
    need = {(r, n): 2 for r in (False, True) for n in (False, True)}
    i = 0
    while any(need.values()):
        pt = T.from_uniform_bytes(hashlib.shake_256(b"corpus-accept-%d" % i).digest(64))
        e, rot, neg = compress_steps(pt)
        if need[(rot, neg)]:
            need[(rot, neg)] -= 1
            accept.append(("hashed%d rotate=%d negate=%d" % (i, rot, neg), e))
        i += 1
        assert i < 400
    # ---- one check alone, from both ends of the range
    for c in "NQTY":
        lo = _search(frozenset(c), range(1, SEARCH), 4)
        hi = _search(frozenset(c), range(P - 1, P - SEARCH, -1), 3)
        reject += [("%s alone s=%d" % (c, v), enc(v), frozenset(c)) for v in lo]
        reject += [("%s alone s=p-%d" % (c, P - v), enc(v), frozenset(c)) for v in hi]
    # C alone: a valid encoding with bit 255 set (a decoder that masks the top bit and forgets the comparison accepts it)
    for name, e in accept:
        reject.append(("C alone: bit 255 | " + name, e[:31] + bytes([e[31] | 0x80]), frozenset("C")))
    # ---- the 19 non-canonical values below 2^255, all ones, and the two roots of -1 (t = v u2^2 = 0: the chain runs on zero)
    for k in range(19):
        e = enc(P + k)
        reject.append(("p+%d" % k, e, failed_checks(e)))
    reject.append(("ff..ff", b"\xff" * 32, failed_checks(b"\xff" * 32)))
    for name, v in (("sqrt(-1)", T.SQRT_M1), ("-sqrt(-1)", P - T.SQRT_M1)):
        reject.append((name, enc(v), failed_checks(enc(v))))
    return accept, reject


ACCEPT, REJECT = _build()                 # [(name, 32 bytes)], [(name, 32 bytes, frozenset of failed checks)]
ACCEPT_ENC = [e for _, e in ACCEPT]
REJECT_ENC = [e for _, e, _ in REJECT]
ALL_ENC = ACCEPT_ENC + REJECT_ENC


def alone(c):
    """The members that fail check c and no other."""
    return [e for _, e, f in REJECT if f == frozenset(c)]


def one_per_class():
    """One member for each of C, N, Q, T, Y that fails that check alone: [(class, encoding)].  The C member is a non-identity
    valid encoding with bit 255 set, the Y member is p - 1 (there is no other)."""
    out = []
    for c in CLASSES:
        m = alone(c)
        out.append((c, m[1] if c == "C" else m[0]))   # (m[0] of C is 00..0080, the identity with the top bit)
    return out


def valid_points(n, tag):
    """n valid encodings (hashed points) for the terms around a member."""
    return [T.compress(T.from_uniform_bytes(hashlib.shake_256(b"corpus-%s-%d" % (tag, i)).digest(64))) for i in range(n)]


def scalars(n, tag):
    return [(int.from_bytes(hashlib.shake_256(b"corpus-sc-%s-%d" % (tag, i)).digest(64), "little") % T.L).to_bytes(32, "little") for i in range(n)]


def reject_batch(nterms, tag, members=None, gap=2):
    """A batch of MSMs of `nterms` terms each: one per member of REJECT (the member at a position that moves with the member's
    index, valid terms around it) and a fully valid MSM after every `gap` of them.  Returns (scalars, points, is_reject flags):
    the byte strings of all MSMs in order, flags[b] = the b-th MSM holds a member."""
    members = REJECT_ENC if members is None else members
    S, Pp, flags = [], [], []
    for i, m in enumerate(members):
        pts = valid_points(nterms, tag + b"-r%d" % i)
        pts[(5 * i + i // nterms) % nterms] = m
        S += scalars(nterms, tag + b"-r%d" % i)
        Pp += pts
        flags.append(True)
        if i % gap == gap - 1:
            S += scalars(nterms, tag + b"-v%d" % i)
            Pp += valid_points(nterms, tag + b"-v%d" % i)
            flags.append(False)
    return b"".join(S), b"".join(Pp), flags


# ---- batches shared by the host tests (device headers compiled for the CPU) and the GPU tests (the shipped library) ---------------
def put(buf, i, e):
    """buf with its i-th 32-byte element replaced by e"""
    return buf[:32 * i] + e + buf[32 * i + 32:]


def top_bit(e):
    """e with bit 255 set: the same s for a decoder that masks the bit, non-canonical for one that compares"""
    return e[:31] + bytes([e[31] | 0x80])


def check_msm_form(call, oracle, nterms, tag, members=None, accept=None):
    """The three batches of one MSM form: call(n_terms list, scalars, points) -> (encodings, status bytes).
    (1) reject_batch: status 1 and a zero encoding for exactly the members' MSMs, the valid ones == oracle; (2) one MSM over the
    ACCEPT members with the edge scalars == oracle; (3) for every ACCEPT member 1 P returns its own bytes and 1 P + 1 (-P) zeros.
    The decoded representative of an encoding always takes rotate = 0, negate = 0 in the encoder, so (3) runs the untaken
    branches only where the form leaves the point as decoded; the taken branches are reached by the random sums of (1) and (2),
    by the multiples of l that the bucket forms stir into the scalars, and by name in the host encoder test on coset()."""
    import limb_corpus as LC
    S, Pp, flags = reject_batch(nterms, tag, members)
    out, st = call([nterms] * len(flags), S, Pp)
    w = 32 * nterms
    for b, rej in enumerate(flags):
        if rej:
            assert st[b] == 1 and out[32 * b:32 * b + 32] == bytes(32), (tag, b, Pp[w * b:w * b + w].hex())
        else:
            est, eout = oracle.msm(S[w * b:w * b + w], Pp[w * b:w * b + w])
            assert est == 0 and st[b] == 0 and out[32 * b:32 * b + 32] == eout, (tag, b)
    acc = ACCEPT_ENC if accept is None else accept
    es = LC.msm_edge_scalars()
    s = b"".join(es[(3 * i + 1) % len(es)].to_bytes(32, "little") for i in range(len(acc)))
    out, st = call([len(acc)], s, b"".join(acc))
    assert st[0] == 0 and out[:32] == oracle.msm(s, b"".join(acc))[1], tag
    one = (1).to_bytes(32, "little")
    nt, s, p = [], b"", b""
    for e in acc:
        nt += [1, 2]
        s += one * 3
        p += e + e + T.compress(T.pt_neg(decode_full(e)[1]))
    out, st = call(nt, s, p)
    for i, e in enumerate(acc):
        assert st[2 * i] == 0 and st[2 * i + 1] == 0 and out[64 * i:64 * i + 32] == e and out[64 * i + 32:64 * i + 64] == bytes(32), (tag, e.hex())


def rp_positions(n, m):
    """Every point of an (n, m) range proof: [(name, position class 'head' | 'L' | 'R' | 'V', 'proof' | 'coms', byte offset)] --
    A, S, T_1, T_2, every L_j and R_j, every V_j"""
    k = (n * m).bit_length() - 1
    out = [("A", "head", "proof", 0), ("S", "head", "proof", 32), ("T_1", "head", "proof", 64), ("T_2", "head", "proof", 96)]
    for j in range(k):
        out += [("L_%d" % j, "L", "proof", 224 + 64 * j), ("R_%d" % j, "R", "proof", 256 + 64 * j)]
    return out + [("V_%d" % j, "V", "coms", 32 * j) for j in range(m)]


def rp_mutate(pr, coms, where, off, e):
    """(proof, commitments) with the point at `off` of the proof or of the commitments replaced by e"""
    if where == "proof":
        return pr[:off] + e + pr[off + 32:], coms
    return pr, coms[:off] + e + coms[off + 32:]


def rp_mutants(pr, coms, n, m):
    """[(name, rejected, proof, commitments)]: one mutated proof per (position, class), a valid proof after every second one"""
    seq = []
    for name, _, where, off in rp_positions(n, m):
        for cls, e in one_per_class():
            seq.append((name + " " + cls, True) + rp_mutate(pr, coms, where, off, e))
            if len(seq) % 3 == 2:
                seq.append(("valid", False, pr, coms))
    return seq


def ipp_verify_variants(inst, n):
    """(names, instances) of InnerProductProof::verify: the valid instance first and last; a member of each class as P, Q, one G_i,
    one H_i; the RIGHT P, Q, G_1, H_{n-1} with bit 255 set.  None of these bases enters the transcript: every variant but the
    valid one must turn Ok into VerificationError by the decoder's decision alone."""
    variants, names = [dict(inst)], ["valid"]
    for k, (cls, e) in enumerate(one_per_class()):
        for key, idx in (("P", 0), ("Q", 0), ("G", (3 * k + 1) % n), ("H", (5 * k + 2) % n)):
            variants.append(dict(inst, **{key: put(inst[key], idx, e)}))
            names.append("%s %s[%d]" % (cls, key, idx))
    for key, idx in (("P", 0), ("Q", 0), ("G", 1), ("H", n - 1)):
        variants.append(dict(inst, **{key: put(inst[key], idx, top_bit(inst[key][32 * idx:32 * idx + 32]))}))
        names.append("bit 255 of the valid %s[%d]" % (key, idx))
    return names + ["valid"], variants + [dict(inst)]


def ipp_create_cases(inst, n):
    """(Q, G, H, expected status) per proof of an InnerProductProof::create batch: a member of each class as Q, as one G_i, as one
    H_i voids that proof (status 1), the untouched instance between them gives the proof"""
    Q, G, H, expect = [inst["Q"]], [inst["G"]], [inst["H"]], [0]
    for k, (cls, e) in enumerate(one_per_class()):
        Q += [e, inst["Q"], inst["Q"], inst["Q"]]
        G += [inst["G"], put(inst["G"], (2 * k + 1) % n, e), inst["G"], inst["G"]]
        H += [inst["H"], inst["H"], put(inst["H"], (3 * k) % n, e), inst["H"]]
        expect += [1, 1, 1, 0]
    return b"".join(Q), b"".join(G), b"".join(H), expect


def linear_verify_cases(li, n):
    """[(name, instance)] of LinearProof::verify: valid; a member of each class as C, one G_i, F, B; the right C with bit 255 set"""
    cases = [("valid", li)]
    for k, (cls, e) in enumerate(one_per_class()):
        cases += [("%s C" % cls, dict(li, C=e)), ("%s G" % cls, dict(li, G=put(li["G"], (3 * k + 2) % n, e))), ("%s F" % cls, dict(li, F=e)),
                  ("%s B" % cls, dict(li, B=e))]
    return cases + [("bit 255 of the valid C", dict(li, C=top_bit(li["C"])))]


def audit_share_cases(r, n, m):
    """(names, party indices, shares, bit commitments, poly commitments) from oracle.prove_shares' result r: the honest shares; a
    member of each class as V_j, A_j, S_j, T_1j, T_2j; and the share's OWN V_j, A_j, S_j, T_1j, T_2j with bit 255 set -- the
    commitments are in no transcript, so there a decoder without the canonical check would accept the share."""
    sl = 32 * (3 + 2 * n)
    S = [r["shares"][sl * j:sl * (j + 1)] for j in range(m)]
    BC = [r["bit_commitments"][96 * j:96 * j + 96] for j in range(m)]
    PCm = [r["poly_commitments"][64 * j:64 * j + 64] for j in range(m)]
    names, idx, sh, bc, pc = ["valid"] * m, list(range(m)), list(S), list(BC), list(PCm)

    def add(name, j, b_, p_):
        names.append(name); idx.append(j); sh.append(S[j]); bc.append(b_); pc.append(p_)
    for k, (cls, e) in enumerate(one_per_class()):
        j = k % m
        for w in range(3):          # V_j, A_j, S_j
            add("%s bit[%d]" % (cls, w), j, put(BC[j], w, e), PCm[j])
        for w in range(2):          # T_1j, T_2j
            add("%s poly[%d]" % (cls, w), j, BC[j], put(PCm[j], w, e))
    for j in range(m):
        for w in range(3):
            add("bit 255 of the valid bit[%d] of party %d" % (w, j), j, put(BC[j], w, top_bit(BC[j][32 * w:32 * w + 32])), PCm[j])
        for w in range(2):
            add("bit 255 of the valid poly[%d] of party %d" % (w, j), j, BC[j], put(PCm[j], w, top_bit(PCm[j][32 * w:32 * w + 32])))
    add("valid", m - 1, BC[m - 1], PCm[m - 1])
    return names, idx, sh, bc, pc
