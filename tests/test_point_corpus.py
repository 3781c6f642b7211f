"""point_corpus.py proves its own claims: every member of REJECT fails exactly the checks it is listed with, each of the five
checks C, N, Q, T, Y has members that fail it ALONE (from both ends of the range where such members exist), failed_checks is
empty exactly where the twin's decoder accepts, the C oracle takes the same decision on every member -- alone and at every lane
position of a wider multiscalar multiplication -- and the four Edwards representatives of an element encode alike."""
import hashlib

import bp_twin as T
import point_corpus as PC

P = T.P


def test_each_check_has_members_that_fail_it_alone_from_both_ends():
    for name, e, want in PC.REJECT:
        assert PC.failed_checks(e) == want and want, name
    for c in PC.CLASSES:
        assert PC.alone(c), c
    lows = {c: [int.from_bytes(e, "little") for e in PC.alone(c) if int.from_bytes(e, "little") < PC.SEARCH] for c in "NQT"}
    highs = {c: [int.from_bytes(e, "little") for e in PC.alone(c) if P - PC.SEARCH < int.from_bytes(e, "little") < P] for c in "NQT"}
    for c in "NQT":
        assert len(lows[c]) >= 3 and len(highs[c]) >= 3, c
    # the members are the FIRST ones from each end: an exhaustive scan of the first and last 40 values begins with them
    for c, lo, hi in (("N", [3, 9, 21, 37], [4, 6, 20]), ("Q", [14, 28, 32, 38], [11, 17, 19]), ("T", [2, 10, 16, 18], [7, 25, 29])):
        assert [v for v in range(1, 40) if PC.failed_checks(PC.enc(v)) == frozenset(c)][:4] == lo
        assert [k for k in range(1, 40) if PC.failed_checks(PC.enc(P - k)) == frozenset(c)][:3] == hi
        assert set(lo) <= set(lows[c]) and {P - k for k in hi} <= set(highs[c])
    # Y alone: s = p - 1 and nothing else within reach of either end (y = 0 needs u1 = 0, s^2 = 1, or a zero inverse root)
    assert PC.alone("Y") == [PC.enc(P - 1)]
    assert [v for v in list(range(PC.SEARCH)) + list(range(P - PC.SEARCH, P)) if PC.failed_checks(PC.enc(v)) == frozenset("Y")] == [P - 1]
    # C alone: every ACCEPT member with bit 255 set, 00..0080 among them; the low 255 bits are still a valid encoding
    ca = PC.alone("C")
    assert bytes(31) + b"\x80" in ca
    for e in PC.ACCEPT_ENC:
        assert e[:31] + bytes([e[31] | 0x80]) in ca
    assert PC.enc(P + 3) in ca and PC.enc(P + 9) in ca            # the two even non-canonical values that reduce to a valid s
    noncanon = [PC.failed_checks(PC.enc(P + k)) for k in range(19)]
    assert all("C" in f for f in noncanon) and [k for k, f in enumerate(noncanon) if f == frozenset("C")] == [3, 9]
    assert "C" not in PC.failed_checks(PC.enc(P - 1)) and PC.enc(P + 18) == b"\xff" * 31 + b"\x7f"
    assert PC.failed_checks(PC.enc(T.SQRT_M1)) | PC.failed_checks(PC.enc(P - T.SQRT_M1)) == frozenset("NQY")
    for v in (T.SQRT_M1, P - T.SQRT_M1):                          # t = v u2^2 = 0 there: u2 = 1 + s^2 = 0
        assert (1 + v * v) % P == 0 and PC.decode_full(PC.enc(v))[1] == (0, 0, 1, 0)
    assert len(set(PC.ALL_ENC)) == len(PC.ALL_ENC)


def test_accept_members_are_valid_and_take_every_branch_of_the_encoder():
    for name, e in PC.ACCEPT:
        f, pt = PC.decode_full(e)
        assert not f, name
        assert PC.compress_steps(pt)[0] == e == T.compress(pt), name
    assert PC.ACCEPT_ENC[0] == bytes(32)
    assert [int.from_bytes(e, "little") for e in PC.ACCEPT_ENC[1:9]] == [4, 6, 20, 22, 30, P - 3, P - 9, P - 21]
    assert [v for v in range(1, 31) if not PC.failed_checks(PC.enc(v))] == [4, 6, 20, 22, 30]
    assert [k for k in range(1, 22) if not PC.failed_checks(PC.enc(P - k))] == [3, 9, 21]
    taken = {}
    for i in range(12):   # the hashed members, re-derived: the decisions of the encoder on the hashed point itself
        pt = T.from_uniform_bytes(hashlib.shake_256(b"corpus-accept-%d" % i).digest(64))
        e, rot, neg = PC.compress_steps(pt)
        assert e == T.compress(pt)
        if e in PC.ACCEPT_ENC:
            taken[(rot, neg)] = taken.get((rot, neg), 0) + 1
    assert all(taken.get((r, n), 0) >= 2 for r in (False, True) for n in (False, True)), taken


def test_failed_checks_is_empty_exactly_where_the_twin_accepts():
    enc = list(PC.ALL_ENC)
    for i in range(300):
        e = hashlib.shake_256(b"pc-rand%d" % i).digest(32)
        enc.append(e if i % 3 == 0 else bytes([e[0] & 0xfe]) + e[1:31] + bytes([e[31] & 0x7f]))
    enc += [PC.enc(v) for v in range(64)] + [PC.enc(P - k) for k in range(1, 64)]
    seen = set()
    for e in enc:
        f, pt = PC.decode_full(e)
        d = T.decompress(e)
        assert (not f) == (d is not None), e.hex()
        if d is not None:
            assert d == pt
        seen.add(f)
    assert frozenset() in seen and all(frozenset(c) in seen for c in PC.CLASSES)


def test_c_oracle_agrees_on_every_member_alone_and_at_every_lane_position(oracle):
    """oracle.msm of one point, and of 9 points with the member at positions 0 .. 8 (every position modulo 4: a build that
    decodes four encodings at a time runs the rejected lanes on zero next to valid ones)."""
    one = (1).to_bytes(32, "little")
    others = PC.valid_points(8, b"oracle")
    sc = PC.scalars(9, b"oracle")
    for algo in (0, 1, 2):
        for e in PC.ALL_ENC:
            bad = bool(PC.failed_checks(e))
            st, out = oracle.msm(one, e, algo)
            assert st == (1 if bad else 0) and out == (bytes(32) if bad else e), e.hex()
            if algo:
                continue
            for pos in range(9):
                pts = others[:pos] + [e] + others[pos:]
                st, out = oracle.msm(b"".join(sc), b"".join(pts))
                if bad:
                    assert st == 1 and out == bytes(32), (e.hex(), pos)
                else:
                    exp = T.msm([int.from_bytes(s, "little") for s in sc], [T.decompress(p) for p in pts])
                    assert st == 0 and out == T.compress(exp), (e.hex(), pos)


def test_the_four_representatives_of_an_element_encode_alike():
    for name, e in PC.ACCEPT:
        pt = PC.decode_full(e)[1]
        reps = PC.coset(pt)
        assert len({(q[0] * T.inv(q[2]) % P, q[1] * T.inv(q[2]) % P) for q in reps}) == 4
        for q in reps:
            assert T.compress(q) == e and PC.compress_steps(q)[0] == e, name
            assert T.pt_eq(q, pt)
    for q in PC.coset(T.IDENT):
        assert T.compress(q) == bytes(32) and T.pt_is_identity(q)


def test_reject_batch_places_each_member_among_valid_terms():
    S, Pp, flags = PC.reject_batch(7, b"self")
    assert len(S) == len(Pp) == 32 * 7 * len(flags) and flags.count(True) == len(PC.REJECT) and flags.count(False) >= len(PC.REJECT) // 2
    k, positions = 0, set()
    for b, fl in enumerate(flags):
        bad = [i for i in range(7) if PC.failed_checks(Pp[32 * (7 * b + i):32 * (7 * b + i) + 32])]
        if fl:
            assert len(bad) == 1 and Pp[32 * (7 * b + bad[0]):32 * (7 * b + bad[0]) + 32] == PC.REJECT_ENC[k]
            positions.add(bad[0])
            k += 1
        else:
            assert not bad
    assert positions == set(range(7))
