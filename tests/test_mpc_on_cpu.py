"""The multi-party aggregation protocol without a GPU: the per-lane bodies of csrc/mpc_party.h and csrc/mpc_dealer.h compiled for the
host (tests/mpc_harness) against the oracle's messages (oracle.prove_shares), the grouping-by-position plan as a pure host function,
and the Python typestate rules of bulletproofs_amd/range_proof_mpc.py that need no device."""
import ctypes as C
import hashlib
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "bulletproofs_amd", "csrc")
L = 2**252 + 27742317777372353535851937790883648493
SHAPES = [(8, 1), (8, 2), (16, 4), (64, 2)]


@pytest.fixture(scope="module")
def H():
    d = os.path.join(HERE, "mpc_harness")
    so, src = os.path.join(d, "libmpcharness.so"), os.path.join(d, "harness.cpp")
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    lib = C.CDLL(so)
    lib.mh_plan_cap.restype = C.c_uint64
    lib.mh_plan_cap.argtypes = [C.c_uint64, C.c_uint64]
    return lib


def _u32(xs):
    return (C.c_uint32 * max(len(xs), 1))(*xs)


def _case(oracle, g, n, m, tag):
    vals = [int.from_bytes(hashlib.shake_256(b"%s-v%d" % (tag, i)).digest(8), "little") % (1 << n) for i in range(m)]
    bl = b"".join(hashlib.shake_256(b"%s-b%d" % (tag, i)).digest(31) + b"\x00" for i in range(m))
    r = oracle.prove_shares(g, vals, bl, n, b"mpc on cpu", tag)
    per = 64 * (2 * n + 2)
    stream = hashlib.shake_256(tag).digest(m * per + 128 * m)
    return vals, bl, r, stream[:m * per], stream[m * per:]


def _party(H, n, pos, vals, bl, rng1, chal, rng2, xs, npos=4):
    nr = len(pos)
    row = 2 * n + 2
    bufs = [C.create_string_buffer(k * nr) for k in (64, 64 * row, 128, 96, 32 * (3 + 2 * n), 1, 1)]
    ns = H.mh_party(n, nr, npos, _u32(pos), (C.c_uint64 * nr)(*vals), bl, rng1, chal, 1 if len(chal) == 64 and nr > 1 else 0, rng2, xs,
                    1 if len(xs) == 32 and nr > 1 else 0, *bufs)
    assert ns > 0 and ns % 64 == 0
    return [b.raw for b in bufs]


@pytest.mark.parametrize("n,m", SHAPES)
def test_party_bodies_match_the_oracles_messages(H, oracle, n, m):
    """Scalar rows x the position's generators (ids from mpc_fill_ids) = the oracle's V_j, A_j, S_j, T_1_j, T_2_j; t(x) from the
    coefficients = the share's t_x; the share at x = the oracle's, byte for byte."""
    g = oracle.Gens(64, 4)
    G, Hh, B, Bb = g.export()
    flat = [Bb, B] + [G[32 * i:32 * i + 32] for i in range(64 * 4)] + [Hh[32 * i:32 * i + 32] for i in range(64 * 4)]
    vals, bl, r, rng1, rng2 = _case(oracle, g, n, m, b"cpu-%d-%d" % (n, m))
    y_z, x = r["challenges"][:64], r["challenges"][64:]
    rows_v, rows_as, rows_t, coeffs, shares, st2, st3 = _party(H, n, list(range(m)), vals, bl, rng1, y_z, rng2, x)
    assert st2 == bytes(m) and st3 == bytes(m)
    assert shares == r["shares"]
    row = 2 * n + 2
    xi = int.from_bytes(x, "little")
    sl = 32 * (3 + 2 * n)
    for j in range(m):
        ids = (C.c_uint32 * row)()
        H.mh_ids(n, j, 64, 4, ids)
        assert list(ids[:2]) == [0, 1] and list(ids[2:2 + n]) == [2 + 64 * j + i for i in range(n)] and list(ids[2 + n:]) == [2 + 256 + 64 * j + i for i in range(n)]
        pts = b"".join(flat[i] for i in ids)
        bc, pc = r["bit_commitments"][96 * j:96 * j + 96], r["poly_commitments"][64 * j:64 * j + 64]
        assert oracle.msm(rows_v[64 * j:64 * j + 64], Bb + B) == (0, bc[:32])
        assert oracle.msm(rows_as[64 * row * j:64 * row * j + 32 * row], pts) == (0, bc[32:64])
        assert oracle.msm(rows_as[64 * row * j + 32 * row:64 * row * (j + 1)], pts) == (0, bc[64:])
        assert oracle.msm(rows_t[128 * j:128 * j + 64], Bb + B) == (0, pc[:32])
        assert oracle.msm(rows_t[128 * j + 64:128 * j + 128], Bb + B) == (0, pc[32:])
        t0, t1, t2 = (int.from_bytes(coeffs[96 * j + 32 * q:96 * j + 32 * q + 32], "little") for q in range(3))
        assert (t0 + t1 * xi + t2 * xi * xi) % L == int.from_bytes(shares[sl * j:sl * j + 32], "little")


def test_party_rows_of_several_sessions_shuffled_and_a_lone_position_3(H, oracle):
    """rows of (8, 1), (8, 2), (8, 4) sessions shuffled into one run with per-row challenges: every share equals its session's; a lone
    party at position 3 equals row 3 of the m = 4 session."""
    g = oracle.Gens(64, 4)
    n, rows = 8, []
    for m in (1, 2, 4):
        vals, bl, r, rng1, rng2 = _case(oracle, g, n, m, b"mix-%d" % m)
        for j in range(m):
            rows.append((j, vals[j], bl[32 * j:32 * j + 32], rng1[64 * 18 * j:64 * 18 * (j + 1)], r["challenges"][:64], rng2[128 * j:128 * j + 128], r["challenges"][64:],
                         r["shares"][32 * 19 * j:32 * 19 * (j + 1)]))
    random.Random(5).shuffle(rows)
    out = _party(H, n, [q[0] for q in rows], [q[1] for q in rows], *(b"".join(q[k] for q in rows) for k in (2, 3, 4, 5, 6)))
    assert out[4] == b"".join(q[7] for q in rows)
    lone = [q for q in rows if q[0] == 3]
    out = _party(H, n, [3], [lone[0][1]], *(lone[0][k] for k in (2, 3, 4, 5, 6)))
    assert out[4] == lone[0][7]


def test_zero_and_non_canonical_challenges(H, oracle):
    """x = 0: MaliciousDealer and a zero share for that row only; a non-canonical x, y or z: BAD_SCALAR."""
    g = oracle.Gens(64, 4)
    n, m = 8, 2
    vals, bl, r, rng1, rng2 = _case(oracle, g, n, m, b"zero")
    x = r["challenges"][64:]
    out = _party(H, n, [0, 1], vals, bl, rng1, r["challenges"][:64], rng2, bytes(32) + x)
    sl = 32 * 19
    assert out[6] == bytes([1, 0]) and out[4][:sl] == bytes(sl) and out[4][sl:] == r["shares"][sl:]
    out = _party(H, n, [0, 1], vals, bl, rng1, r["challenges"][:64], rng2, x + b"\xff" * 32)
    assert out[6] == bytes([0, 3]) and out[4][:sl] == r["shares"][:sl] and out[4][sl:] == bytes(sl)
    out = _party(H, n, [0, 1], vals, bl, rng1, r["challenges"][:64] + L.to_bytes(32, "little") + r["challenges"][32:64], rng2, x)
    assert out[5] == bytes([0, 3]) and out[2][128:] == bytes(128) and out[4][:sl] == r["shares"][:sl]


@pytest.mark.parametrize("n,m", SHAPES)
def test_dealer_bodies_sums_concatenation_and_h_factors(H, oracle, n, m):
    g = oracle.Gens(64, 4)
    cases = [_case(oracle, g, n, m, b"deal-%d-%d-%d" % (n, m, q))[2] for q in range(2)]
    ns, nm, sl = len(cases), n * m, 32 * (3 + 2 * n)
    sums, bad = C.create_string_buffer(96 * ns), C.create_string_buffer(m * ns)
    a, b, hf = (C.create_string_buffer(32 * nm * ns) for _ in range(3))
    assert H.mh_dealer(n, m, ns, b"".join(c["shares"] for c in cases), b"".join(c["challenges"][:32] for c in cases), sums, bad, a, b, hf) == 0
    assert bad.raw == bytes(m * ns)
    for p, c in enumerate(cases):
        assert sums.raw[96 * p:96 * p + 96] == c["proof"][128:224]          # t_x, t_x_blinding, e_blinding of the proof
        sh = [c["shares"][sl * j:sl * (j + 1)] for j in range(m)]
        assert a.raw[32 * nm * p:32 * nm * (p + 1)] == b"".join(s[96:96 + 32 * n] for s in sh)
        assert b.raw[32 * nm * p:32 * nm * (p + 1)] == b"".join(s[96 + 32 * n:] for s in sh)
        yinv = pow(int.from_bytes(c["challenges"][:32], "little"), L - 2, L)
        assert hf.raw[32 * nm * p:32 * nm * (p + 1)] == b"".join(pow(yinv, i, L).to_bytes(32, "little") for i in range(nm))
    t = bytearray(cases[0]["shares"] + cases[1]["shares"])                   # a non-canonical l_vec entry of party m - 1 of session 1
    o = sl * m + sl * (m - 1) + 96
    t[o:o + 32] = b"\xff" * 32
    assert H.mh_dealer(n, m, ns, bytes(t), b"".join(c["challenges"][:32] for c in cases), sums, bad, a, b, hf) == 0
    assert bad.raw == bytes(m) + bytes(m - 1) + b"\x01"
    assert a.raw[:32 * nm] == b"".join(cases[0]["shares"][sl * j + 96:sl * j + 96 + 32 * n] for j in range(m)) and a.raw[32 * nm:] == bytes(32 * nm)


@pytest.mark.parametrize("nrows", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("kind", ["random", "all-equal", "one-of-each"])
def test_grouping_by_position_is_a_permutation_with_position_uniform_wavefronts(H, nrows, kind):
    rnd = random.Random(nrows * 7 + len(kind))
    pos = {"random": [rnd.randrange(4) for _ in range(nrows)], "all-equal": [2] * nrows, "one-of-each": [r % 4 for r in range(nrows)]}[kind]
    cap = H.mh_plan_cap(nrows, 4)
    row_slot, slot_row, blk_pos = (C.c_uint32 * nrows)(), (C.c_uint32 * cap)(*([0xffffffff] * cap)), (C.c_uint32 * (cap // 64))()
    ns = H.mh_plan(nrows, _u32(pos), 4, row_slot, slot_row, blk_pos)
    assert ns % 64 == 0 and nrows <= ns <= cap and ns <= nrows + 63 * len(set(pos))
    live = [s for s in range(ns) if slot_row[s] != 0xffffffff]
    assert sorted(slot_row[s] for s in live) == list(range(nrows)) and sorted(row_slot) == live       # a permutation of the rows onto the live slots
    assert all(slot_row[row_slot[r]] == r for r in range(nrows))                                      # the inverse restores the caller's order
    for b in range(ns // 64):
        group = [slot_row[s] for s in range(64 * b, 64 * b + 64) if slot_row[s] != 0xffffffff]
        assert group and all(pos[r] == blk_pos[b] for r in group)                                     # every wavefront is position-uniform
    for j in set(pos):                                                                                # rows keep their order inside a position
        mine = [row_slot[r] for r in range(nrows) if pos[r] == j]
        assert mine == sorted(mine)


# ---- the Python typestates ------------------------------------------------------------------------------------------------------
class _FakeCtx:
    """records calls; stands in for a Context so that the typestate rules run without a device"""

    def __init__(self):
        self.calls = []

    def mpc_party_bit_commit(self, n, idx, vals, bl, rng=None):
        self.calls.append("bit")
        return bytes(96), bytearray(b"\x11" * 64)

    def mpc_party_poly_commit(self, n, st, ch, rng=None):
        self.calls.append("poly")
        return bytes(64), bytearray(b"\x22" * 64), bytes(1)

    def mpc_party_proof_share(self, n, st, x):
        self.calls.append("share")
        zero = x == bytes(32)
        return bytes(32 * (3 + 2 * n)), bytes([1 if zero else 0])


class _FakeGens:
    gens_capacity, party_capacity = 64, 4

    def __init__(self):
        self.ctx = _FakeCtx()


def test_typestates_are_consumed_and_party_blobs_are_zeroed():
    import bulletproofs_amd.range_proof_mpc as M
    gens = _FakeGens()
    p0 = M.Party.new(gens, None, 5, b"\x07" * 32, 8)
    bl0 = p0._blob
    p1, bc = p0.assign_position(1)
    assert isinstance(bc, M.BitCommitment) and bl0 == bytearray(32)
    with pytest.raises(M.StateConsumed):
        p0.assign_position(1)
    blob1 = p1._blob
    assert any(blob1)
    p2, pc = p1.apply_challenge(M.BitChallenge(bytes(64)))
    assert blob1 == bytearray(len(blob1)) and isinstance(pc, M.PolyCommitment)
    with pytest.raises(M.StateConsumed):
        p1.apply_challenge(M.BitChallenge(bytes(64)))
    blob2 = p2._blob
    with pytest.raises(M.MPCError.MaliciousDealer):
        p2.apply_challenge(M.PolyChallenge(bytes(32)))
    assert blob2 == bytearray(len(blob2))
    with pytest.raises(M.StateConsumed):
        p2.apply_challenge(M.PolyChallenge(b"\x01" + bytes(31)))
    assert gens.ctx.calls == ["bit", "poly", "share"]
    q1, _ = M.Party.new(gens, None, 5, bytes(32), 8).assign_position(0)       # dropped without a transition: zeroed too
    blob = q1._blob
    del q1
    assert blob == bytearray(len(blob))


def test_parameter_and_count_errors_need_no_device():
    import bulletproofs_amd.range_proof_mpc as M
    from bulletproofs_amd.api import Transcript
    gens = _FakeGens()
    with pytest.raises(M.MPCError.InvalidBitsize):
        M.Party.new(gens, None, 5, bytes(32), 12)
    with pytest.raises(M.MPCError.InvalidBitsize):
        M.Dealer.new(gens, None, None, 12, 2)
    with pytest.raises(M.MPCError.InvalidAggregation):
        M.Dealer.new(gens, None, None, 8, 3)
    with pytest.raises(M.MPCError.InvalidGeneratorsLength):
        M.Dealer.new(gens, None, None, 8, 8)
    with pytest.raises(M.MPCError.InvalidGeneratorsLength):
        M.Party.new(gens, None, 5, bytes(32), 8).assign_position(4)
    assert all(issubclass(getattr(M.MPCError, v), M.MPCError) for v in ("MaliciousDealer", "InvalidBitsize", "InvalidAggregation", "InvalidGeneratorsLength",
                                                                        "WrongNumBitCommitments", "WrongNumPolyCommitments", "WrongNumProofShares", "MalformedProofShares"))
    assert M.MPCError.MalformedProofShares([1, 3]).bad_shares == [1, 3]

    class T:   # a transcript stand-in: the count checks come before any call into the library
        state, fresh_label = bytes(208), None
    d0 = M.Dealer.new(gens, None, T(), 8, 2)
    with pytest.raises(M.MPCError.WrongNumBitCommitments):
        d0.receive_bit_commitments([M.BitCommitment(bytes(96))])
    d1 = M.DealerAwaitingPolyCommitments(d0, bytes(192), bytes(64), bytes(64))
    with pytest.raises(M.MPCError.WrongNumPolyCommitments):
        d1.receive_poly_commitments([M.PolyCommitment(bytes(64))] * 3)
    d2 = M.DealerAwaitingProofShares(d1, bytes(128), bytes(32))
    for call in (d2.receive_shares, d2.receive_trusted_shares, d2.receive_shares_with_rng):
        with pytest.raises(M.MPCError.WrongNumProofShares):
            call([M.ProofShare(bytes(32 * 19))])
    with pytest.raises(M.MPCError.MalformedProofShares) as e:                 # check_size: a share of another bitsize names its party
        d2.receive_shares([M.ProofShare(bytes(32 * 19)), M.ProofShare(bytes(32 * 35))])
    assert e.value.bad_shares == [1]
    with pytest.raises(M.StateConsumed):
        d2.receive_trusted_shares([M.ProofShare(bytes(32 * 19))] * 2)
    assert Transcript is not None


def test_message_types_round_trip_and_check_their_length():
    import bulletproofs_amd.range_proof_mpc as M
    from bulletproofs_amd.api import FormatError
    for cls, size in ((M.BitCommitment, 96), (M.BitChallenge, 64), (M.PolyCommitment, 64), (M.PolyChallenge, 32), (M.ProofShare, 32 * 19)):
        raw = bytes(range(1, 33)) * (size // 32)
        msg = cls.from_bytes(raw)
        assert msg.to_bytes() == raw and msg == cls(raw)
        for wrong in (raw[:-1], raw + b"\x00", b""):
            with pytest.raises(FormatError):
                cls.from_bytes(wrong)
    with pytest.raises(FormatError):
        M.ProofShare.from_bytes(bytes(32 * 20))                               # 3 + 2n elements: an even count is no share
    assert M.ProofShare(bytes(32 * 131)).n == 64
    bc = M.BitCommitment(bytes(range(96)))
    assert (bc.V_j, bc.A_j, bc.S_j) == (bytes(range(32)), bytes(range(32, 64)), bytes(range(64, 96)))
