"""The multi-party aggregation protocol on the GPU (bpgpu_mpc_*, bulletproofs_amd/range_proof_mpc.py): every message of the three
party steps and the three dealer steps is byte-identical to the oracle's (oracle.prove_shares / prove_ts), with the constant-time walk
on and off, and the reference's own scenarios detect_dishonest_party_during_aggregation (src/range_proof/mod.rs:726-799) and
detect_dishonest_dealer_during_aggregation (mod.rs:800-840)."""
import hashlib
import random

import pytest

import point_corpus as PC

pytestmark = pytest.mark.gpu
LABEL = b"mpc gpu"
L = 2**252 + 27742317777372353535851937790883648493


@pytest.fixture(scope="module")
def ctx():
    import bulletproofs_amd as bp
    c = bp.Context(0)
    c.gens_create(64, 4)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_ct():
    import bulletproofs_amd as bp
    c = bp.Context(0)
    c.gens_create(64, 4)
    c.set_option("prover_constant_time", 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def g(oracle):
    return oracle.Gens(64, 4)


_CACHE = {}


def _session(oracle, g, n, m, seed, vals=None, bl=None, label=LABEL):
    """one oracle session and the random bytes each of its parties drew (SHAKE256(seed) in the prover's draw order); computed once"""
    key = (n, m, seed)
    if key not in _CACHE:
        if vals is None:
            vals = [int.from_bytes(hashlib.shake_256(b"%s-v%d" % (seed, i)).digest(8), "little") % (1 << n) for i in range(m)]
        if bl is None:
            bl = b"".join(hashlib.shake_256(b"%s-b%d" % (seed, i)).digest(31) + b"\x00" for i in range(m))
        r = oracle.prove_shares(g, vals, bl, n, label, seed)
        per = 64 * (2 * n + 2)
        stream = hashlib.shake_256(seed).digest(m * per + 128 * m)
        r.update(n=n, m=m, vals=vals, bl=bl, seed=seed, label=label, rng1=[stream[per * j:per * (j + 1)] for j in range(m)],
                 rng2=[stream[m * per + 128 * j:m * per + 128 * (j + 1)] for j in range(m)])
        _CACHE[key] = r
    return _CACHE[key]


def _rows(sessions):
    """the parties of the sessions as independent rows: (j, v, blinding, rng1, y z, rng2, x, bit commitment, poly commitment, share)"""
    rows = []
    for s in sessions:
        sl = 32 * (3 + 2 * s["n"])
        for j in range(s["m"]):
            rows.append((j, s["vals"][j], s["bl"][32 * j:32 * j + 32], s["rng1"][j], s["challenges"][:64], s["rng2"][j], s["challenges"][64:],
                         s["bit_commitments"][96 * j:96 * j + 96], s["poly_commitments"][64 * j:64 * j + 64], s["shares"][sl * j:sl * (j + 1)]))
    return rows


def _run_parties(c, n, rows, residue=True):
    cat = lambda k: b"".join(q[k] for q in rows)
    bc, st1 = c.mpc_party_bit_commit(n, [q[0] for q in rows], [q[1] for q in rows], cat(2), cat(3))
    if residue:
        assert c.get_option("staging_residue") == 0          # secrets cleared on the way out (prover_exit)
    pc, st2, status2 = c.mpc_party_poly_commit(n, st1, cat(4), cat(5))
    if residue:
        assert c.get_option("staging_residue") == 0
    sh, status3 = c.mpc_party_proof_share(n, st2, cat(6))
    if residue:
        assert c.get_option("staging_residue") == 0
    return bc, pc, sh, status2, status3


def _check_parties(c, n, rows):
    bc, pc, sh, status2, status3 = _run_parties(c, n, rows)
    nr, sl = len(rows), 32 * (3 + 2 * n)
    assert status2 == bytes(nr) and status3 == bytes(nr)
    for r, q in enumerate(rows):
        assert bc[96 * r:96 * r + 96] == q[7], ("bit commitment", r, q[0])
        assert pc[64 * r:64 * r + 64] == q[8], ("poly commitment", r, q[0])
        assert sh[sl * r:sl * (r + 1)] == q[9], ("share", r, q[0])


def _tiled_n8(oracle, g, nrows):
    """sessions (8, 1), (8, 2), (8, 4) tiled with distinct seeds, shuffled together, cut to nrows rows (rows are independent parties)"""
    sessions, t = [], 0
    while 7 * t < nrows:
        sessions += [_session(oracle, g, 8, m, b"t%d-%d" % (t, m)) for m in (1, 2, 4)]
        t += 1
    rows = _rows(sessions)
    random.Random(nrows).shuffle(rows)
    return rows[:nrows]


# ---- 1, 2: party steps ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrows", [7, 65, 130, 160])   # 160: position 0 holds more than 64 rows -- its group crosses a wavefront
def test_party_steps_of_shuffled_sessions_are_byte_identical_to_the_oracle(ctx, oracle, g, nrows):
    _check_parties(ctx, 8, _tiled_n8(oracle, g, nrows))


@pytest.mark.parametrize("n,m", [(16, 4), (32, 2), (64, 4)])
def test_party_steps_of_one_session(ctx, oracle, g, n, m):
    _check_parties(ctx, n, _rows([_session(oracle, g, n, m, b"one-%d-%d" % (n, m))]))


def test_a_lone_party_at_position_3_equals_row_3_of_its_session(ctx, oracle, g):
    rows = _rows([_session(oracle, g, 8, 4, b"t0-4")])
    _check_parties(ctx, 8, [rows[3]])


@pytest.mark.parametrize("n", [8, 64])
def test_party_steps_through_the_constant_time_walk(ctx_ct, oracle, g, n):
    assert ctx_ct.get_option("prover_constant_time") == 1
    rows = _tiled_n8(oracle, g, 7) if n == 8 else _rows([_session(oracle, g, 64, 4, b"one-64-4")])
    _check_parties(ctx_ct, n, rows)


def test_party_steps_with_library_drawn_randomness_audit_clean(ctx, oracle, g):
    """rng = NULL (OS CSPRNG): nothing to compare bytes with -- the dealer's audit accepts every share"""
    n, m = 8, 4
    bc, st1 = ctx.mpc_party_bit_commit(n, list(range(m)), [3, 250, 0, 77], bytes(32 * m))
    ch, _, ts, st = ctx.mpc_dealer_bit_challenge(n, m, bc, LABEL)
    pc, st2, s2 = ctx.mpc_party_poly_commit(n, st1, ch)
    x, _, ts, _ = ctx.mpc_dealer_poly_challenge(m, pc, ts)
    sh, s3 = ctx.mpc_party_proof_share(n, st2, x)
    assert st == bytes(1) and s2 == bytes(m) and s3 == bytes(m)
    assert ctx.rangeproof_audit_shares(n, list(range(m)), sh, bc, pc, ch + x) == bytes(m)
    proof, bad, status, _ = ctx.mpc_dealer_assemble(n, m, sh, bc, pc, ch + x, ts, LABEL)
    assert status == bytes(1) and bad == bytes(m)
    assert ctx.rangeproof_verify_batch(n, m, proof, len(proof), b"".join(bc[96 * j:96 * j + 32] for j in range(m)), LABEL) == bytes(1)


# ---- 3: dealer steps ------------------------------------------------------------------------------------------------------------
def _run_dealer(c, oracle, g, sessions, initial, trusted=False):
    """the three dealer steps over the sessions' oracle messages; initial: None (label) or a 208-byte state shared by the sessions"""
    n, m, label = sessions[0]["n"], sessions[0]["m"], sessions[0]["label"]
    cat = lambda k: b"".join(s[k] for s in sessions)
    ch, AS, ts, st4 = c.mpc_dealer_bit_challenge(n, m, cat("bit_commitments"), label, initial)
    x, T, ts, st5 = c.mpc_dealer_poly_challenge(m, cat("poly_commitments"), ts)
    chal = b"".join(ch[64 * p:64 * p + 64] + x[32 * p:32 * p + 32] for p in range(len(sessions)))
    proofs, bad, st6, ts = c.mpc_dealer_assemble(n, m, cat("shares"), cat("bit_commitments"), cat("poly_commitments"), chal, ts, label, initial, trusted=trusted)
    return chal, AS, T, proofs, bad, st4, st5, st6, ts


@pytest.mark.parametrize("n,m,ns", [(8, 1, 1), (8, 1, 3), (8, 2, 1), (8, 2, 3), (8, 2, 65), (8, 4, 1), (8, 4, 3), (16, 4, 1), (16, 4, 3), (32, 2, 1), (32, 2, 3),
                                    (64, 4, 1), (64, 4, 3)])
@pytest.mark.parametrize("bound", [False, True])
def test_dealer_steps_are_byte_identical_to_the_oracle(ctx, oracle, g, n, m, ns, bound):
    sessions = [_session(oracle, g, n, m, b"d%d-%d-%d" % (n, m, p)) for p in range(ns)]
    initial = oracle.transcript_append_message(oracle.transcript_new(b"application"), b"bound", b"earlier messages") if bound else None
    pl = len(sessions[0]["proof"])
    start = initial if bound else oracle.transcript_new(LABEL)
    if not bound:   # Transcript::new(LABEL): the transcript the oracle's messages were made on
        chal, AS, T, proofs, bad, st4, st5, st6, ts = _run_dealer(ctx, oracle, g, sessions, None)
        assert st4 == st5 == st6 == bytes(ns) and bad == bytes(ns * m)
        for p, s in enumerate(sessions):
            assert chal[96 * p:96 * p + 96] == s["challenges"], p
            assert AS[64 * p:64 * p + 64] == s["proof"][:64] and T[64 * p:64 * p + 64] == s["proof"][64:128], p
            assert proofs[pl * p:pl * (p + 1)] == s["proof"], p
            _, _, ets = oracle.prove_ts(g, s["vals"], s["bl"], n, start, s["seed"])
            assert ts[208 * p:208 * p + 208] == ets, p
    if bound:
        # a pre-bound transcript shared by the sessions.  The oracle's later messages answer the challenges of Transcript::new(LABEL), so the
        # parties here are the GPU's (pinned above against the oracle) with the oracle's randomness: the dealer's sums, proof and final transcript
        # equal prove_multiple_with_rng's on that transcript
        cat = lambda k: b"".join(s[k] for s in sessions)
        rows = _rows(sessions)
        bc, st1 = ctx.mpc_party_bit_commit(n, [q[0] for q in rows], [q[1] for q in rows], b"".join(q[2] for q in rows), b"".join(q[3] for q in rows))
        assert bc == cat("bit_commitments")
        ch, AS, ts, st4 = ctx.mpc_dealer_bit_challenge(n, m, bc, transcripts=initial)
        pc, st2, _ = ctx.mpc_party_poly_commit(n, st1, b"".join(ch[64 * p:64 * p + 64] * m for p in range(ns)), b"".join(q[5] for q in rows))
        x, T, ts, st5 = ctx.mpc_dealer_poly_challenge(m, pc, ts)
        sh, _ = ctx.mpc_party_proof_share(n, st2, b"".join(x[32 * p:32 * p + 32] * m for p in range(ns)))
        chal = b"".join(ch[64 * p:64 * p + 64] + x[32 * p:32 * p + 32] for p in range(ns))
        proofs, bad, st6, ts = ctx.mpc_dealer_assemble(n, m, sh, bc, pc, chal, ts, initial_transcripts=initial)
        assert st4 == st5 == st6 == bytes(ns) and bad == bytes(ns * m)
        for p, s in enumerate(sessions):
            epr, _, ets = oracle.prove_ts(g, s["vals"], s["bl"], n, start, s["seed"])
            assert proofs[pl * p:pl * (p + 1)] == epr and ts[208 * p:208 * p + 208] == ets, p
            assert AS[64 * p:64 * p + 64] == epr[:64] and T[64 * p:64 * p + 64] == epr[64:128], p


# ---- 4: end to end through the typestates ---------------------------------------------------------------------------------------
def test_typestates_end_to_end_proof_equals_the_oracles_and_verifies(oracle, g):
    from bulletproofs_amd import BulletproofGens, RangeProof, Transcript
    from bulletproofs_amd.range_proof_mpc import Dealer, Party
    n, m = 8, 4
    s = _session(oracle, g, n, m, b"t0-4")
    gens = BulletproofGens(64, 4)
    pc_gens = gens.pedersen()
    transcript = Transcript(LABEL)
    dealer = Dealer.new(gens, pc_gens, transcript, n, m)
    parties = [Party.new(gens, pc_gens, s["vals"][j], s["bl"][32 * j:32 * j + 32], n) for j in range(m)]
    parties, bit_coms = zip(*[p.assign_position_with_rng(j, s["rng1"][j]) for j, p in enumerate(parties)])
    dealer, bit_chal = dealer.receive_bit_commitments(list(bit_coms))
    parties, poly_coms = zip(*[p.apply_challenge_with_rng(bit_chal, s["rng2"][j]) for j, p in enumerate(parties)])
    dealer, poly_chal = dealer.receive_poly_commitments(list(poly_coms))
    shares = [p.apply_challenge(poly_chal) for p in parties]
    proof = dealer.receive_shares(shares)
    assert proof.to_bytes() == s["proof"]
    assert bit_chal.to_bytes() + poly_chal.to_bytes() == s["challenges"]
    assert transcript.state == oracle.prove_ts(g, s["vals"], s["bl"], n, oracle.transcript_new(LABEL), s["seed"])[2]   # advanced in place
    proof.verify_multiple(gens, pc_gens, Transcript(LABEL), [b.V_j for b in bit_coms], n)
    gens.ctx.close()


# ---- 5: detect_dishonest_party_during_aggregation -------------------------------------------------------------------------------
def test_detect_dishonest_party_during_aggregation(ctx, oracle, g):
    """mod.rs:726-799: n = 32, four parties, parties 1 and 3 hold 64-bit values (Party::new accepts them).  The bad session shares one assemble
    call with an honest one: MalformedProofShares { bad_shares: [1, 3] } and no proof for it, the honest neighbour untouched."""
    n, m = 32, 4
    rnd = hashlib.shake_256(b"dishonest").digest(8 * 8)
    u = lambda i: int.from_bytes(rnd[8 * i:8 * i + 8], "little")
    bl = b"".join(hashlib.shake_256(b"dbl%d" % i).digest(31) + b"\x00" for i in range(m))
    lab = b"AggregatedRangeProofTest"
    bad = _session(oracle, g, n, m, b"s1", [u(0) & 0xffffffff, u(1) | (1 << 63), u(2) & 0xffffffff, u(3) | (1 << 62)], bl, lab)
    good = _session(oracle, g, n, m, b"s2", [u(4) & 0xffffffff, u(5) & 0xffffffff, u(6) & 0xffffffff, u(7) & 0xffffffff], bl, lab)
    _check_parties(ctx, n, _rows([bad, good]))                       # the GPU parties commit to the oversized values exactly as the reference's do
    pl = len(good["proof"])
    chal, _, _, proofs, named, st4, st5, st6, _ = _run_dealer(ctx, oracle, g, [bad, good], None)
    assert chal == bad["challenges"] + good["challenges"] and st4 == st5 == bytes(2)
    assert st6 == bytes([2, 0])                                      # BPGPU_MPC_MALFORMED_SHARES, BPGPU_MPC_OK
    assert [j for j in range(m) if named[j]] == [1, 3] and named[m:] == bytes(m)
    assert proofs[:pl] == bytes(pl) and proofs[pl:] == good["proof"]
    _, _, _, proofs, named, _, _, st6, _ = _run_dealer(ctx, oracle, g, [bad, good], None, trusted=True)
    assert st6 == bytes(2) and named == bytes(2 * m) and proofs == bad["proof"] + good["proof"]   # receive_trusted_shares: the non-verifying proof comes out
    assert ctx.rangeproof_verify_batch(n, m, proofs, pl, bad["commitments"] + good["commitments"], lab) == bytes([1, 0])


# ---- 6: detect_dishonest_dealer_during_aggregation ------------------------------------------------------------------------------
def test_detect_dishonest_dealer_during_aggregation(ctx, oracle, g):
    """mod.rs:800-840: a zero poly challenge.  One row among honest rows: MALICIOUS_DEALER and a zero share for it, the others unchanged."""
    n = 8
    rows = _tiled_n8(oracle, g, 7)
    cat = lambda k: b"".join(q[k] for q in rows)
    _, st1 = ctx.mpc_party_bit_commit(n, [q[0] for q in rows], [q[1] for q in rows], cat(2), cat(3))
    _, st2, _ = ctx.mpc_party_poly_commit(n, st1, cat(4), cat(5))
    xs = b"".join(bytes(32) if r == 4 else q[6] for r, q in enumerate(rows))
    sh, status = ctx.mpc_party_proof_share(n, st2, xs)
    sl = 32 * 19
    assert status == bytes([0, 0, 0, 0, 1, 0, 0])
    for r, q in enumerate(rows):
        assert sh[sl * r:sl * (r + 1)] == (bytes(sl) if r == 4 else q[9]), r


def test_malicious_dealer_through_the_typestates():
    from bulletproofs_amd import BulletproofGens
    from bulletproofs_amd.range_proof_mpc import BitChallenge, MPCError, Party, PolyChallenge
    gens = BulletproofGens(8, 1)
    p, _ = Party.new(gens, gens.pedersen(), 200, bytes(32), 8).assign_position(0)
    p, _ = p.apply_challenge(BitChallenge((5).to_bytes(32, "little") + (7).to_bytes(32, "little")))
    blob = p._blob
    with pytest.raises(MPCError.MaliciousDealer):
        p.apply_challenge(PolyChallenge(bytes(32)))
    assert blob == bytearray(len(blob))
    gens.ctx.close()


# ---- 7: rejections, each alone --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,e", PC.one_per_class())
def test_an_undecodable_a_j_fails_only_its_session(ctx, oracle, g, cls, e):
    n, m = 8, 2
    sessions = [_session(oracle, g, n, m, b"d8-2-%d" % p) for p in range(3)]
    bc = bytearray(b"".join(s["bit_commitments"] for s in sessions))
    o = 96 * (1 * m + 1) + 32                                        # A_1 of session 1
    bc[o:o + 32] = e
    ch, AS, ts, status = ctx.mpc_dealer_bit_challenge(n, m, bytes(bc), LABEL)
    assert status == bytes([0, 4, 0]), cls                           # BPGPU_MPC_BAD_POINT
    assert ch[64:128] == bytes(64) and AS[64:128] == bytes(64) and ts[208:416] == oracle.transcript_new(LABEL)
    for p in (0, 2):
        assert ch[64 * p:64 * p + 64] == sessions[p]["challenges"][:64] and AS[64 * p:64 * p + 64] == sessions[p]["proof"][:64]
    bc[o:o + 32] = sessions[1]["bit_commitments"][96 + 32:96 + 64]   # the same message in the V_j slot is appended as given, never decoded
    bc[o - 32:o] = e
    ch, _, _, status = ctx.mpc_dealer_bit_challenge(n, m, bytes(bc), LABEL)
    assert status == bytes(3) and ch[:64] == sessions[0]["challenges"][:64] and ch[64:128] != sessions[1]["challenges"][:64]


def test_a_non_canonical_share_scalar_names_its_party(ctx, oracle, g):
    n, m = 8, 4
    sessions = [_session(oracle, g, n, m, b"d8-4-%d" % p) for p in range(2)]
    cat = lambda k: b"".join(s[k] for s in sessions)
    ch, _, ts, _ = ctx.mpc_dealer_bit_challenge(n, m, cat("bit_commitments"), LABEL)
    x, _, ts, _ = ctx.mpc_dealer_poly_challenge(m, cat("poly_commitments"), ts)
    chal = cat("challenges")
    assert chal == b"".join(ch[64 * p:64 * p + 64] + x[32 * p:32 * p + 32] for p in range(2))
    sl, pl = 32 * 19, len(sessions[0]["proof"])
    sh = bytearray(cat("shares"))
    o = sl * (m + 2) + 96 + 32 * 3                                   # l_vec[3] of party 2 of session 1: itself plus the group order
    sh[o:o + 32] = (int.from_bytes(sh[o:o + 32], "little") + L).to_bytes(32, "little")
    for trusted in (False, True):
        proofs, bad, status, _ = ctx.mpc_dealer_assemble(n, m, bytes(sh), cat("bit_commitments"), cat("poly_commitments"), chal, ts, LABEL, trusted=trusted)
        assert status == bytes([0, 2]) and bad == bytes(m) + bytes([0, 0, 1, 0]), trusted
        assert proofs[:pl] == sessions[0]["proof"] and proofs[pl:] == bytes(pl)


def test_parameter_errors(ctx, oracle, g):
    import bulletproofs_amd as bp
    s8 = _session(oracle, g, 8, 1, b"t0-1")
    s82 = _session(oracle, g, 8, 2, b"t0-2")
    s1, s2 = ctx.mpc_state_bytes(12)
    with pytest.raises(bp.BpgpuError, match="InvalidBitsize"):       # n = 12
        ctx.mpc_party_bit_commit(12, [0], [5], bytes(32))
    with pytest.raises(bp.BpgpuError, match="InvalidBitsize"):
        ctx.mpc_party_poly_commit(12, bytes(s1), bytes(64))
    with pytest.raises(bp.BpgpuError, match="InvalidBitsize"):
        ctx.mpc_party_proof_share(12, bytes(s2), bytes(32))
    with pytest.raises(bp.BpgpuError, match="InvalidBitsize"):
        ctx.mpc_dealer_bit_challenge(12, 1, bytes(96), LABEL)
    with pytest.raises(bp.BpgpuError, match="InvalidAggregation"):   # m = 3
        ctx.mpc_dealer_bit_challenge(8, 3, bytes(96 * 3), LABEL)
    with pytest.raises(bp.BpgpuError, match="InvalidAggregation"):
        ctx.mpc_dealer_poly_challenge(3, bytes(64 * 3), oracle.transcript_new(LABEL))
    with pytest.raises(bp.BpgpuError, match="InvalidAggregation"):
        ctx.mpc_dealer_assemble(8, 3, bytes(32 * 19 * 3), bytes(96 * 3), bytes(64 * 3), bytes(96), oracle.transcript_new(LABEL), LABEL)
    with pytest.raises(bp.BpgpuError, match="NO_GENS"):              # j >= party_capacity
        ctx.mpc_party_bit_commit(8, [0, 4], [5, 6], bytes(64))
    with pytest.raises(bp.BpgpuError, match="not supported"):        # n m beyond the prover's limit
        ctx.mpc_dealer_bit_challenge(64, 2048, bytes(96 * 2048), LABEL)
    with pytest.raises(bp.BpgpuError, match="INVALID_ARG"):          # a blob that is no state of the step
        ctx.mpc_party_proof_share(8, bytes(ctx.mpc_state_bytes(8)[1]), bytes(32))
    small = bp.Context(0)
    small.gens_create(8, 1)
    with pytest.raises(bp.BpgpuError, match="NO_GENS"):              # InvalidGeneratorsLength: n = 16 on an (8, 1) set
        small.mpc_party_bit_commit(16, [0], [5], bytes(32))
    with pytest.raises(bp.BpgpuError, match="NO_GENS"):
        small.mpc_dealer_bit_challenge(16, 1, bytes(96), LABEL)
    with pytest.raises(bp.BpgpuError, match="NO_GENS"):              # m = 2
        small.mpc_dealer_bit_challenge(8, 2, s82["bit_commitments"], LABEL)
    with pytest.raises(bp.BpgpuError, match="NO_GENS"):
        small.mpc_party_bit_commit(8, [1], [5], bytes(32))
    bc, _ = small.mpc_party_bit_commit(8, [0], s8["vals"], s8["bl"], s8["rng1"][0])   # what it does hold works
    assert bc == s8["bit_commitments"]
    small.close()
