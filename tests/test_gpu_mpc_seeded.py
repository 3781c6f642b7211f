"""The seeded party steps on the GPU (bpgpu_mpc_party_bit_commit_seeded, bpgpu_mpc_party_poly_commit_seeded): a party's rng is
ChaChaRng::from_seed(seed) advanced by first_draw scalars, every draw a ChaCha20 block computed by the lane that consumes it.  The
CONTRACT is parity with the unseeded calls on the expanded keystream (the ChaCha20 of oracle/py/chacha_rng.py, vectorised below and
pinned against it); on top of it a seeded multi-party session reproduces bpgpu_rangeproof_prove_batch_ts byte for byte."""
import ctypes as C
import hashlib
import random

import numpy as np
import pytest

import chacha_rng as CR

pytestmark = pytest.mark.gpu
L = CR.L
U64 = 2**64
NROWS = 70   # over four positions: two or more wavefronts per call, every position's run padded, the row-to-slot map not the identity


# ---- the keystream, many blocks at once -----------------------------------------------------------------------------------------
def _rotl(x, r):
    return (x << np.uint32(r)) | (x >> np.uint32(32 - r))


def blocks(seeds, counters):
    """ChaCha20 blocks (64-bit counter, stream id 0) of seeds[k] at counters[k], as in oracle/py/chacha_rng.chacha20_block"""
    k = len(counters)
    key = np.frombuffer(b"".join(seeds), dtype="<u4").reshape(k, 8).T
    ctr = np.array(counters, dtype=np.uint64)
    st = [np.full(k, c, dtype=np.uint32) for c in (0x61707865, 0x3320646e, 0x79622d32, 0x6b206574)] + [key[q].copy() for q in range(8)]
    st += [(ctr & np.uint64(0xffffffff)).astype(np.uint32), (ctr >> np.uint64(32)).astype(np.uint32), np.zeros(k, np.uint32), np.zeros(k, np.uint32)]
    x = [w.copy() for w in st]

    def qr(a, b, c, d):
        x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 16)
        x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 12)
        x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 8)
        x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 7)
    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    out = np.stack([a + b for a, b in zip(x, st)], axis=1).astype("<u4").tobytes()
    return [out[64 * q:64 * q + 64] for q in range(k)]


def keystream(seed, first, ndraws):
    return b"".join(blocks([seed] * ndraws, [first + d for d in range(ndraws)]))


def check_keystream():
    """the vectorised blocks are the oracle's, across the carry into the counter's high word and up to block 2^64 - 1"""
    seed = bytes(range(7, 39))
    for first in (0, 5, 2**32 - 3, 2**64 - 18):
        assert keystream(seed, first, 18) == b"".join(CR.chacha20_block(seed, first + d) for d in range(18))


# ---- contexts and rows ----------------------------------------------------------------------------------------------------------
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


_ROWS, _WANT = {}, {}


def _h(tag, what, r, k):
    return hashlib.shake_256(b"%s-%s-%d" % (tag, what, r)).digest(k)


def rows_of(n):
    """NROWS independent parties of bitsize n: positions over 0..3 in shuffled order, distinct seeds, first draws mixed over 0, 2n + 2 and
    2^32 - 3 (the 2n + 2 draws straddle the carry into the counter's high word) in both steps; y, z, x canonical and per row"""
    if n not in _ROWS:
        if not _ROWS:
            check_keystream()
        tag = b"seeded-%d" % n
        pos = [r % 4 for r in range(NROWS)]
        random.Random(n).shuffle(pos)
        firsts = [0, 2 * n + 2, 2**32 - 3]
        rows = []
        for r in range(NROWS):
            f1 = firsts[r % 3]
            f2 = f1 + 2 * n + 2 if r % 2 else firsts[(r // 2) % 3]   # carried on from step 1, or a position of its own
            seed = _h(tag, b"s", r, 32)
            rows.append(dict(pos=pos[r], v=int.from_bytes(_h(tag, b"v", r, 8), "little"), bl=_h(tag, b"b", r, 32), seed=seed, f1=f1, f2=f2,
                             chal=_h(tag, b"y", r, 31) + b"\x00" + _h(tag, b"z", r, 31) + b"\x00", x=_h(tag, b"x", r, 31) + b"\x00",
                             rng1=keystream(seed, f1, 2 * n + 2), rng2=keystream(seed, f2, 2)))
        assert pos != sorted(pos) and len({q["seed"] for q in rows}) == NROWS
        _ROWS[n] = rows
    return _ROWS[n]


def cat(rows, k):
    return b"".join(q[k] for q in rows)


def col(rows, k):
    return [q[k] for q in rows]


def unseeded(c, n, rows):
    bc, st1 = c.mpc_party_bit_commit(n, col(rows, "pos"), col(rows, "v"), cat(rows, "bl"), cat(rows, "rng1"))
    pc, st2, status = c.mpc_party_poly_commit(n, st1, cat(rows, "chal"), cat(rows, "rng2"))
    sh, status3 = c.mpc_party_proof_share(n, st2, cat(rows, "x"))
    return dict(bc=bc, st1=bytes(st1), pc=pc, st2=bytes(st2), status=status, sh=sh, status3=status3)


def want_of(ctx, n):
    """the unseeded calls on the expanded keystream, computed once per bitsize and left unchanged"""
    if n not in _WANT:
        _WANT[n] = unseeded(ctx, n, rows_of(n))
        assert _WANT[n]["status"] == bytes(NROWS) and _WANT[n]["status3"] == bytes(NROWS)
    return _WANT[n]


def seeded(c, n, rows, f1="f1", f2="f2"):
    bc, st1 = c.mpc_party_bit_commit(n, col(rows, "pos"), col(rows, "v"), cat(rows, "bl"), rng_seed32=cat(rows, "seed"), first_draw=f1 and col(rows, f1))
    assert c.get_option("staging_residue") == 0                  # seeds cleared with the working set on the way out
    pc, st2, status = c.mpc_party_poly_commit(n, st1, cat(rows, "chal"), rng_seed32=cat(rows, "seed"), first_draw=f2 and col(rows, f2))
    assert c.get_option("staging_residue") == 0
    return dict(bc=bc, st1=bytes(st1), pc=pc, st2=bytes(st2), status=status)


def same(got, want, n, nrows=NROWS):
    """every output of every row, byte for byte"""
    for k in ("bc", "st1", "pc", "st2", "status"):
        w = len(want[k]) // nrows
        for r in range(nrows):
            assert got[k][w * r:w * (r + 1)] == want[k][w * r:w * (r + 1)], (k, n, r)


# ---- 1: row parity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 64])
def test_seeded_rows_equal_the_unseeded_calls_on_the_keystream(ctx, n):
    same(seeded(ctx, n, rows_of(n)), want_of(ctx, n), n)


@pytest.mark.parametrize("n", [8, 64])
def test_first_draw_null_is_0_in_bit_commit_and_2n_plus_2_in_poly_commit(ctx, n):
    rows = [dict(q, f1=0, f2=2 * n + 2) for q in rows_of(n)]
    explicit = seeded(ctx, n, rows)
    same(seeded(ctx, n, rows, None, None), explicit, n)
    head = [dict(q, rng1=keystream(q["seed"], 0, 2 * n + 2), rng2=keystream(q["seed"], 2 * n + 2, 2)) for q in rows[:5]]   # ... and 0, 2n + 2 they are
    want = unseeded(ctx, n, head)
    for k in ("bc", "st1", "pc", "st2"):
        assert explicit[k][:len(want[k])] == want[k], k


# ---- 2: a seeded multi-party session is prove_batch_ts ---------------------------------------------------------------------------
def _sessions(oracle, n, m, ns=3):
    tag = b"flow-%d-%d" % (n, m)
    initial = b"".join(oracle.transcript_append_message(oracle.transcript_new(b"seeded mpc"), b"session", b"%s/%d" % (tag, p)) for p in range(ns))
    vals = [int.from_bytes(_h(tag, b"v", i, 8), "little") % (1 << n) for i in range(ns * m)]
    bl = b"".join(_h(tag, b"b", i, 31) + b"\x00" for i in range(ns * m))
    seeds = [_h(tag, b"s", p, 32) for p in range(ns)]
    return initial, vals, bl, seeds


def _flow(c, n, m, ns, initial, vals, bl, seeds, trusted):
    """parties seeded at j (2n + 2) -> bit challenge -> seeded poly commit at m (2n + 2) + 2j -> poly challenge -> shares -> assemble.
    seeds None: rng32 = NULL in both party steps."""
    idx = [j for _ in range(ns) for j in range(m)]
    s32 = None if seeds is None else b"".join(seeds[p] for p in range(ns) for _ in range(m))
    bc, st1 = c.mpc_party_bit_commit(n, idx, vals, bl, rng_seed32=s32, first_draw=[j * (2 * n + 2) for j in idx])
    ch, _, ts, st4 = c.mpc_dealer_bit_challenge(n, m, bc, transcripts=initial)
    pc, st2, s2 = c.mpc_party_poly_commit(n, st1, b"".join(ch[64 * p:64 * p + 64] * m for p in range(ns)), rng_seed32=s32,
                                          first_draw=[m * (2 * n + 2) + 2 * j for j in idx])
    x, _, ts, st5 = c.mpc_dealer_poly_challenge(m, pc, ts)
    sh, s3 = c.mpc_party_proof_share(n, st2, b"".join(x[32 * p:32 * p + 32] * m for p in range(ns)))
    chal = b"".join(ch[64 * p:64 * p + 64] + x[32 * p:32 * p + 32] for p in range(ns))
    proofs, bad, st6, ts = c.mpc_dealer_assemble(n, m, sh, bc, pc, chal, ts, initial_transcripts=initial, trusted=trusted)
    assert s2 == s3 == bytes(ns * m) and st4 == st5 == bytes(ns) and bad == bytes(ns * m)
    return bc, proofs, st6, ts


@pytest.mark.parametrize("n,m", [(8, 2), (64, 4)])
def test_a_seeded_session_equals_prove_batch_ts_on_the_sessions_seed_and_transcript(ctx, oracle, n, m):
    ns = 3
    initial, vals, bl, seeds = _sessions(oracle, n, m, ns)
    bc, proofs, st6, ts = _flow(ctx, n, m, ns, initial, vals, bl, seeds, trusted=True)
    eproofs, ecoms, ets = ctx.rangeproof_prove_batch_ts(n, m, vals, bl, initial, b"".join(seeds), want_transcripts=True)
    assert st6 == bytes(ns)
    pl = len(eproofs) // ns
    for p in range(ns):
        assert proofs[pl * p:pl * (p + 1)] == eproofs[pl * p:pl * (p + 1)], p
        assert ts[208 * p:208 * (p + 1)] == ets[208 * p:208 * (p + 1)], p
    assert b"".join(bc[96 * r:96 * r + 32] for r in range(ns * m)) == ecoms
    assert ctx.rangeproof_verify_batch_ts(n, m, proofs, pl, ecoms, initial) == bytes(ns)


# ---- 3: seeded and unseeded steps interoperate ----------------------------------------------------------------------------------
def test_a_seeded_step_feeds_an_unseeded_one_and_the_reverse(ctx):
    n = 8
    rows, want = rows_of(n), want_of(ctx, n)
    pos, v, bl, seed = col(rows, "pos"), col(rows, "v"), cat(rows, "bl"), cat(rows, "seed")
    _, st1 = ctx.mpc_party_bit_commit(n, pos, v, bl, rng_seed32=seed, first_draw=col(rows, "f1"))
    pc, st2, _ = ctx.mpc_party_poly_commit(n, st1, cat(rows, "chal"), cat(rows, "rng2"))                       # seeded -> unseeded
    sh, st = ctx.mpc_party_proof_share(n, st2, cat(rows, "x"))
    assert (pc, sh, st) == (want["pc"], want["sh"], bytes(NROWS))
    _, st1 = ctx.mpc_party_bit_commit(n, pos, v, bl, cat(rows, "rng1"))
    pc, st2, _ = ctx.mpc_party_poly_commit(n, st1, cat(rows, "chal"), rng_seed32=seed, first_draw=col(rows, "f2"))   # unseeded -> seeded
    sh, st = ctx.mpc_party_proof_share(n, st2, cat(rows, "x"))
    assert (pc, sh, st) == (want["pc"], want["sh"], bytes(NROWS))


# ---- 4: the constant-time walk --------------------------------------------------------------------------------------------------
def test_prover_constant_time_gives_byte_identical_outputs(ctx, ctx_ct):
    assert ctx_ct.get_option("prover_constant_time") == 1
    same(seeded(ctx_ct, 8, rows_of(8)), want_of(ctx, 8), 8)


# ---- 5: rng32 = NULL ------------------------------------------------------------------------------------------------------------
def test_library_drawn_seeds_differ_between_calls(ctx):
    n, rows = 8, rows_of(8)[:6]
    a, b = (ctx.mpc_party_bit_commit(n, col(rows, "pos"), col(rows, "v"), cat(rows, "bl"), first_draw=[0] * 6)[0] for _ in range(2))
    for r in range(6):
        assert a[96 * r:96 * r + 32] == b[96 * r:96 * r + 32]                                                  # V_j draws nothing
        assert a[96 * r + 32:96 * r + 64] != b[96 * r + 32:96 * r + 64] and a[96 * r + 64:96 * r + 96] != b[96 * r + 64:96 * r + 96], r


@pytest.mark.parametrize("n,m", [(8, 2), (64, 4)])
def test_a_session_on_library_drawn_seeds_passes_the_dealers_verification(ctx, oracle, n, m):
    ns = 3
    initial, vals, bl, _ = _sessions(oracle, n, m, ns)
    bc, proofs, st6, _ = _flow(ctx, n, m, ns, initial, vals, bl, None, trusted=False)
    assert st6 == bytes(ns)                                                                                    # BPGPU_MPC_OK: the dealer verified every proof
    coms = b"".join(bc[96 * r:96 * r + 32] for r in range(ns * m))
    assert ctx.rangeproof_verify_batch_ts(n, m, proofs, len(proofs) // ns, coms, initial) == bytes(ns)


# ---- 6: errors and per-row status -----------------------------------------------------------------------------------------------
def _raw_bit_commit(c, n, rows, first):
    nr = len(rows)
    bc, st = C.create_string_buffer(b"\xaa" * (96 * nr), 96 * nr), C.create_string_buffer(b"\xaa" * (c.mpc_state_bytes(n)[0] * nr), c.mpc_state_bytes(n)[0] * nr)
    rc = c._L.bpgpu_mpc_party_bit_commit_seeded(c.h, n, nr, (C.c_uint32 * nr)(*col(rows, "pos")), (C.c_uint64 * nr)(*col(rows, "v")), cat(rows, "bl"), cat(rows, "seed"),
                                                (C.c_uint64 * nr)(*first), bc, st)
    return rc, bc.raw, st.raw


def _raw_poly_commit(c, n, rows, st1, first):
    nr, s2 = len(rows), c.mpc_state_bytes(n)[1]
    pc, st, status = (C.create_string_buffer(b"\xaa" * (k * nr), k * nr) for k in (64, s2, 1))
    rc = c._L.bpgpu_mpc_party_poly_commit_seeded(c.h, n, nr, bytes(st1), cat(rows, "chal"), 0, cat(rows, "seed"), (C.c_uint64 * nr)(*first), pc, st, status)
    return rc, pc.raw, st.raw, status.raw


@pytest.mark.parametrize("n", [8, 64])
def test_a_first_draw_that_would_wrap_the_counter_is_refused_and_nothing_is_written(ctx, n):
    rows, want = rows_of(n)[:3], want_of(ctx, n)
    invalid = ctx._L.bpgpu_mpc_party_bit_commit_seeded(ctx.h, n, 1, None, None, None, None, None, None, None)   # BPGPU_ERR_INVALID_ARG, here by a NULL argument
    assert invalid != 0
    for bad in (U64 - 1, U64 - (2 * n + 2) + 1):
        rc, bc, st = _raw_bit_commit(ctx, n, rows, [0, bad, 0])
        assert rc == invalid and set(bc) == {0xaa} and set(st) == {0xaa}, bad
    s1 = ctx.mpc_state_bytes(n)[0]
    rc, pc, st, status = _raw_poly_commit(ctx, n, rows, want["st1"][:3 * s1], [0, 0, U64 - 1])
    assert rc == invalid and set(pc) == {0xaa} and set(st) == {0xaa} and set(status) == {0xaa}
    # the last positions that do not wrap are served: draws up to block 2^64 - 1
    last1, last2 = U64 - (2 * n + 2), U64 - 2
    rc, bc, st = _raw_bit_commit(ctx, n, rows, [last1] * 3)
    assert rc == 0
    rc, pc, st2, status = _raw_poly_commit(ctx, n, rows, st, [last2] * 3)
    assert rc == 0 and status == bytes(3)
    edge = unseeded(ctx, n, [dict(q, rng1=keystream(q["seed"], last1, 2 * n + 2), rng2=keystream(q["seed"], last2, 2)) for q in rows])
    assert (bc, st, pc, st2) == (edge["bc"], edge["st1"], edge["pc"], edge["st2"])


def test_a_non_canonical_y_fails_its_row_only(ctx):
    n = 8
    rows, want = [dict(q) for q in rows_of(n)], want_of(ctx, n)
    rows[9]["chal"] = L.to_bytes(32, "little") + rows[9]["chal"][32:]
    got = seeded(ctx, n, rows)
    s2 = ctx.mpc_state_bytes(n)[1]
    assert got["status"] == bytes(9) + b"\x03" + bytes(NROWS - 10)                                             # BPGPU_MPC_BAD_SCALAR
    assert got["pc"][64 * 9:64 * 10] == bytes(64) and got["st2"][s2 * 9:s2 * 10] == bytes(s2)
    for k, w in (("pc", 64), ("st2", s2)):
        assert got[k][:w * 9] == want[k][:w * 9] and got[k][w * 10:] == want[k][w * 10:], k
    _, st1 = ctx.mpc_party_bit_commit(n, col(rows, "pos"), col(rows, "v"), cat(rows, "bl"), cat(rows, "rng1"))
    assert ctx.mpc_party_poly_commit(n, st1, cat(rows, "chal"), cat(rows, "rng2"))[2] == got["status"]        # as the unseeded call


def test_a_state_blob_with_a_wrong_magic_and_an_empty_batch(ctx):
    import bulletproofs_amd as bp
    n = 8
    rows, want = rows_of(n)[:3], want_of(ctx, n)
    s1 = ctx.mpc_state_bytes(n)[0]
    st1 = bytearray(want["st1"][:3 * s1])
    st1[s1] ^= 1                                                                                               # the magic of row 1
    errs = []
    for kw in (dict(rng=cat(rows, "rng2")), dict(rng_seed32=cat(rows, "seed"))):
        with pytest.raises(bp.BpgpuError, match="INVALID_ARG") as e:
            ctx.mpc_party_poly_commit(n, st1, cat(rows, "chal"), **kw)
        errs.append(str(e.value))
    assert errs[0] == errs[1]                                                                                  # as in the unseeded call
    assert ctx.mpc_party_bit_commit(n, [], [], b"", rng_seed32=b"") == (b"", bytearray())                      # nparties = 0: BPGPU_OK
    assert ctx.mpc_party_poly_commit(n, b"", b"", rng_seed32=b"") == (b"", bytearray(), b"")
    assert ctx._L.bpgpu_mpc_party_bit_commit_seeded(ctx.h, n, 0, None, None, None, None, None, None, None) == 0
    assert ctx._L.bpgpu_mpc_party_poly_commit_seeded(ctx.h, n, 0, None, None, 0, None, None, None, None, None) == 0
    with pytest.raises(ValueError):
        ctx.mpc_party_bit_commit(n, col(rows, "pos"), col(rows, "v"), cat(rows, "bl"), cat(rows, "rng1"), rng_seed32=cat(rows, "seed"))
    with pytest.raises(ValueError):
        ctx.mpc_party_poly_commit(n, want["st1"][:3 * s1], cat(rows, "chal"), cat(rows, "rng2"), first_draw=[0, 0, 0])


# ---- 7: the Python typestates ---------------------------------------------------------------------------------------------------
def test_seeded_typestates_reproduce_prove_multiple_with_rng():
    from bulletproofs_amd import BulletproofGens, RangeProof, Transcript
    from bulletproofs_amd.range_proof_mpc import Dealer, Party
    n, m, s, label = 8, 4, bytes(range(100, 132)), b"seeded typestates"
    vals = [3, 250, 0, 77]
    bl = [_h(b"ts", b"b", j, 31) + b"\x00" for j in range(m)]
    gens = BulletproofGens(64, 4)
    pc_gens = gens.pedersen()
    transcript = Transcript(label)
    dealer = Dealer.new(gens, pc_gens, transcript, n, m)
    parties = [Party.new(gens, pc_gens, vals[j], bl[j], n) for j in range(m)]
    with pytest.raises(ValueError):
        parties[0].assign_position_with_rng(0, bytes(64 * (2 * n + 2)), rng_seed32=s)
    parties, bit_coms = zip(*[p.assign_position_with_rng(j, rng_seed32=s, first_draw=j * (2 * n + 2)) for j, p in enumerate(parties)])
    dealer, bit_chal = dealer.receive_bit_commitments(list(bit_coms))
    with pytest.raises(ValueError):
        parties[0].apply_challenge_with_rng(bit_chal, bytes(128), rng_seed32=s)
    parties, poly_coms = zip(*[p.apply_challenge_with_rng(bit_chal, rng_seed32=s, first_draw=m * (2 * n + 2) + 2 * j) for j, p in enumerate(parties)])
    dealer, poly_chal = dealer.receive_poly_commitments(list(poly_coms))
    proof = dealer.receive_shares([p.apply_challenge(poly_chal) for p in parties])
    t2 = Transcript(label)
    want, coms = RangeProof.prove_multiple_with_rng(gens, pc_gens, t2, vals, bl, n, rng_seed32=s)
    assert proof.to_bytes() == want.to_bytes() and [b.V_j for b in bit_coms] == coms and transcript.state == t2.state
    # one party, one rng carried through both steps: the defaults (0, then 2n + 2) are prove_single_with_rng's positions
    t3, t4 = Transcript(label), Transcript(label)
    dealer = Dealer.new(gens, pc_gens, t3, n, 1)
    p, bc = Party.new(gens, pc_gens, 200, bl[0], n).assign_position_with_rng(0, rng_seed32=s)
    dealer, bit_chal = dealer.receive_bit_commitments([bc])
    p, pc = p.apply_challenge_with_rng(bit_chal, rng_seed32=s)
    dealer, poly_chal = dealer.receive_poly_commitments([pc])
    proof = dealer.receive_shares([p.apply_challenge(poly_chal)])
    want, com = RangeProof.prove_single_with_rng(gens, pc_gens, t4, 200, bl[0], n, rng_seed32=s)
    assert proof.to_bytes() == want.to_bytes() and bc.V_j == com and t3.state == t4.state
    gens.ctx.close()
