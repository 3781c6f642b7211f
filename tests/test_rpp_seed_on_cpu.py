"""The seeded range-proof prover without a GPU: rp_prover.h's rpp_draw, the three lane bodies that consume random scalars under either
draw source, and the separator-applying start of the first transcript lane, compiled for the host (tests/rpp_seed_harness) and run lane
by lane -- the draws against the oracle's restatement of rand_chacha's ChaChaRng (pinned by the reference's own golden blindings), the
seed-fed lanes against the buffer-fed ones on the expanded keystream, the transcript against the oracle twin's."""
import ctypes as C
import hashlib
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
L_ORDER = 2**252 + 27742317777372353535851937790883648493
FILL = 0x5a5a5a5a
RPP_FIXED, RPP_PARTY_FIELDS, RPP_T1, RPP_T2 = 5, 9, 7, 8       # rp_prover.h's enums
TS_WORDS = 52


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rppseed") / "librppseed.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "rpp_seed_harness", "harness.cpp")])
    lib = C.CDLL(so)
    lib.rppseed_draw.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_uint32)]
    lib.rppseed_draw.restype = None
    lib.rppseed_role_legacy.restype = None
    lib.rppseed_chal1_sep.restype = None
    return lib


def _draw(harness, seed, d):
    out = (C.c_uint32 * 8)()
    harness.rppseed_draw(seed, d, out)
    return bytes(out)


def _ndraws(n, m):
    return m * (2 * n + 2) + 2 * m


def test_draws_of_the_reference_seed_are_its_golden_blindings(harness):
    """rpp_draw([24] * 32, d), d = 0..7 == the r_j behind the reference's committed value commitments (tests/range_proof.rs:108-113)"""
    from chacha_rng import golden_blindings
    assert [_draw(harness, bytes([24]) * 32, d) for d in range(8)] == golden_blindings()


@pytest.mark.parametrize("tag", [b"a", b"b", b"c"])
def test_draws_follow_chacha_rng_for_every_index_of_the_widest_shape(harness, tag):
    """d = 0..D-1 at (64, 16), the most draws a tested shape takes: draw d == the d-th Scalar::random of ChaChaRng::from_seed(seed)"""
    from chacha_rng import ChaChaRng, scalar_random
    seed = hashlib.shake_256(b"rpp-seed-" + tag).digest(32)
    rng = ChaChaRng(seed)
    D = _ndraws(64, 16)
    assert [_draw(harness, seed, d) for d in range(D)] == [scalar_random(rng) for _ in range(D)]


def _filled(nwords):
    return (C.c_uint32 * max(nwords, 1))(*([FILL] * max(nwords, 1)))


def _arrays(n, m, nproofs, t_rows):
    """the output arrays of the three roles, pre-filled with a pattern; the T_1 / T_2 sums rpp_tcommit reads are reduced scalars"""
    nm, PB = n * m, nproofs * m
    gs = _filled(8 * nproofs * (2 + m) * (2 * nm + 2))
    sL, sR = _filled(8 * nproofs * nm), _filled(8 * nproofs * nm)
    party = _filled(8 * RPP_PARTY_FIELDS * PB)
    for f, rows in ((RPP_T1, t_rows[0]), (RPP_T2, t_rows[1])):
        for pj, x in enumerate(rows):
            for q in range(8):
                party[8 * (f * PB + pj) + q] = (x >> (32 * q)) & 0xffffffff
    return gs, sL, sR, party


@pytest.mark.parametrize("nproofs", [1, 3])
@pytest.mark.parametrize("n,m", [(8, 1), (8, 2), (16, 4), (64, 1)])
def test_seed_fed_lanes_equal_buffer_fed_lanes_on_the_expanded_keystream(harness, n, m, nproofs):
    """every lane of rpp_blind_lane, rpp_bits_lane and rpp_tcommit_lane, once fed rpp_draw(seed_of_p, d) and once the byte buffer
    ChaChaRng(seed).fill_bytes(64 D): gen_scalars rows, sL, sR and party compared whole, word for word (untouched words keep the pattern in
    both), no lane asks for a draw at or past D, and the entry points' own wrappers (rpp_*_thread) leave the same arrays again"""
    from chacha_rng import ChaChaRng
    rnd = random.Random(1000 * n + 10 * m + nproofs)
    D = _ndraws(n, m)
    seeds = [hashlib.shake_256(b"lane-%d-%d-%d-%d" % (n, m, nproofs, p)).digest(32) for p in range(nproofs)]
    buf = b"".join(ChaChaRng(s).fill_bytes(64 * D) for s in seeds)
    assert len(buf) == 64 * D * nproofs
    values = (C.c_uint64 * (nproofs * m))(*[rnd.getrandbits(n) for _ in range(nproofs * m)])
    blindings = b"".join(rnd.randrange(L_ORDER).to_bytes(32, "little") for _ in range(nproofs * m))
    t_rows = [[rnd.randrange(L_ORDER) for _ in range(nproofs * m)] for _ in range(2)]
    for role in (0, 1, 2):
        got = _arrays(n, m, nproofs, t_rows)
        want = _arrays(n, m, nproofs, t_rows)
        legacy = _arrays(n, m, nproofs, t_rows)
        assert harness.rppseed_role(role, 1, n, m, nproofs, values, blindings, b"".join(seeds), *got) == 0
        assert harness.rppseed_role(role, 0, n, m, nproofs, values, blindings, buf, *want) == 0
        harness.rppseed_role_legacy(role, n, m, nproofs, values, blindings, buf, *legacy)
        for name, a, b, c in zip(("gen_scalars", "sL", "sR", "party"), got, want, legacy):
            assert bytes(a) == bytes(b) == bytes(c), (role, name)
        touched = [bytes(a) != bytes(f) for a, f in zip(got, _arrays(n, m, nproofs, t_rows))]
        assert touched == {0: [True, False, False, True], 1: [True, True, True, False], 2: [True, False, False, True]}[role]


def _state_of(t):
    """the 208-byte state of an oracle-twin transcript (include/bpgpu.h BPGPU_TRANSCRIPT_BYTES)"""
    s = t.strobe
    return bytes(s.st) + bytes([s.pos, s.pos_begin, s.cur_flags]) + bytes(5)


def _bound(length):
    import bp_twin
    t = bp_twin.Transcript(b"payment-protocol v3")
    t.append_message(b"session", bytes(i & 0xff for i in range(length)))
    return t


def _wrap_item(t, n, m):
    """which of the separator's three appended items crosses the rate boundary (0: none)"""
    t = t.clone()
    hit = 0
    for item, (label, msg) in enumerate(((b"dom-sep", b"rangeproof v1"), (b"n", n.to_bytes(8, "little")), (b"m", m.to_bytes(8, "little"))), 1):
        before = t.strobe.pos
        t.append_message(label, msg)
        if t.strobe.pos < before:
            assert hit == 0
            hit = item
    return hit


def _wrapping_transcripts(n, m):
    """a fresh transcript, then three bound ones found by search: the separator wraps the 166-byte rate inside its 1st, 2nd and 3rd item"""
    import bp_twin
    found = {}
    for length in range(400):
        t = _bound(length)
        found.setdefault(_wrap_item(t, n, m), t)
    assert sorted(found) == [0, 1, 2, 3]
    return [bp_twin.Transcript(b"fresh")] + [found[i] for i in (1, 2, 3)]


@pytest.mark.parametrize("stride", [TS_WORDS, 0], ids=["per-proof", "shared"])
@pytest.mark.parametrize("n,m", [(64, 1), (16, 2)])
def test_separator_applying_transcript_lane_equals_the_oracle_twin(harness, n, m, stride):
    """rpp_chal1_lane<true> from un-separated states -- fresh, and wrapping the rate at each item of the separator: the state it leaves, y
    and z equal the twin's rangeproof_domain_sep(n, m); V_j, A, S; challenge y, z.  Proof and commitment bytes are the rows handed in."""
    starts = _wrapping_transcripts(n, m)
    if stride == 0:
        starts = [starts[2]] * 3
    nb = len(starts)
    rnd = random.Random(n * m + stride)
    rows = [bytes(rnd.getrandbits(8) for _ in range(32)) for _ in range(nb * (2 + m))]          # 2p: A, 2p + 1: S, 2 nb + p m + j: V_j
    msm_out = (C.c_uint32 * (8 * len(rows))).from_buffer_copy(b"".join(rows))
    ts_in = (C.c_uint32 * (TS_WORDS * nb)).from_buffer_copy(b"".join(_state_of(t) for t in starts)) if stride else \
        (C.c_uint32 * TS_WORDS).from_buffer_copy(_state_of(starts[0]))
    proof_len = 32 * (9 + 2 * ((n * m).bit_length() - 1))
    ts, fields = _filled(TS_WORDS * nb), _filled(8 * RPP_FIXED * nb)
    proofs, coms = C.create_string_buffer(b"\x5a" * (proof_len * nb), proof_len * nb), C.create_string_buffer(b"\x5a" * (32 * m * nb), 32 * m * nb)
    harness.rppseed_chal1_sep(n, m, nb, msm_out, ts_in, stride, ts, fields, proofs, coms)
    for p, t0 in enumerate(starts):
        t = t0.clone()
        t.rangeproof_domain_sep(n, m)
        for j in range(m):
            t.append_message(b"V", rows[2 * nb + p * m + j])
        t.append_message(b"A", rows[2 * p])
        t.append_message(b"S", rows[2 * p + 1])
        y = int.from_bytes(t.challenge_bytes(b"y", 64), "little") % L_ORDER
        z = int.from_bytes(t.challenge_bytes(b"z", 64), "little") % L_ORDER
        assert bytes(ts)[4 * TS_WORDS * p:4 * TS_WORDS * (p + 1)] == _state_of(t), p
        f = bytes(fields)
        assert f[32 * p:32 * p + 32] == y.to_bytes(32, "little") and f[32 * (nb + p):32 * (nb + p) + 32] == z.to_bytes(32, "little")
        assert proofs.raw[proof_len * p:proof_len * p + 64] == rows[2 * p] + rows[2 * p + 1]
        assert proofs.raw[proof_len * p + 64:proof_len * (p + 1)] == b"\x5a" * (proof_len - 64)
        assert coms.raw[32 * m * p:32 * m * (p + 1)] == b"".join(rows[2 * nb + p * m + j] for j in range(m))
    assert bytes(fields)[64 * nb:] == FILL.to_bytes(4, "little") * (8 * (RPP_FIXED - 2) * nb)
