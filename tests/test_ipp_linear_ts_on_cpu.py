"""The inner-product / linear front ends on the callers' own transcripts without a GPU: the lanes that start from per-proof states and apply
innerproduct_domain_sep themselves (ipp_prepare_lane<true>, ipp_vs_front_lane<true>, lin_prepare_lane<true>, ipp_ts_fill_thread) and the
linear prover's public lane under either draw source (linc_public_lane), compiled for the host (tests/ipp_linear_ts_harness) and run lane
by lane -- the transcripts, challenges and emitted scalars against the oracle twin's Transcript, ipp_verify and linear_verify, the seed-fed
public lane against the buffer-fed one on the keystream ChaChaRng(seed) would hand out."""
import ctypes as C
import hashlib
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ELL = 2**252 + 27742317777372353535851937790883648493
FILL = 0x5a5a5a5a
TS_WORDS, TS = 52, 208
OK, VERIFICATION, FORMAT = 0, 1, 2
u32p = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("iplts") / "libiplts.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "ipp_linear_ts_harness", "harness.cpp")])
    lib = C.CDLL(so)
    u8p, u32, i = C.c_char_p, C.c_uint32, C.c_int
    lib.iplts_ipp_prepare.argtypes = [u32, u32, u8p, u32, u8p, u8p, u8p, u8p, u8p, u8p, u32, u32p, u32, i, u32p, u32p, u32p, u32p]
    lib.iplts_ipp_vs_front.argtypes = [u32, u32, u8p, u32, u32p, u32, i, u32p, u32p, u32p, u32p, u32p]
    lib.iplts_ts_fill.argtypes = [u32, u32, u32p, u32, u32p]
    lib.iplts_ts_fill.restype = None
    lib.iplts_lin_prepare.argtypes = [u32, u32, u8p, u32, u8p, u8p, u32, u8p, u8p, u8p, u32p, u32, i, u32p, u32p, u32p, u32p, u32p]
    lib.iplts_linc_public.argtypes = [i, i, i, u32, u32, u8p, u8p, u32, u8p, u8p, u8p, u8p, u8p, u32p, u32, u32p, u32p, u32p, u32p]
    return lib


# ---- transcripts ------------------------------------------------------------------------------------------------------------------------
def _state_of(t):
    """the 208-byte state of an oracle-twin transcript (include/bpgpu.h BPGPU_TRANSCRIPT_BYTES)"""
    s = t.strobe
    return bytes(s.st) + bytes([s.pos, s.pos_begin, s.cur_flags]) + bytes(5)


def _bound(length):
    import bp_twin
    t = bp_twin.Transcript(b"payment-protocol v3")
    t.append_message(b"session", bytes(i & 0xff for i in range(length)))
    return t


def _wrap_item(t, n):
    """which of innerproduct_domain_sep(n)'s two appended items crosses the 166-byte rate boundary (0: none)"""
    t = t.clone()
    hit = 0
    for item, (label, msg) in enumerate(((b"dom-sep", b"ipp v1"), (b"n", n.to_bytes(8, "little"))), 1):
        before = t.strobe.pos
        t.append_message(label, msg)
        if t.strobe.pos < before:
            assert hit == 0
            hit = item
    return hit


def _starts(n):
    """a fresh transcript, then two bound ones found by search: the separator wraps the rate inside its 1st (`dom-sep`) and its 2nd (`n`) item"""
    import bp_twin
    found = {}
    for length in range(400):
        t = _bound(length)
        found.setdefault(_wrap_item(t, n), t)
    assert sorted(found) == [0, 1, 2]
    return [bp_twin.Transcript(b"fresh"), found[1], found[2]]


def _words(b):
    return (C.c_uint32 * (len(b) // 4)).from_buffer_copy(b)


def _filled(nwords):
    return (C.c_uint32 * max(nwords, 1))(*([FILL] * max(nwords, 1)))


def _zeros(nwords):
    return (C.c_uint32 * max(nwords, 1))()


def _le(x):
    return (x % ELL).to_bytes(32, "little")


# how the lanes get their start states: (name, ts_in_stride in words, by_value)
MODES = [("per-proof", TS_WORDS, 0), ("stride-0", 0, 0), ("by-value", 0, 1)]


def _mode_starts(starts, mode):
    """stride 0 and by-value runs give every proof ONE state: the one whose separator wraps inside `n`"""
    return starts if mode[1] else [starts[2]] * len(starts)


def _ts_in(starts, mode):
    return _words(b"".join(_state_of(t) for t in starts) if mode[1] else _state_of(starts[0]))


# ---- inner-product proofs ----------------------------------------------------------------------------------------------------------------
def _ipp_rows(oracle, n, nb, tag):
    """nb valid proofs (the oracle's test instances re-made on the row's own transcript by the twin), then one of each rejection class of the
    reference: non-canonical b (from_bytes), identity R_1 resp. L_0 (validate_and_append_point); the wrong-n class is a call of its own"""
    return [oracle.ipp_test_instance(n, b"unused", b"%s-%d-%d" % (tag, n, j)) for j in range(nb)]


def _twin_ipp_proof(inst, n, t0):
    """InnerProductProof::create on transcript t0 for the instance's witness: the proof bytes (twin) and P"""
    import bp_twin as T
    rnd = random.Random(inst["Q"])
    a = [rnd.randrange(ELL) for _ in range(n)]
    b = [rnd.randrange(ELL) for _ in range(n)]
    Gf = [int.from_bytes(inst["Gf"][32 * i:32 * i + 32], "little") for i in range(n)]
    Hf = [int.from_bytes(inst["Hf"][32 * i:32 * i + 32], "little") for i in range(n)]
    G = [T.decompress(inst["G"][32 * i:32 * i + 32]) for i in range(n)]
    H = [T.decompress(inst["H"][32 * i:32 * i + 32]) for i in range(n)]
    Q = T.decompress(inst["Q"])
    Lv, Rv, a0, b0 = T.ipp_create(t0.clone(), Q, Gf, Hf, G, H, a, b)
    c = sum(x * y for x, y in zip(a, b)) % ELL
    P = T.compress(T.msm([x * g % ELL for x, g in zip(a, Gf)] + [y * h % ELL for y, h in zip(b, Hf)] + [c], G + H + [Q]))
    return b"".join(l + r for l, r in zip(Lv, Rv)) + _le(a0) + _le(b0), P


def _twin_ipp_expect(proof, n, t0, inst, P):
    """(status, the scalars of the 2n + 2k + 2 terms or None, the transcript as the reference leaves it, compress(expect_P - P) or None)"""
    import bp_twin as T
    t = t0.clone()
    k = (len(proof) // 32 - 2) // 2
    pr = T.RangeProof()
    pr.L_vec = [proof[64 * i:64 * i + 32] for i in range(k)]
    pr.R_vec = [proof[64 * i + 32:64 * i + 64] for i in range(k)]
    try:
        pr.a, pr.b = T._canonical_scalar(proof[64 * k:64 * k + 32]), T._canonical_scalar(proof[64 * k + 32:])
    except T.FormatError:
        return FORMAT, None, t, None
    try:
        u_sq, u_inv_sq, s = T.verification_scalars(pr, n, t)
    except T.VerificationError:
        return VERIFICATION, None, t, None
    Gf = [int.from_bytes(inst["Gf"][32 * i:32 * i + 32], "little") for i in range(n)]
    Hf = [int.from_bytes(inst["Hf"][32 * i:32 * i + 32], "little") for i in range(n)]
    sc = [pr.a * pr.b] + [pr.a * s[i] * Gf[i] for i in range(n)] + [pr.b * s[n - 1 - i] * Hf[i] for i in range(n)] + \
         [-u for u in u_sq] + [-u for u in u_inv_sq] + [-1]
    dec = lambda b: [T.decompress(b[32 * i:32 * i + 32]) for i in range(len(b) // 32)]
    em = T.ipp_verify(proof, n, t0.clone(), Gf, Hf, T.decompress(P), T.decompress(inst["Q"]), dec(inst["G"]), dec(inst["H"]))
    return OK, [_le(x) for x in sc], t, em


@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("n", [2, 64])
def test_inner_product_front_lanes_from_per_proof_states_equal_the_twin(harness, oracle, n, mode):
    """ipp_prepare_lane<true> and ipp_vs_front_lane<true> (the per-proof and the combined call's front end): status, the scalars of every
    term, u^2 / u^-2 and ts_out == the twin's, for valid proofs made on each start state and for the rejection classes of C4"""
    starts = _mode_starts(_starts(n), mode)
    k = n.bit_length() - 1
    insts = _ipp_rows(oracle, n, 6, b"cpu-ipp-ts")
    rows_t = [starts[j % 3] for j in range(6)]
    made = [_twin_ipp_proof(i, n, t) for i, t in zip(insts, rows_t)]
    proofs, Ps = [m[0] for m in made], [m[1] for m in made]
    bad = bytearray(proofs[3])
    bad[-32:] = b"\xff" * 32                                   # from_bytes: non-canonical b
    proofs[3] = bytes(bad)
    bad = bytearray(proofs[4])
    bad[64 * (k - 1) + 32:64 * k] = bytes(32)                  # identity R in the last round: every earlier round is absorbed
    proofs[4] = bytes(bad)
    bad = bytearray(proofs[5])
    bad[0:32] = bytes(32)                                      # identity L_0: only the separator is absorbed
    proofs[5] = bytes(bad)
    nb, pl = 6, len(proofs[0])
    G, H = insts[0]["G"], insts[0]["H"]
    assert all(i["G"] == G and i["H"] == H for i in insts)
    cat = lambda key: b"".join(i[key] for i in insts)
    want = [_twin_ipp_expect(proofs[j], n, rows_t[j], insts[j], Ps[j]) for j in range(nb)]
    assert [w[0] for w in want] == [OK, OK, OK, FORMAT, VERIFICATION, VERIFICATION]
    assert all(w[3] == bytes(32) for w in want[:3])
    ts_in = _ts_in(rows_t, mode)
    N = 2 * n + 2 * k + 2
    sc, pt, status, ts_out = _zeros(8 * N * nb), _zeros(8 * N * nb), _zeros(nb), _filled(TS_WORDS * nb)
    assert harness.iplts_ipp_prepare(n, nb, b"".join(proofs), pl, cat("Gf"), cat("Hf"), b"".join(Ps), cat("Q"), G, H, 1, ts_in, mode[1], mode[2],
                                     sc, pt, status, ts_out) == N
    usq, uisq, tab, status2, ts_out2 = _zeros(8 * k * nb), _zeros(8 * k * nb), _filled(20 * k * nb), _zeros(nb), _filled(TS_WORDS * nb)
    assert harness.iplts_ipp_vs_front(n, nb, b"".join(proofs), pl, ts_in, mode[1], mode[2], usq, uisq, tab, status2, ts_out2) == k
    assert list(status) == list(status2) == [w[0] for w in want]
    assert bytes(ts_out) == bytes(ts_out2) == b"".join(_state_of(w[2]) for w in want)
    # what the reference leaves behind for the rejected rows (C4): the input state, and the state as of the identity point
    assert _state_of(want[3][2]) == _state_of(rows_t[3])
    for j, rounds in ((4, k - 1), (5, 0)):
        t = rows_t[j].clone()
        t.innerproduct_domain_sep(n)
        for r in range(rounds):
            t.append_message(b"L", proofs[j][64 * r:64 * r + 32])
            t.append_message(b"R", proofs[j][64 * r + 32:64 * r + 64])
            t.challenge_bytes(b"u", 64)
        if j == 4:
            t.append_message(b"L", proofs[j][64 * (k - 1):64 * (k - 1) + 32])
        assert _state_of(t) == _state_of(want[j][2])
    for j in range(3):
        assert bytes(sc)[32 * N * j:32 * N * (j + 1)] == b"".join(want[j][1]), j
        pts = insts[j]["Q"] + G + H + b"".join(proofs[j][64 * r:64 * r + 32] for r in range(k)) + \
            b"".join(proofs[j][64 * r + 32:64 * r + 64] for r in range(k)) + Ps[j]
        assert bytes(pt)[32 * N * j:32 * N * (j + 1)] == pts, j
        neg = lambda b: _le(-int.from_bytes(b, "little"))
        assert [neg(x) for x in want[j][1][1 + 2 * n:1 + 2 * n + k]] == [bytes(usq)[32 * (k * j + r):32 * (k * j + r) + 32] for r in range(k)]
        assert [neg(x) for x in want[j][1][1 + 2 * n + k:1 + 2 * n + 2 * k]] == [bytes(uisq)[32 * (k * j + r):32 * (k * j + r) + 32] for r in range(k)]
    # a FormatError row writes no term at all
    assert bytes(sc)[32 * N * 3:32 * N * 4] == bytes(32 * N)
    # n != 2^lg_n: the reference returns before the separator, every row gets its input state back
    status, ts_out = _zeros(nb), _filled(TS_WORDS * nb)
    sc, pt = _zeros(16 * nb), _zeros(16 * nb)
    assert harness.iplts_ipp_prepare(2 * n, nb, b"".join(proofs), pl, cat("Gf") * 2, cat("Hf") * 2, b"".join(Ps), cat("Q"), G * 2, H * 2, 1, ts_in, mode[1],
                                     mode[2], sc, pt, status, ts_out) == 2
    assert list(status) == [VERIFICATION] * 3 + [FORMAT] + [VERIFICATION] * 2
    assert bytes(ts_out) == b"".join(_state_of(t) for t in rows_t)
    status2, ts_out2 = _zeros(nb), _filled(TS_WORDS * nb)
    assert harness.iplts_ipp_vs_front(2 * n, nb, b"".join(proofs), pl, ts_in, mode[1], mode[2], usq, uisq, tab, status2, ts_out2) == k
    assert list(status2) == list(status) and bytes(ts_out2) == bytes(ts_out)


@pytest.mark.parametrize("mode", MODES[:2], ids=[m[0] for m in MODES[:2]])
@pytest.mark.parametrize("n", [2, 64])
def test_state_fill_of_the_inner_product_prover_is_the_separator(harness, n, mode):
    starts = _mode_starts(_starts(n), mode)
    ts = _filled(TS_WORDS * 3)
    harness.iplts_ts_fill(n, 3, _ts_in(starts, mode), mode[1], ts)
    want = []
    for t in starts:
        t = t.clone()
        t.innerproduct_domain_sep(n)
        want.append(_state_of(t))
    assert bytes(ts) == b"".join(want)


def test_a_state_with_position_bytes_out_of_range_starts_at_position_0(harness):
    """device states cannot be checked by the host: position 200 (past the 166-byte rate) is started at 0, as rpp_chal1_lane<true> does"""
    import bp_twin
    t = bp_twin.Transcript(b"fresh")
    st = bytearray(_state_of(t))
    st[200], st[201] = 200, 3
    ts = _filled(TS_WORDS)
    harness.iplts_ts_fill(8, 1, _words(bytes(st)), 0, ts)
    t.strobe.pos = t.strobe.pos_begin = 0
    t.innerproduct_domain_sep(8)
    assert bytes(ts) == _state_of(t)


# ---- linear proofs -----------------------------------------------------------------------------------------------------------------------
def _linear_rows(oracle, n, starts, nb):
    """nb proofs over one (G, F, B), each made by the twin on its own start state; per-proof public vectors"""
    import bp_twin as T
    base = oracle.linear_test_instance(n, b"cpu-lin-ts-%d" % n)
    dec = lambda b: [T.decompress(b[32 * i:32 * i + 32]) for i in range(len(b) // 32)]
    G, F, B = dec(base["G"]), T.decompress(base["F"]), T.decompress(base["B"])
    rows = []
    for j in range(nb):
        rnd = random.Random(1000 * n + j)
        a = [rnd.randrange(ELL) for _ in range(n)]
        b = [rnd.randrange(ELL) for _ in range(n)]
        r = rnd.randrange(ELL)
        c = sum(x * y for x, y in zip(a, b)) % ELL
        Cb = T.compress(T.msm(a + [r, c], G + [B, F]))
        proof = T.linear_create(starts[j].clone(), T.ShakeRng(b"cpu-lin-ts-rng-%d-%d" % (n, j)), Cb, r, a, b, G, F, B)
        rows.append(dict(proof=proof, C=Cb, b=b, a=a, r=r))
    return base, (G, F, B), rows


def _twin_linear_expect(row, n, t0, base, pts):
    """(status, the n + 2k + 4 scalars in the lane's term order or None, ts_out as bpgpu_linear_verify_batch documents it, compress or None)"""
    import bp_twin as T
    G, F, B = pts
    proof, k = row["proof"], n.bit_length() - 1
    t = t0.clone()
    t.innerproduct_domain_sep(n)
    behind_sep = t.clone()
    a_b, r_b = proof[64 * k + 32:64 * k + 64], proof[64 * k + 64:]
    if int.from_bytes(a_b, "little") >= ELL or int.from_bytes(r_b, "little") >= ELL:
        return FORMAT, None, behind_sep, None
    a, r = int.from_bytes(a_b, "little"), int.from_bytes(r_b, "little")
    t.append_message(b"C", row["C"])
    for x in row["b"]:
        t.append_message(b"b_i", _le(x))
    for i in range(n):
        t.append_message(b"G_i", base["G"][32 * i:32 * i + 32])
    t.append_message(b"F", base["F"])
    t.append_message(b"B", base["B"])
    xs = []
    for j in range(k):
        Lb, Rb = proof[64 * j:64 * j + 32], proof[64 * j + 32:64 * j + 64]
        if Lb == bytes(32) or Rb == bytes(32):
            return VERIFICATION, None, behind_sep, None
        t.append_message(b"L", Lb)
        t.append_message(b"R", Rb)
        xs.append(t.challenge_scalar(b"x_j"))
    t.append_message(b"S", proof[64 * k:64 * k + 32])
    x_star = t.challenge_scalar(b"x_star")
    s = [1]
    for i in range(1, n):
        lg_i = i.bit_length() - 1
        s.append(s[i - (1 << lg_i)] * xs[(k - 1) - lg_i] % ELL)
    b0 = sum(si * bi for si, bi in zip(s, row["b"])) % ELL
    sc = [r, a * b0, -x_star] + [-x_star * x for x in xs] + [-x_star * T.sc_inv(x) for x in xs] + [a * si for si in s] + [-1]
    em = T.linear_verify(proof, t0.clone(), row["C"], G, F, B, row["b"])
    return OK, [_le(x) for x in sc], t, em


@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("n", [2, 64])
def test_linear_front_lane_from_per_proof_states_equals_the_twin(harness, oracle, n, mode):
    """lin_prepare_lane<true>: status, every term's scalar and point and ts_out == the twin's, for valid proofs made on each start state, a
    non-canonical a, an identity L_0 and n != 2^lg_n -- rejected rows get their own state behind the separator (bpgpu_linear_verify_batch's
    documented start state, per proof)"""
    starts = _mode_starts(_starts(n), mode)
    k, nb = n.bit_length() - 1, 5
    rows_t = [starts[j % 3] for j in range(nb)]
    base, pts, rows = _linear_rows(oracle, n, rows_t, nb)
    bad = bytearray(rows[3]["proof"])
    bad[64 * k + 32:64 * k + 64] = b"\xff" * 32                # non-canonical a
    rows[3]["proof"] = bytes(bad)
    bad = bytearray(rows[4]["proof"])
    bad[0:32] = bytes(32)                                      # identity L_0
    rows[4]["proof"] = bytes(bad)
    pl = len(rows[0]["proof"])
    want = [_twin_linear_expect(rows[j], n, rows_t[j], base, pts) for j in range(nb)]
    assert [w[0] for w in want] == [OK, OK, OK, FORMAT, VERIFICATION] and all(w[3] == bytes(32) for w in want[:3])
    proofs, Cs = b"".join(r["proof"] for r in rows), b"".join(r["C"] for r in rows)
    bs = b"".join(_le(x) for r in rows for x in r["b"])
    ts_in = _ts_in(rows_t, mode)
    N = n + 2 * k + 4
    sc, pt, status, ts_out = _zeros(8 * N * nb), _zeros(8 * N * nb), _zeros(nb), _filled(TS_WORDS * nb)
    assert harness.iplts_lin_prepare(n, nb, proofs, pl, Cs, bs, 0, base["G"], base["F"], base["B"], ts_in, mode[1], mode[2], sc, pt, status, ts_out, None) == N
    assert list(status) == [w[0] for w in want]
    assert bytes(ts_out) == b"".join(_state_of(w[2]) for w in want)
    for j in range(3):
        pr = rows[j]["proof"]
        assert bytes(sc)[32 * N * j:32 * N * (j + 1)] == b"".join(want[j][1]), j
        points = base["B"] + base["F"] + rows[j]["C"] + b"".join(pr[64 * r:64 * r + 32] for r in range(k)) + \
            b"".join(pr[64 * r + 32:64 * r + 64] for r in range(k)) + base["G"] + pr[64 * k:64 * k + 32]
        assert bytes(pt)[32 * N * j:32 * N * (j + 1)] == points, j
    # generator-table mode: the coefficients of (B, F, G_0..) in a row of their own, the same scalars
    M = 2 * k + 2
    sc2, pt2, status2, ts_out2, gen = _zeros(8 * M * nb), _zeros(8 * M * nb), _zeros(nb), _filled(TS_WORDS * nb), _zeros(8 * (n + 2) * nb)
    assert harness.iplts_lin_prepare(n, nb, proofs, pl, Cs, bs, 0, base["G"], base["F"], base["B"], ts_in, mode[1], mode[2], sc2, pt2, status2, ts_out2, gen) == M
    assert list(status2) == list(status) and bytes(ts_out2) == bytes(ts_out)
    for j in range(3):
        w = want[j][1]
        assert bytes(gen)[32 * (n + 2) * j:32 * (n + 2) * (j + 1)] == w[0] + w[1] + b"".join(w[3 + 2 * k:3 + 2 * k + n])
        assert bytes(sc2)[32 * M * j:32 * M * (j + 1)] == b"".join(w[2:3 + 2 * k]) + w[-1]
    # n != 2^lg_n: VerificationError for the rows from_bytes accepts, each with its own state behind the separator of the CALLER's n
    status, ts_out = _zeros(nb), _filled(TS_WORDS * nb)
    sc, pt = _zeros(32 * nb), _zeros(32 * nb)
    assert harness.iplts_lin_prepare(2 * n, nb, proofs, pl, Cs, bs * 2, 0, base["G"] * 2, base["F"], base["B"], ts_in, mode[1], mode[2], sc, pt, status, ts_out,
                                     None) == 4
    assert list(status) == [VERIFICATION] * 3 + [FORMAT, VERIFICATION]
    behind = []
    for t in rows_t:
        t = t.clone()
        t.innerproduct_domain_sep(2 * n)
        behind.append(_state_of(t))
    assert bytes(ts_out) == b"".join(behind)


# ---- the linear prover's public lane -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nproofs", [1, 3])
@pytest.mark.parametrize("n", [2, 64])
def test_seed_fed_public_lane_equals_the_buffer_fed_lane_on_the_expanded_keystream(harness, oracle, n, nproofs):
    """linc_public_lane fed rpp_draw(seed_of_p, d) and fed the byte buffer ChaChaRng(seed).fill_bytes(64 (2k + 2)): the `draws`, r and status
    arrays compared whole, word for word (untouched words keep the pattern in both); no lane asks for a draw at or past 2k + 2; the existing
    kernel's wrapper (linc_public_thread) leaves the same arrays again; draw d is the d-th Scalar::random of the seed's ChaChaRng; and the
    separator-applying start leaves the transcript the twin leaves"""
    from chacha_rng import ChaChaRng, scalar_random
    k = n.bit_length() - 1
    D = 2 * k + 2
    starts = _starts(n)[:nproofs]
    base = oracle.linear_test_instance(n, b"cpu-linc-%d" % n)
    rnd = random.Random(n * 10 + nproofs)
    seeds = [hashlib.shake_256(b"linc-%d-%d-%d" % (n, nproofs, p)).digest(32) for p in range(nproofs)]
    buf = b"".join(ChaChaRng(s).fill_bytes(64 * D) for s in seeds)
    assert len(buf) == 64 * D * nproofs
    Cs = b"".join(hashlib.shake_256(b"linc-C-%d-%d" % (n, p)).digest(32) for p in range(nproofs))
    bs = b"".join(_le(rnd.randrange(ELL)) for _ in range(nproofs * n))
    rs = b"".join(_le(rnd.randrange(ELL)) for _ in range(nproofs))
    separated = []
    for t in starts:
        t = t.clone()
        t.innerproduct_domain_sep(n)
        separated.append(_state_of(t))

    def run(seeded, sep, legacy, stride=TS_WORDS):
        ts = _filled(TS_WORDS * nproofs) if sep else _words(b"".join(separated))
        ts_in = _words(b"".join(_state_of(t) for t in starts))
        r_out, draws, status = _filled(8 * nproofs), _filled(8 * D * nproofs + 8), _zeros(nproofs)
        bad = harness.iplts_linc_public(seeded, sep, legacy, n, nproofs, Cs, bs, 0, base["G"], base["F"], base["B"], rs, b"".join(seeds) if seeded else buf,
                                        ts_in if sep else None, stride, ts, r_out, draws, status)
        assert bad == 0
        return bytes(ts), bytes(r_out), bytes(draws), bytes(status)
    want = run(0, 0, 0)
    assert run(1, 1, 0) == want and run(1, 0, 0) == want and run(0, 1, 0) == want and run(0, 0, 1) == want
    ts, r_out, draws, status = want
    assert r_out == rs and status == bytes(4 * nproofs)
    assert draws[32 * D * nproofs:] == FILL.to_bytes(4, "little") * 8                      # nothing past the last draw
    for p, seed in enumerate(seeds):
        rng = ChaChaRng(seed)
        assert [draws[32 * (D * p + d):32 * (D * p + d) + 32] for d in range(D)] == [scalar_random(rng) for _ in range(D)]
        t = starts[p].clone()
        t.innerproduct_domain_sep(n)
        t.append_message(b"C", Cs[32 * p:32 * p + 32])
        for i in range(n):
            t.append_message(b"b_i", bs[32 * (n * p + i):32 * (n * p + i) + 32])
        for i in range(n):
            t.append_message(b"G_i", base["G"][32 * i:32 * i + 32])
        t.append_message(b"F", base["F"])
        t.append_message(b"B", base["B"])
        assert ts[TS * p:TS * (p + 1)] == _state_of(t), p
    # stride 0: every proof from the first state
    ts0 = run(1, 1, 0, stride=0)[0]
    assert ts0[:TS] == ts[:TS] and (nproofs == 1 or ts0[TS:2 * TS] != ts[TS:2 * TS])
