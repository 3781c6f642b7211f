"""The batched Pedersen commitments without a GPU: pedersen.h's lane bodies compiled for the host (tests/pedersen_harness) and run lane by
lane over a two-generator window table that the host-compiled table builders make from the oracle's B and B_blinding -- the variable-time
body at W = 7, 8, 13 and the constant-time body at W = 4, against oracle.msm([v, r], [B, B_blinding]) row by row.  The table lists
[B, B_blinding] and the id list is (1, 0): the ids place the bases, not their position.  The same harness also runs as a stand-alone
program under AddressSanitizer and UBSan with every buffer at its exact size."""
import ctypes as C
import os
import subprocess

import pytest

import pedersen_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "pedersen_harness", "harness.cpp")
FORMS = [(4, 1), (7, 0), (8, 0), (13, 0)]       # (W, constant-time body)
SEED24 = bytes([24]) * 32


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pedersen") / "libpedersen.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.ped_table_entries.restype = C.c_uint64
    lib.ped_table_entries.argtypes = [C.c_uint32, C.c_uint32]
    lib.ped_build_table.argtypes = [C.c_uint32, C.c_uint32, C.c_char_p, C.c_void_p]
    lib.ped_commit_rows.restype = None
    lib.ped_commit_rows.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint32), C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ped_open_rows.restype = None
    lib.ped_open_rows.argtypes = [C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p]
    lib.ped_encode_against_compress.argtypes = [C.c_char_p, C.c_uint32]
    return lib


@pytest.fixture(scope="module")
def bases(oracle):
    _, _, B, Bb = oracle.Gens(8, 1).export()
    return B, Bb


@pytest.fixture(scope="module")
def tables(harness, bases):
    """W -> the window table of [B, B_blinding], built once per module by fb_base_thread / fb_fill_thread / fb_norm_thread"""
    B, Bb = bases
    out = {}
    for W, _ in FORMS:
        buf = C.create_string_buffer(harness.ped_table_entries(W, 2) * harness.ped_table_entry_bytes())
        assert harness.ped_build_table(W, 2, B + Bb, buf) == 0
        out[W] = buf
    return out


IDS = (C.c_uint32 * 2)(1, 0)     # B_blinding is row 1 of the table, B row 0


def _commit(harness, tables, W, ct, values, value_bytes, blindings=None, seed=None, first_draw=0, want_blindings=False):
    """values: ints; blindings: ints or None.  Returns (commitments, status[, blindings]) as lists of 32-byte strings / a bytes object"""
    nb = len(values)
    packed = b"".join(v.to_bytes(value_bytes, "little") for v in values)
    bl = None if blindings is None else b"".join(pc.le32(b) for b in blindings)
    out = C.create_string_buffer(b"\x5a" * (32 * nb + 1), 32 * nb + 1)      # one guard byte behind the last row
    st = C.create_string_buffer(b"\x5a" * (nb + 1), nb + 1)
    blo = C.create_string_buffer(32 * nb) if want_blindings else None
    harness.ped_commit_rows(ct, W, nb, packed, value_bytes // 4, bl, seed, first_draw, IDS, tables[W], out, blo, st)
    assert out.raw[32 * nb:] == b"\x5a" and st.raw[nb:] == b"\x5a"
    res = ([out.raw[32 * i:32 * i + 32] for i in range(nb)], st.raw[:nb])
    return res + ([blo.raw[32 * i:32 * i + 32] for i in range(nb)],) if want_blindings else res


def _open(harness, tables, W, commitments, values, value_bytes, blindings):
    nb = len(values)
    vd = C.create_string_buffer(b"\x5a" * (nb + 1), nb + 1)
    harness.ped_open_rows(W, nb, b"".join(v.to_bytes(value_bytes, "little") for v in values), value_bytes // 4, b"".join(pc.le32(b) for b in blindings),
                          b"".join(commitments), IDS, tables[W], vd)
    assert vd.raw[nb:] == b"\x5a"
    return vd.raw[:nb]


@pytest.fixture(scope="module")
def expected(oracle, bases):
    """the oracle's commitment to every row of the matrix, computed once"""
    memo = {}

    def get(v, r):
        if (v, r) not in memo:
            memo[(v, r)] = pc.expect(oracle, bases[0], bases[1], v, r)
        return memo[(v, r)]
    return get


def test_a_u64_value_takes_only_the_windows_it_can_reach(harness):
    """ceil(66 / W) windows, never more than the scalar's: 9 instead of 32 at W = 8; v + bias stays below 2^(W nw) for every u64 v"""
    harness.ped_windows_u64.restype = C.c_uint32
    assert [harness.ped_windows_u64(W) for W in (4, 7, 8, 13, 20)] == [17, 10, 9, 6, 4]
    for W in range(2, 21):
        nw = harness.ped_windows_u64(W)
        bias = sum(2**(W - 1) << (W * k) for k in range(nw))
        assert 2**64 - 1 + bias < 2**(W * nw) and nw <= -(-255 // W)


@pytest.mark.parametrize("W,ct", FORMS)
def test_rows_equal_the_oracles_two_term_msm(harness, tables, expected, W, ct):
    """every (value, blinding) of the matrix as a u64 and as a 32-byte scalar: the oracle's bytes, status OK, the same bytes both ways;
    (0, 0) gives 32 zero bytes"""
    rows = pc.rows()
    vals, bls = [v for v, _ in rows], [r for _, r in rows]
    want = [expected(v, r) for v, r in rows]
    got8, st8 = _commit(harness, tables, W, ct, vals, 8, bls)
    got32, st32 = _commit(harness, tables, W, ct, vals, 32, bls)
    assert st8 == st32 == bytes(len(rows))
    for i, (v, r) in enumerate(rows):
        assert got8[i] == want[i], (hex(v), hex(r))
        assert got32[i] == want[i], (hex(v), hex(r))
    assert got8[0] == bytes(32)


@pytest.mark.parametrize("W,ct", FORMS)
def test_scalar_values_and_rejected_scalars(harness, tables, expected, W, ct):
    """32-byte values beyond a u64 (2^64, 2^252, l - 1); l and 2^256 - 1 as a value, l as a blinding: status BAD_SCALAR and 32 zero
    bytes, the rows beside them unaffected"""
    bls = pc.blindings()
    vals = pc.SCALAR_ONLY_VALUES + pc.REJECTED_SCALARS + [5, 7, pc.L_ORDER - 1]
    rs = [bls[3], bls[2], bls[2], bls[4], bls[5], pc.L_ORDER, 1, 0]
    got, st = _commit(harness, tables, W, ct, vals, 32, rs)
    for i, (v, r) in enumerate(zip(vals, rs)):
        if v >= pc.L_ORDER or r >= pc.L_ORDER:
            assert st[i] == pc.BAD_SCALAR and got[i] == bytes(32)
        else:
            assert st[i] == pc.OK and got[i] == expected(v, r)
    got, st = _commit(harness, tables, W, ct, [3, 4, 5], 8, [1, pc.L_ORDER, 2])
    assert st == bytes([pc.OK, pc.BAD_SCALAR, pc.OK]) and got[1] == bytes(32)
    assert got[0] == expected(3, 1) and got[2] == expected(5, 2)


@pytest.mark.parametrize("W,ct", FORMS)
def test_seeded_rows_are_the_references_golden_commitments(harness, tables, golden, W, ct):
    """seed [24] * 32, values 0 .. 7: the eight vc[j] the reference commits in tests/range_proof.rs:103-113, and its r_j"""
    from chacha_rng import golden_blindings
    got, st, bl = _commit(harness, tables, W, ct, list(range(8)), 8, seed=SEED24, want_blindings=True)
    assert st == bytes(8)
    assert b"".join(got) == golden["vc_bytes"]
    assert bl == golden_blindings()
    # first_draw = 3 with 5 rows == rows 3 .. 7 of the full call
    part, st, blp = _commit(harness, tables, W, ct, list(range(3, 8)), 8, seed=SEED24, first_draw=3, want_blindings=True)
    assert part == got[3:] and blp == bl[3:] and st == bytes(5)


@pytest.mark.parametrize("W,ct", [(4, 1), (8, 0)])
def test_draw_index_crosses_the_32_bit_counter_boundary(harness, tables, expected, W, ct):
    """first_draw = 2^32 - 2 with 4 rows: blinding i == chacha20_block(seed, 2^32 - 2 + i) reduced mod l -- a 64-bit block counter"""
    from chacha_rng import chacha20_block
    first = 2**32 - 2
    got, st, bl = _commit(harness, tables, W, ct, [9, 8, 7, 6], 8, seed=SEED24, first_draw=first, want_blindings=True)
    want_bl = [int.from_bytes(chacha20_block(SEED24, first + i), "little") % pc.L_ORDER for i in range(4)]
    assert [int.from_bytes(b, "little") for b in bl] == want_bl and st == bytes(4)
    assert got == [expected(v, r) for v, r in zip([9, 8, 7, 6], want_bl)]
    assert len(set(want_bl)) == 4 and want_bl[2] != int.from_bytes(chacha20_block(SEED24, 0), "little") % pc.L_ORDER   # (no wrap to block 0)


@pytest.mark.parametrize("W", [7, 13])
def test_open_body(harness, tables, expected, W):
    """accepts every commitment of the matrix; rejects each with one bit flipped in the commitment, in the value and in the blinding;
    VerificationError for an encoding that does not decode, FormatError for a non-canonical scalar"""
    rows = pc.rows()
    vals, bls = [v for v, _ in rows], [r for _, r in rows]
    coms = [expected(v, r) for v, r in rows]
    assert _open(harness, tables, W, coms, vals, 8, bls) == bytes(len(rows))
    assert _open(harness, tables, W, coms, vals, 32, bls) == bytes(len(rows))
    n = len(rows)
    assert _open(harness, tables, W, [pc.flip_bit(c, (37 * i) % 256) for i, c in enumerate(coms)], vals, 8, bls) == bytes([pc.VERIFICATION_ERROR]) * n
    assert _open(harness, tables, W, coms, [v ^ (1 << ((11 * i) % 64)) for i, v in enumerate(vals)], 8, bls) == bytes([pc.VERIFICATION_ERROR]) * n
    flipped = [r ^ (1 << ((13 * i) % 252)) for i, r in enumerate(bls)]
    flipped = [f if f < pc.L_ORDER else r & (r - 1) for f, r in zip(flipped, bls)]      # (still one bit, still canonical: the lowest set bit cleared)
    assert _open(harness, tables, W, coms, vals, 8, flipped) == bytes([pc.VERIFICATION_ERROR]) * n
    # a mixed batch: opens, does not, no valid encoding (a non-canonical field element; the odd, "negative" one), non-canonical scalars
    bad_encodings = [b"\xff" * 32, (1).to_bytes(32, "little")]
    mixed_c = [coms[5], coms[6], bad_encodings[0], bad_encodings[1], coms[9], coms[10], bytes(32)]
    mixed_v = [vals[5], vals[6] + 1, vals[7], vals[8], pc.L_ORDER, vals[10], 0]
    mixed_r = [bls[5], bls[6], bls[7], bls[8], bls[9], pc.L_ORDER, 0]
    assert _open(harness, tables, W, mixed_c, mixed_v, 32, mixed_r) == bytes([pc.OPENS, pc.VERIFICATION_ERROR, pc.VERIFICATION_ERROR, pc.VERIFICATION_ERROR,
                                                                               pc.FORMAT_ERROR, pc.FORMAT_ERROR, pc.OPENS])


def test_the_in_lane_finish_is_ristretto_compress(harness, bases):
    """ped_encode (the point parked, its coordinates read again, one field element across the squaring chain) against ristretto_compress
    on k B, k = 0 .. 199"""
    assert harness.ped_encode_against_compress(bases[0], 200) == 0


def test_stand_alone_harness_is_clean_under_address_and_ub_sanitizers(tmp_path):
    """the harness as a program with its own main, -fsanitize=address,undefined, every buffer at its exact size"""
    exe = str(tmp_path / "pedersen_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DPED_HARNESS_MAIN", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pedersen harness ok" in out.stdout
