"""The signed sums of Pedersen commitments without a GPU: pedersen_sum.h's host plan and lane bodies compiled for the host
(tests/pedersen_sum_harness) and run the way the kernels run them -- a workgroup phase by phase, launch after launch -- over the
two-generator window table of tests/pedersen_harness: the variable-time finish at W = 7 and 13, the constant-time one at W = 4,
against oracle.msm over (+-1, C_i) ..., (v, B), (x, B_blinding) row by row.  The same harness also runs as a stand-alone program under
AddressSanitizer and UBSan with every buffer at its exact size."""
import ctypes as C
import os
import subprocess

import pytest

import pedersen_cases as pc
import pedersen_sum_cases as sc
import point_corpus as corpus

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "pedersen_sum_harness", "harness.cpp")
FORMS = [(4, 1), (7, 0), (13, 0)]       # (W, constant-time body)
IDS = (C.c_uint32 * 2)(1, 0)            # B_blinding is row 1 of the table, B row 0
KINDS = ("u64", "scalar", "none")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pedersen_sum") / "libpedersen_sum.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.ped_table_entries.restype = C.c_uint64
    lib.ped_table_entries.argtypes = [C.c_uint32, C.c_uint32]
    lib.ped_build_table.argtypes = [C.c_uint32, C.c_uint32, C.c_char_p, C.c_void_p]
    lib.ped_open_rows.restype = None
    lib.ped_open_rows.argtypes = [C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p]
    lib.psum_plan_table.restype = C.c_uint32
    lib.psum_plan_table.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p]
    lib.psum_run.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_char_p, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.c_void_p]
    lib.psum_decode_against_decompress.argtypes = [C.c_char_p, C.c_uint32]
    return lib


@pytest.fixture(scope="module")
def bases(oracle):
    _, _, B, Bb = oracle.Gens(8, 1).export()
    return B, Bb


@pytest.fixture(scope="module")
def tables(harness, bases):
    B, Bb = bases
    out = {}
    for W, _ in FORMS:
        buf = C.create_string_buffer(harness.ped_table_entries(W, 2) * harness.ped_table_entry_bytes())
        assert harness.ped_build_table(W, 2, B + Bb, buf) == 0
        out[W] = buf
    return out


def _run(harness, tables, W, ct, balance, off, pts, sg=None, values=None, value_bytes=8, blindings=None):
    """-> (encodings, status bytes, passes) or (verdict bytes, passes); values / blindings: ints or None"""
    nb = len(off) - 1
    offs = (C.c_uint32 * (nb + 1))(*off)
    vals = None if values is None else sc.pack(values, value_bytes)
    bl = None if blindings is None else b"".join(pc.le32(b) for b in blindings)
    scalars = values is not None or blindings is not None
    out = C.create_string_buffer(b"\x5a" * (32 * nb + 1), 32 * nb + 1)      # one guard byte behind the last row
    st = C.create_string_buffer(b"\x5a" * (nb + 1), nb + 1)
    passes = harness.psum_run(balance, ct, W, nb, offs, b"".join(pts), sg, vals, value_bytes // 4, bl, IDS if scalars else None, tables[W] if scalars else None,
                              None if balance else out, st)
    assert passes >= 1, "a partial's slot was out of range, stored twice or never stored"
    assert st.raw[nb:] == b"\x5a" and out.raw[32 * nb:] == b"\x5a"
    if balance:
        return st.raw[:nb], passes
    return [out.raw[32 * i:32 * i + 32] for i in range(nb)], st.raw[:nb], passes


@pytest.fixture(scope="module")
def batches(oracle, bases):
    """the shared inputs and the oracle's rows, computed once: name -> (offsets, points, values, blindings) and
    expected(name, sign mode, kind) -> encodings"""
    B, Bb = bases
    data, memo = {}, {}
    for name, lengths in (("rows", sc.ROWS), ("long", [3, sc.LONG_ROW, 2])):
        off = sc.offsets(lengths)
        vals, bls = sc.scalars(len(lengths))
        data[name] = (off, sc.points(off[-1], shift=len(lengths)), vals, bls)

    def expected(name, mode, kind):
        with_scalars = kind != "none"
        if (name, mode, with_scalars) not in memo:
            off, pts, vals, bls = data[name]
            memo[(name, mode, with_scalars)] = sc.expect_rows(oracle, B, Bb, off, pts, sc.signs(mode, off[-1]), vals if with_scalars else None,
                                                              bls if with_scalars else None)
        return memo[(name, mode, with_scalars)]
    return data, expected


def _scalars_of(kind, vals, bls):
    return {"u64": (vals, 8, bls), "scalar": (vals, 32, bls), "none": (None, 8, None)}[kind]


def test_the_cases_are_cut_for_the_headers_block_and_serial_bound(harness):
    assert (harness.psum_block(), harness.psum_serial_max()) == (sc.BLOCK, sc.SERIAL_MAX)
    edge, whole, most = sc.boundaries(sc.ROWS)
    off = sc.offsets(sc.ROWS)
    assert len(edge) >= 2 and any(off[r] % 64 == 63 and (off[r + 1] - 1) % 64 == 0 for r in edge)     # (last lane, first lane of the next)
    assert len(whole) >= 2 and any(sc.ROWS[r - 1] == 0 for r in whole)                                 # one workgroup exactly, also behind an empty row
    assert most >= 11 and sc.ROWS.count(0) >= 3
    assert -(-sc.LONG_ROW // sc.BLOCK) == sc.SERIAL_MAX + 1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W,ct", FORMS)
def test_every_row_equals_the_oracles_msm(harness, tables, batches, W, ct, kind):
    """the whole pattern, every sign mode: bit for bit the oracle's bytes; one pass"""
    data, expected = batches
    off, pts, vals, bls = data["rows"]
    v, vb, b = _scalars_of(kind, vals, bls)
    for mode in sc.SIGN_MODES:
        got, st, passes = _run(harness, tables, W, ct, 0, off, pts, sc.signs(mode, off[-1]), v, vb, b)
        assert passes == 1 and st == bytes(len(off) - 1)
        want = expected("rows", mode, kind)
        for r, (g, w) in enumerate(zip(got, want)):
            assert g == w, (mode, r, sc.ROWS[r])
    # zeros and None are the same call; an all-subtracted row is minus the all-added one: together they cancel
    assert expected("rows", "zeros", kind) == expected("rows", None, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W,ct", FORMS)
def test_a_row_past_the_serial_bound_takes_a_reduce_pass(harness, tables, batches, W, ct, kind):
    """8 193 terms are 129 partials, one more than a finish lane may add: two passes, the rows beside it unaffected"""
    data, expected = batches
    off, pts, vals, bls = data["long"]
    v, vb, b = _scalars_of(kind, vals, bls)
    got, st, passes = _run(harness, tables, W, ct, 0, off, pts, sc.signs("alternating", off[-1]), v, vb, b)
    assert passes == 2 and st == bytes(3)
    assert got == expected("long", "alternating", kind)


def _check_plan(harness, lengths):
    nb = len(lengths)
    off0 = sc.offsets(lengths)
    stride = nb + 1
    buf = (C.c_uint32 * ((harness.psum_max_passes() + 1) * stride))()
    npasses = harness.psum_plan_table(nb, (C.c_uint32 * stride)(*off0), buf)
    table = [list(buf[k * stride:(k + 1) * stride]) for k in range(npasses + 1)]
    assert table[0] == off0
    for k in range(npasses):
        off, nxt = table[k], table[k + 1]
        nblocks = -(-off[nb] // sc.BLOCK)
        slots = {}
        for r in range(nb):
            if off[r + 1] == off[r]:
                assert nxt[r + 1] == nxt[r]
                continue
            blocks = range(off[r] // sc.BLOCK, (off[r + 1] - 1) // sc.BLOCK + 1)
            mine = [nxt[r] + (b - off[r] // sc.BLOCK) for b in blocks]
            assert mine == list(range(nxt[r], nxt[r + 1]))                  # the row's slots are contiguous and fill its span
            for b, s in zip(blocks, mine):
                assert s not in slots
                slots[s] = (b, r)
        assert sorted(slots) == list(range(nxt[nb]))                        # every pair one slot, every slot one pair
        assert nxt[nb] <= nblocks + nb
        longest = max(nxt[r + 1] - nxt[r] for r in range(nb))
        assert (longest > sc.SERIAL_MAX) == (k + 1 < npasses)               # another pass exactly while a row is too long for one lane
    return npasses


def test_plan_properties(harness):
    assert _check_plan(harness, sc.ROWS) == 1
    assert _check_plan(harness, sc.ROWS + [sc.LONG_ROW]) == 2
    assert _check_plan(harness, [sc.LONG_ROW - 1]) == 1 and _check_plan(harness, [63, sc.LONG_ROW - 1]) == 2     # 128 whole workgroups / the same shifted: 129
    assert _check_plan(harness, [0, 0, 0]) == 1 and _check_plan(harness, [1]) == 1
    assert _check_plan(harness, [sc.SERIAL_MAX * sc.BLOCK * sc.BLOCK + 1]) == 3
    for seed in range(6):
        _check_plan(harness, sc.random_lengths(seed, 300, 40))
    for seed in range(3):
        _check_plan(harness, sc.random_lengths(100 + seed, 40, 30000))


def test_special_sums(harness, tables, oracle, bases):
    """P + P and P + P + P + P (the doubling case of the unified addition), -P, P - P, the identity encoding as a term"""
    P, Q = sc.pool()[:2]
    rows = [([P, P], b"\0\0"), ([P, P, P, P], b"\0\0\0\0"), ([P], b"\1"), ([P, P], b"\0\1"), ([bytes(32)], b"\0"), ([bytes(32), Q, bytes(32)], b"\1\0\1"),
            ([Q, P, Q, P], b"\0\1\1\0")]
    off = sc.offsets([len(p) for p, _ in rows])
    pts = [e for p, _ in rows for e in p]
    sg = b"".join(s for _, s in rows)
    want = sc.expect_rows(oracle, bases[0], bases[1], off, pts, sg)
    for W, ct in FORMS:
        got, st, _ = _run(harness, tables, W, ct, 0, off, pts, sg)
        assert got == want and st == bytes(len(rows))
        assert got[3] == bytes(32) and got[4] == bytes(32) and got[5] == Q and got[6] == bytes(32)
        vd, _ = _run(harness, tables, W, 0, 1, off, pts, sg)
        assert vd == bytes([1, 1, 1, 0, 0, 1, 0])                           # with no scalars a row balances when its sum is the identity


def test_the_parked_decoder_is_ristretto_decompress(harness):
    """psum_decode (one field element parked across the squaring chain) on every member of the corpus and on hashed points"""
    encs = corpus.ALL_ENC + sc.pool()[:40]
    assert harness.psum_decode_against_decompress(b"".join(encs), len(encs)) == 0


@pytest.mark.parametrize("W,ct", FORMS)
def test_each_rejection_class_alone_in_a_row(harness, tables, oracle, bases, W, ct):
    lengths, pts, flags = sc.reject_rows()
    off = sc.offsets(lengths)
    sg = sc.signs("alternating", off[-1])
    got, st, _ = _run(harness, tables, W, ct, 0, off, pts, sg)
    vd, _ = _run(harness, tables, W, 0, 1, off, pts, sg)
    assert len(flags) == 2 * len(corpus.REJECT_ENC) + 1
    for r, rejected in enumerate(flags):
        if rejected:
            assert (st[r], got[r], vd[r]) == (sc.BAD_POINT, bytes(32), sc.VERIFICATION_ERROR), corpus.REJECT[r // 2][0]
        else:
            s, e = sc.expect_row(oracle, bases[0], bases[1], pts[off[r]:off[r + 1]], sg[off[r]:off[r + 1]])
            assert s == 0 and (st[r], got[r]) == (sc.OK, e), r
    # every accepted member: [e] returns e, [e, e] with signs (0, 1) returns zeros
    acc = corpus.ACCEPT_ENC
    off = sc.offsets([1] * len(acc) + [2] * len(acc))
    pts = acc + [e for e in acc for _ in range(2)]
    got, st, _ = _run(harness, tables, W, ct, 0, off, pts, bytes(len(acc)) + b"\0\1" * len(acc))
    assert st == bytes(2 * len(acc)) and got[:len(acc)] == acc and got[len(acc):] == [bytes(32)] * len(acc)


@pytest.mark.parametrize("W,ct", FORMS)
def test_rejected_scalars_take_precedence_over_a_rejected_point(harness, tables, oracle, bases, W, ct):
    p = sc.pool()
    bad_point = corpus.REJECT_ENC[0]
    lengths = [2, 2, 2, 2, 2, 2]
    off = sc.offsets(lengths)
    pts = [p[0], p[1], p[2], p[3], p[4], bad_point, p[5], p[6], bad_point, p[7], p[8], p[9]]
    for bad in pc.REJECTED_SCALARS:
        vals = [5, bad, bad, 6, 7, 8]
        bls = [1, 2, 3, bad, bad, 4]          # rows 1, 3: the scalar alone; rows 2, 4: the scalar and a bad point; rows 0, 5: fine
        got, st, _ = _run(harness, tables, W, ct, 0, off, pts, None, vals, 32, bls)
        vd, _ = _run(harness, tables, W, 0, 1, off, pts, None, vals, 32, bls)
        assert st == bytes([sc.OK] + [sc.BAD_SCALAR] * 4 + [sc.OK])
        assert vd == bytes([sc.VERIFICATION_ERROR] + [sc.FORMAT_ERROR] * 4 + [sc.VERIFICATION_ERROR])
        assert got[1:5] == [bytes(32)] * 4
        for r in (0, 5):
            assert got[r] == sc.expect_row(oracle, bases[0], bases[1], pts[off[r]:off[r + 1]], None, vals[r], bls[r])[1]
    # a u64 value beside a blinding that is not canonical
    got, st, _ = _run(harness, tables, W, ct, 0, [0, 1, 2], p[:2], None, [3, 4], 8, [pc.L_ORDER, 1])
    assert st == bytes([sc.BAD_SCALAR, sc.OK]) and got[0] == bytes(32)


@pytest.mark.parametrize("W", [7, 13])
def test_balance_accepts_sums_of_commitments_and_rejects_one_flipped_bit(harness, tables, oracle, bases, W):
    lengths = [1, 2, 3, 0, 64, 65, 7]
    off, pts, vals, bls = sc.balanced_rows(oracle, bases[0], bases[1], lengths)
    nb = len(lengths)
    for vb in (8, 32):
        assert _run(harness, tables, W, 0, 1, off, pts, None, vals, vb, bls)[0] == bytes(nb)
    # the sum form agrees: minus the terms plus the opening is the identity
    got, st, _ = _run(harness, tables, W, 0, 0, off, pts, sc.signs("ones", off[-1]), vals, 8, bls)
    assert st == bytes(nb) and got == [bytes(32)] * nb
    bad = bytes(sc.VERIFICATION_ERROR if n else sc.BALANCED for n in lengths)
    flipped = list(pts)
    for r, n in enumerate(lengths):
        if n:
            t = off[r] + (5 * r) % n
            flipped[t] = pc.flip_bit(pts[t], (37 * r + 9) % 255)
    assert _run(harness, tables, W, 0, 1, off, flipped, None, vals, 8, bls)[0] == bad
    every = bytes([sc.VERIFICATION_ERROR]) * nb
    assert _run(harness, tables, W, 0, 1, off, pts, None, [v ^ (1 << ((11 * r + 3) % 64)) for r, v in enumerate(vals)], 8, bls)[0] == every
    bl2 = [b ^ (1 << ((13 * r) % 252)) for r, b in enumerate(bls)]
    bl2 = [f if f < pc.L_ORDER else (b & (b - 1) if b else 1) for f, b in zip(bl2, bls)]
    assert _run(harness, tables, W, 0, 1, off, pts, None, vals, 8, bl2)[0] == every
    # the terms subtracted: they open to minus the sums
    neg_v, neg_b = [(pc.L_ORDER - v) % pc.L_ORDER for v in vals], [(pc.L_ORDER - b) % pc.L_ORDER for b in bls]
    assert _run(harness, tables, W, 0, 1, off, pts, sc.signs("ones", off[-1]), neg_v, 32, neg_b)[0] == bytes(nb)


@pytest.mark.parametrize("W", [7, 13])
def test_a_one_term_balance_row_has_the_open_bodys_verdict(harness, tables, oracle, bases, W):
    """contract (c) on the (value, blinding) matrix: right openings, one bit flipped in the commitment / the value / the blinding, an
    encoding that does not decode, scalars that are not canonical"""
    rows = pc.rows()
    vals, bls = [v for v, _ in rows], [r for _, r in rows]
    coms = [pc.expect(oracle, bases[0], bases[1], v, r) for v, r in rows]
    n = len(rows)

    def both(c, v, vb, b):
        vd = C.create_string_buffer(n)
        harness.ped_open_rows(W, n, sc.pack(v, vb), vb // 4, b"".join(pc.le32(x) for x in b), b"".join(c), IDS, tables[W], vd)
        mine = _run(harness, tables, W, 0, 1, list(range(n + 1)), c, None, v, vb, b)[0]
        assert mine == vd.raw
        return mine
    assert both(coms, vals, 8, bls) == bytes(n) and both(coms, vals, 32, bls) == bytes(n)
    assert both([pc.flip_bit(c, (37 * i) % 256) for i, c in enumerate(coms)], vals, 8, bls) == bytes([sc.VERIFICATION_ERROR]) * n
    assert both(coms, [v ^ (1 << ((11 * i) % 64)) for i, v in enumerate(vals)], 8, bls) == bytes([sc.VERIFICATION_ERROR]) * n
    mixed_c = list(coms)
    mixed_v, mixed_b = list(vals), list(bls)
    mixed_c[2], mixed_c[3] = b"\xff" * 32, (1).to_bytes(32, "little")
    mixed_v[4], mixed_b[5] = pc.L_ORDER, pc.L_ORDER
    mixed_c[6], mixed_v[6] = corpus.REJECT_ENC[1], 2**256 - 1               # both: the scalar takes precedence in either body
    got = both(mixed_c, mixed_v, 32, mixed_b)
    assert got[:7] == bytes([0, 0, 1, 1, 2, 2, 2]) and got[7:] == bytes(n - 7)


def test_pinned_on_the_references_golden_commitments(harness, tables, oracle, bases, golden):
    """the vc[j] = j B + r_j B_blinding of tests/golden/rangeproof_v1.json and chacha_rng.golden_blindings(): their sum opens to
    (28, sum r_j mod l); vc[7] - vc[3] - vc[4] opens to (0, r_7 - r_3 - r_4 mod l) and not to value 1"""
    from chacha_rng import golden_blindings
    vc = [golden["vc_bytes"][32 * j:32 * j + 32] for j in range(8)]
    r = [int.from_bytes(b, "little") for b in golden_blindings()]
    L = pc.L_ORDER
    off, pts, sg = [0, 8, 11, 14], vc + [vc[7], vc[3], vc[4]] * 2, bytes(8) + b"\0\1\1" * 2
    vals, bls = [28, 0, 1], [sum(r) % L, (r[7] - r[3] - r[4]) % L, (r[7] - r[3] - r[4]) % L]
    for W in (7, 13):
        assert _run(harness, tables, W, 0, 1, off, pts, sg, vals, 8, bls)[0] == bytes([0, 0, sc.VERIFICATION_ERROR])
        got, st, _ = _run(harness, tables, W, 0, 0, off[:3], pts[:11], sg[:11])
        assert st == bytes(2) and got == [pc.expect(oracle, bases[0], bases[1], 28, bls[0]), pc.expect(oracle, bases[0], bases[1], 0, bls[1])]


def test_stand_alone_harness_is_clean_under_address_and_ub_sanitizers(tmp_path):
    """the harness as a program with its own main, -fsanitize=address,undefined, every buffer at its exact size"""
    exe = str(tmp_path / "pedersen_sum_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DPSUM_HARNESS_MAIN", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pedersen sum harness ok" in out.stdout
