"""Scanning under many keys without a GPU: scan.h's lane bodies compiled for the host (tests/scan_harness) and run lane by lane over the
grids k_scan.hip launches, against tests/scan_twin.py at n = 8: the variable-time walk at W = 7 and 13, the constant-time form at
W = 4; start states at STROBE positions 0, 40, 100, 150 and 165; nkeys in {1, 2, 3, 65} and rows in {1, 63, 64, 65}, so that rows x nkeys
is not a multiple of 64 and a workgroup's last lanes run past the grid.  The twin asserts the one-permutation claim for every candidate it
derives (position 91 after the key, one Keccak-f at 144 < 166); here the library's own constants are compared with what its prefix lane
computes.  The same harness also runs as a stand-alone program under AddressSanitizer and UBSan with every buffer at its exact size."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "scan_harness", "harness.cpp")
FORMS = [(4, 1), (7, 0), (13, 0)]       # (W, constant-time form)
POSITIONS = (0, 40, 100, 150, 165)
IDS = (C.c_uint32 * 2)(1, 0)            # the table lists [B, B_blinding]: B_blinding is row 1, B row 0
TS, N, PL = 208, 8, 32 * 15
NONE = 0xFFFFFFFF
NKEYS = (1, 2, 3, 65)
ROWS = (1, 63, 64, 65)


@pytest.fixture(scope="module")
def tw(oracle):
    import scan_twin
    return scan_twin


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("scan") / "libscan.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    lib = C.CDLL(so)
    vp, u32, cp = C.c_void_p, C.c_uint32, C.c_char_p
    lib.ped_table_entries.restype = C.c_uint64
    lib.ped_table_entries.argtypes = [u32, u32]
    lib.ped_build_table.argtypes = [u32, u32, cp, vp]
    lib.scn_rows.restype = C.c_uint64
    lib.scn_rows.argtypes = [C.c_int, u32, u32, u32, cp, cp, cp, u32, cp, u32, C.POINTER(u32), vp, vp, vp, vp, vp, vp, vp, vp]
    lib.scn_seed_rows.restype = None
    lib.scn_seed_rows.argtypes = [u32, cp, cp, u32, vp]
    lib.scn_prefix_pos.restype = u32
    lib.scn_prefix_meta.restype = u32
    lib.scn_prf_pos.restype = u32
    return lib


@pytest.fixture(scope="module")
def gens(tw):
    T = tw.T
    pc = T.PedersenGens()
    return dict(bp=T.BulletproofGens(N, 1), pc=pc, B=T.compress(pc.B), Bb=T.compress(pc.B_blinding))


@pytest.fixture(scope="module")
def tables(harness, gens):
    out = {}
    for W, _ in FORMS:
        buf = C.create_string_buffer(harness.ped_table_entries(W, 2) * harness.ped_table_entry_bytes())
        assert harness.ped_build_table(W, 2, gens["B"] + gens["Bb"], buf) == 0
        out[W] = buf
    return out


def key_of(j):
    return bytes([0x40 + (j & 0x3f)]) * 4 + j.to_bytes(4, "little") + b"scan test wallet key...."


@pytest.fixture(scope="module")
def cases(tw, gens):
    """Ten proofs shared by the tests and left unchanged: the twin's rewindable proofs at n = 8 over the five start positions, proof i
    made under the seed of (key_of(OWNER[i]), V_i).  Owners 0, 1, 2 and 64 put a row's key first, in the middle and last among 1, 2, 3
    and 65 keys; 999 is a key no scan holds."""
    R = tw.R
    rows = []
    plan = [(0, 0, None, 0), (1, 1, bytes(16), 1), (255, tw.L - 1, b"\xff" * 16, 2), (255, None, b"\xff" * 16, 64), (0, None, b"scan message  4.", 0),
            (1, None, None, 1), (77, None, bytes(range(16)), 2), (255, 1, None, 64), (128, 0, b"\xff" * 16, 999), (3, None, b"\x01" + bytes(15), 0)]
    for i, (v, g, msg, owner) in enumerate(plan):
        state = R.state_at(POSITIONS[i % len(POSITIONS)], b"row%d" % i)
        g = R.det_scalar(b"scan-g", i) if g is None else g
        V = tw.T.compress(gens["pc"].commit(v, g))
        seed = tw.seed_for(key_of(owner), V)
        proof, V2, _ = R.prove(gens["bp"], gens["pc"], state, v, g, N, seed, msg)
        assert V2 == V
        rows.append(dict(state=state, v=v, g=g, msg=msg or bytes(16), owner=owner, proof=proof, V=V))
    return rows


_memo = {}


def twin_scan(tw, gens, row, keys):
    """the twin's answer for one row, computed once per (row, keys)"""
    k = (row["state"], row["proof"], row["V"], tuple(keys))
    if k not in _memo:
        _memo[k] = tw.scan(gens["pc"], row["state"], row["proof"], row["V"], N, list(keys))
    return _memo[k]


def _scan(harness, tables, W, ct, rows, keys, shared_state=None):
    nb, nk = len(rows), len(keys)
    guard = lambda n: C.create_string_buffer(b"\x5a" * (n + 1), n + 1)      # one guard byte behind the last row
    st, ki, vo, mo, go, meta, cand = guard(nb), guard(4 * nb), guard(8 * nb), guard(16 * nb), guard(32 * nb), guard(4 * (nk + 1)), guard(4 * nb * nk)
    states = shared_state if shared_state is not None else b"".join(r["state"] for r in rows)
    ran = harness.scn_rows(ct, W, N, nb, b"".join(r["proof"] for r in rows), b"".join(r["V"] for r in rows), states, 0 if shared_state is not None else TS // 4,
                           b"".join(keys), nk, IDS, tables[W], st, ki, vo, mo, go, meta, cand)
    for buf, n in ((st, nb), (ki, 4 * nb), (vo, 8 * nb), (mo, 16 * nb), (go, 32 * nb), (meta, 4 * (nk + 1)), (cand, 4 * nb * nk)):
        assert buf.raw[n:] == b"\x5a"
    u32 = lambda buf, i: int.from_bytes(buf.raw[4 * i:4 * i + 4], "little")
    assert all(u32(meta, j) == harness.scn_prefix_meta() for j in range(nk)) and u32(meta, nk) & 0xff == 48
    got = [(st.raw[i], u32(ki, i), int.from_bytes(vo.raw[8 * i:8 * i + 8], "little"), mo.raw[16 * i:16 * i + 16],
            int.from_bytes(go.raw[32 * i:32 * i + 32], "little")) for i in range(nb)]
    return got, ran, [[u32(cand, i * nk + j) for j in range(nk)] for i in range(nb)]


def test_the_librarys_prefix_constants_are_the_twins(harness, tw):
    """the hot lane starts every candidate from constants (position 91, the key's AD begun at 58): they are what the twin measures, and
    what the prefix lane itself computes (checked in every _scan)"""
    seed, prefix_pos, ran = tw.seed_traced(key_of(0), bytes(32))
    assert harness.scn_prefix_pos() == prefix_pos == tw.PREFIX_POS == 91
    assert harness.scn_prefix_meta() == 91 | (58 << 8) | (2 << 16)
    assert ran == [tw.PRF_POS] and harness.scn_prf_pos() == tw.PRF_POS == 144 < tw.RATE


def test_seeds_of_the_two_step_derivation_equal_seed_for(harness, cases, tw):
    keys = [key_of(j) for j in (0, 1, 64, 999)]
    out = C.create_string_buffer(32 * len(cases) * len(keys))
    harness.scn_seed_rows(len(cases), b"".join(r["V"] for r in cases), b"".join(keys), len(keys), out)
    for i, r in enumerate(cases):
        for j, k in enumerate(keys):
            assert out.raw[32 * (i * len(keys) + j):32 * (i * len(keys) + j) + 32] == tw.seed_for(k, r["V"]), (i, j)


@pytest.mark.parametrize("W,ct", FORMS)
@pytest.mark.parametrize("nkeys", NKEYS)
def test_scanned_rows_equal_the_twin(harness, tables, cases, tw, gens, W, ct, nkeys):
    """rows 1, 63, 64 and 65 (the ten proofs in turn) under the first nkeys keys: status, key index and outputs equal the twin's, every
    replayed row costs nkeys candidate lanes, and a row whose owner is among the keys comes back under that key"""
    keys = [key_of(j) for j in range(nkeys)]
    for nrows in ROWS:
        rows = [cases[(i * 3 + nrows) % len(cases)] for i in range(nrows)]
        got, ran, cand = _scan(harness, tables, W, ct, rows, keys)
        assert ran == nrows * nkeys
        for i, r in enumerate(rows):
            want = twin_scan(tw, gens, r, keys)
            assert got[i] == want[:5], (nrows, i)
            if r["owner"] < nkeys:
                assert got[i] == (tw.OK, r["owner"], r["v"], r["msg"], r["g"]) and want[5] == tw.PRF_POS
                assert cand[i] == [j if j == r["owner"] else NONE for j in range(nkeys)]
            else:
                assert got[i] == (tw.NOT_FOUND, NONE, 0, bytes(16), 0) and cand[i] == [NONE] * nkeys


@pytest.mark.parametrize("W,ct", FORMS)
def test_each_way_to_miss_stands_alone_among_good_rows(harness, tables, cases, tw, gens, W, ct):
    """nobody's row, a FORMAT scalar, A / S / T_1 / T_2 of 32 zero bytes, a duplicated key, and e_blinding rewritten so that a LOWER key
    than the owner passes the 2^192 test (NOT_FOUND although the owner's key is listed): each equals the twin, a row that is not OK has
    zero outputs and key index 0xFFFFFFFF, a row whose replay failed spends no candidate lane, and the good rows do not move"""
    keys = [key_of(2), key_of(0), key_of(1), key_of(1), key_of(64)]      # key_of(1) twice: index 2 is reported
    rows = [dict(r) for r in cases]
    lb = tw.L.to_bytes(32, "little")
    zero = lambda b, off: b[:off] + bytes(32) + b[off + 32:]
    rows[0]["proof"] = rows[0]["proof"][:192] + lb + rows[0]["proof"][224:]          # FORMAT: e_blinding = l
    rows[2]["proof"] = zero(rows[2]["proof"], 0)                                       # A
    rows[3]["proof"] = zero(rows[3]["proof"], 32)                                      # S
    rows[4]["proof"] = zero(rows[4]["proof"], 64)                                      # T_1
    rows[6]["proof"] = zero(rows[6]["proof"], 96)                                      # T_2
    # row 7 (owner key_of(64), index 4): e_blinding rewritten for key_of(0), index 1 -- it passes step 2 and fails at the commitment
    rows[7]["proof"] = tw.forge_e_blinding(rows[7]["state"], rows[7]["proof"], rows[7]["V"], N, key_of(0), e=rows[7]["v"])
    got, ran, cand = _scan(harness, tables, W, ct, rows, keys)
    want = [twin_scan(tw, gens, r, keys) for r in rows]
    assert [g for g in got] == [w[:5] for w in want]
    assert [g[0] for g in got] == [tw.FORMAT, tw.OK, tw.NOT_FOUND, tw.NOT_FOUND, tw.NOT_FOUND, tw.OK, tw.NOT_FOUND, tw.NOT_FOUND, tw.NOT_FOUND, tw.OK]
    assert [g[1] for g in got] == [NONE, 2, NONE, NONE, NONE, 2, NONE, NONE, NONE, 1]
    assert all(g[2:] == (0, bytes(16), 0) for g in got if g[0] != tw.OK)
    assert ran == 5 * len(keys)                       # rows 1, 5, 7, 8, 9 were replayed
    assert cand[1] == [NONE, NONE, 2, 3, NONE]        # both copies of the key pass; the lower index is kept
    assert cand[7] == [NONE, 1, NONE, NONE, NONE]     # the forged e_blinding turned the owner's own candidate away too
    # without the forgery the same row opens under its owner
    got2, _, _ = _scan(harness, tables, W, ct, [cases[7]], keys)
    assert got2[0] == (tw.OK, 4, cases[7]["v"], cases[7]["msg"], cases[7]["g"])


def test_one_shared_state(harness, tables, tw, gens):
    """stride 0: every row from one state"""
    R = tw.R
    state = R.state_at(150, b"shared")
    keys = [key_of(j) for j in range(3)]
    rows = []
    for i in range(3):
        v, g = 200 + i, R.det_scalar(b"scan-sh", i)
        V = tw.T.compress(gens["pc"].commit(v, g))
        proof, _, _ = R.prove(gens["bp"], gens["pc"], state, v, g, N, tw.seed_for(keys[2 - i], V), None if i else b"shared state msg")
        rows.append(dict(state=state, v=v, g=g, msg=bytes(16) if i else b"shared state msg", proof=proof, V=V))
    for W, ct in FORMS[:2]:
        got, _, _ = _scan(harness, tables, W, ct, rows, keys, shared_state=state)
        assert got == [(tw.OK, 2 - i, r["v"], r["msg"], r["g"]) for i, r in enumerate(rows)]


def test_stand_alone_harness_is_clean_under_address_and_ub_sanitizers(tmp_path):
    """the harness as a program with its own main, -fsanitize=address,undefined, every buffer at its exact size, run directly (-O0:
    nothing is optimised away from under the sanitizers, and the lane bodies' inlined Keccak sites compile in a second instead of a minute)"""
    exe = str(tmp_path / "scan_main")
    subprocess.check_call(["g++", "-O0", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DSCN_HARNESS_MAIN", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "scan harness ok" in out.stdout
