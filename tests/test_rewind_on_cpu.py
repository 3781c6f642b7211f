"""Rewinding without a GPU: rewind.h's lane bodies compiled for the host (tests/rewind_harness) and run lane by lane over the
two-generator window table of tests/pedersen_harness -- the variable-time walk at W = 7 and 13, the constant-time walk at W = 4 --
against tests/rewind_twin.py at n = 8 (bp_twin's prover under the draw wrapper, the rewind in integers).  Start states lie at STROBE
positions 0, 100, 150 and 165, and 40 beside them: the separator crosses the 166-byte rate boundary from 150 and 165, V from 100,
A from 40, S from 0, 150 and 165.  (T_1 cannot cross: the challenge z before it always leaves the position at 64.)  The same harness
also runs as a stand-alone program under AddressSanitizer and UBSan with every buffer at its exact size."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "rewind_harness", "harness.cpp")
FORMS = [(4, 1), (7, 0), (13, 0)]       # (W, constant-time form)
POSITIONS = (0, 100, 150, 165, 40)
IDS = (C.c_uint32 * 2)(1, 0)            # the table lists [B, B_blinding]: B_blinding is row 1, B row 0
TS, N, PL = 208, 8, 32 * 15


@pytest.fixture(scope="module")
def tw(oracle):
    import rewind_twin
    return rewind_twin


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rewind") / "librewind.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    lib = C.CDLL(so)
    vp, u32, cp = C.c_void_p, C.c_uint32, C.c_char_p
    lib.ped_table_entries.restype = C.c_uint64
    lib.ped_table_entries.argtypes = [u32, u32]
    lib.ped_build_table.argtypes = [u32, u32, cp, vp]
    lib.rwd_rows.restype = None
    lib.rwd_rows.argtypes = [C.c_int, u32, u32, u32, cp, cp, cp, cp, u32, C.POINTER(u32), vp, vp, vp, vp, vp]
    lib.rwd_replay_rows.restype = None
    lib.rwd_replay_rows.argtypes = [u32, u32, cp, cp, cp, u32, vp, vp, vp]
    lib.rwd_draw_rows.restype = None
    lib.rwd_draw_rows.argtypes = [u32, cp, cp, cp, u32, vp, vp]
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


@pytest.fixture(scope="module")
def cases(tw, gens):
    """One batch shared by the tests and left unchanged: the twin's rewindable proofs at n = 8 over the start positions, values 0, 1
    and 2^n - 1, blindings 0, 1, l - 1 and random ones, the message absent, zero and sixteen 0xff bytes; row 0 is (0, 0): V is 32 zero
    bytes and the walk never starts"""
    rows = []
    plan = [(0, 0, None), (1, 1, bytes(16)), (255, tw.L - 1, b"\xff" * 16), (255, None, b"\xff" * 16), (0, None, b"rewind message 4"),
            (1, None, None), (77, None, bytes(range(16))), (255, 1, None), (128, 0, b"\xff" * 16), (3, None, b"\x01" + bytes(15))]
    for i, (v, g, msg) in enumerate(plan):
        state = tw.state_at(POSITIONS[i % len(POSITIONS)], b"row%d" % i)
        g = tw.det_scalar(b"g", i) if g is None else g
        seed = tw.det_seed(b"s", i)
        proof, V, _ = tw.prove(gens["bp"], gens["pc"], state, v, g, N, seed, msg)
        assert tw.rewind(gens["pc"], state, proof, V, N, seed) == (tw.OK, v, msg or bytes(16), g)
        rows.append(dict(state=state, v=v, g=g, msg=msg or bytes(16), seed=seed, proof=proof, V=V))
    assert rows[0]["V"] == bytes(32)
    return rows


def _rewind(harness, tables, W, ct, rows, shared_state=None):
    nb = len(rows)
    guard = lambda n: C.create_string_buffer(b"\x5a" * (n + 1), n + 1)      # one guard byte behind the last row
    st, vo, mo, go = guard(nb), guard(8 * nb), guard(16 * nb), guard(32 * nb)
    states = shared_state if shared_state is not None else b"".join(r["state"] for r in rows)
    harness.rwd_rows(ct, W, N, nb, b"".join(r["proof"] for r in rows), b"".join(r["V"] for r in rows), b"".join(r["seed"] for r in rows), states,
                     0 if shared_state is not None else TS // 4, IDS, tables[W], st, vo, mo, go)
    assert st.raw[nb:] == b"\x5a" and vo.raw[8 * nb:] == b"\x5a" and mo.raw[16 * nb:] == b"\x5a" and go.raw[32 * nb:] == b"\x5a"
    return [(st.raw[i], int.from_bytes(vo.raw[8 * i:8 * i + 8], "little"), mo.raw[16 * i:16 * i + 16], int.from_bytes(go.raw[32 * i:32 * i + 32], "little"))
            for i in range(nb)]


def test_the_start_positions_put_the_messages_across_the_rate_boundary(tw, cases):
    crossed = {"sep": set(), "V": set(), "A": set(), "S": set(), "T": set()}
    for row in cases:
        p0 = row["state"][200]
        pV, pA, pS, pT1, pT1e, pT2e = tw.positions(row["state"], N, row["V"], row["proof"])
        if pV < p0:
            crossed["sep"].add(p0)
        if pA < pV:
            crossed["V"].add(p0)
        if pS < pA:
            crossed["A"].add(p0)
        if (pS + 41) >= tw.RATE:
            crossed["S"].add(p0)
        if pT1 != 64 or pT1e < pT1 or pT2e < pT1e:
            crossed["T"].add(p0)
    assert crossed == {"sep": {150, 165}, "V": {100}, "A": {40}, "S": {0, 150, 165}, "T": set()}


@pytest.mark.parametrize("W,ct", FORMS)
def test_rewound_rows_equal_the_twin(harness, tables, cases, tw, W, ct):
    """every row comes back as (OK, v, msg, gamma), one state per row"""
    got = _rewind(harness, tables, W, ct, cases)
    for i, r in enumerate(cases):
        assert got[i] == (tw.OK, r["v"], r["msg"], r["g"]), i


@pytest.mark.parametrize("W,ct", FORMS)
def test_each_way_to_miss_stands_alone_among_good_rows(harness, tables, cases, tw, gens, W, ct):
    """wrong seed, e_blinding + 1 (step 5 with step 3 passing), t_x_blinding + 1, wrong transcript, another row's commitment, A of 32
    zero bytes: NOT_FOUND; e_blinding = l, a = l: FORMAT; an ordinary seeded proof under its own seed: NOT_FOUND.  The status and the
    outputs equal the twin's, a row that is not OK has all-zero outputs, and the good rows do not move."""
    rows = [dict(r) for r in cases]
    bump = lambda b, off: b[:off] + ((int.from_bytes(b[off:off + 32], "little") + 1) % tw.L).to_bytes(32, "little") + b[off + 32:]
    lb = tw.L.to_bytes(32, "little")
    rows[1]["seed"] = tw.det_seed(b"other", 1)
    rows[2]["proof"] = bump(rows[2]["proof"], 192)
    rows[3]["proof"] = bump(rows[3]["proof"], 160)
    rows[4]["state"] = tw.state_at(POSITIONS[4], b"someone else")
    rows[5]["V"] = cases[6]["V"]
    rows[6]["proof"] = bytes(32) + rows[6]["proof"][32:]
    rows[7]["proof"] = rows[7]["proof"][:192] + lb + rows[7]["proof"][224:]
    rows[8]["proof"] = rows[8]["proof"][:PL - 64] + lb + rows[8]["proof"][PL - 32:]
    # row 9: the seeded prover's own proof (no value taken off draw 0)
    t = tw.transcript_from_state(rows[9]["state"])
    pr, Vs = tw.T.prove_multiple(gens["bp"], gens["pc"], t, [rows[9]["v"]], [rows[9]["g"]], N, tw.RewindRng(rows[9]["seed"], 0))
    rows[9]["proof"], rows[9]["V"] = pr.to_bytes(), Vs[0]
    got = _rewind(harness, tables, W, ct, rows)
    want = [tw.rewind(gens["pc"], r["state"], r["proof"], r["V"], N, r["seed"]) for r in rows]
    assert got == want
    assert [g[0] for g in got] == [tw.OK] + [tw.NOT_FOUND] * 6 + [tw.FORMAT] * 2 + [tw.NOT_FOUND]
    assert all(g[1:] == (0, bytes(16), 0) for g in got[1:])
    # e_blinding + 1 passes step 3 (e - 1 is still below 2^192: v = 255) and fails at the commitment
    e = (tw.payload(cases[2]["v"], cases[2]["msg"]) - 1) % tw.L
    assert e >> 192 == 0


def test_one_shared_state(harness, tables, cases, tw, gens):
    """stride 0: every row from one state"""
    state = tw.state_at(150, b"shared")
    rows = []
    for i in range(3):
        v, g, seed = 200 + i, tw.det_scalar(b"sh", i), tw.det_seed(b"sh", i)
        proof, V, _ = tw.prove(gens["bp"], gens["pc"], state, v, g, N, seed, None if i else b"shared state msg")
        rows.append(dict(state=state, v=v, g=g, msg=bytes(16) if i else b"shared state msg", seed=seed, proof=proof, V=V))
    for W, ct in FORMS[:2]:
        got = _rewind(harness, tables, W, ct, rows, shared_state=state)
        assert got == [(tw.OK, r["v"], r["msg"], r["g"]) for r in rows]


def test_the_replay_gives_the_twins_challenges(harness, cases, tw):
    nb = len(cases)
    st, xs, zs = (C.create_string_buffer(n) for n in (4 * nb, 32 * nb, 32 * nb))
    harness.rwd_replay_rows(N, nb, b"".join(r["proof"] for r in cases), b"".join(r["V"] for r in cases), b"".join(r["state"] for r in cases), TS // 4, st, xs, zs)
    assert st.raw == bytes(4 * nb)
    for i, r in enumerate(cases):
        t = tw.transcript_from_state(r["state"])
        t.rangeproof_domain_sep(N, 1)
        for label, off in ((b"V", None), (b"A", 0), (b"S", 32)):
            t.append_point(label, r["V"] if off is None else r["proof"][off:off + 32])
        t.challenge_scalar(b"y")
        z = t.challenge_scalar(b"z")
        t.append_point(b"T_1", r["proof"][64:96])
        t.append_point(b"T_2", r["proof"][96:128])
        x = t.challenge_scalar(b"x")
        assert int.from_bytes(xs.raw[32 * i:32 * i + 32], "little") == x and int.from_bytes(zs.raw[32 * i:32 * i + 32], "little") == z, i


def test_the_provers_draw_source_takes_e_off_draw_zero_only(harness, cases, tw):
    """rpp_from_seed_rw: draw 0 is d_0 - (v + 2^64 msg) mod l, with and without a message buffer; every other draw is the seed's"""
    nb = len(cases)
    seeds = b"".join(r["seed"] for r in cases)
    vals = b"".join(r["v"].to_bytes(8, "little") for r in cases)
    msgs = b"".join(r["msg"] for r in cases)
    sc = lambda buf, i: int.from_bytes(buf.raw[32 * i:32 * i + 32], "little")
    for d in (0, 1, 2 * N + 2, 2 * N + 3):
        for m in (msgs, None):
            rw, plain = C.create_string_buffer(32 * nb), C.create_string_buffer(32 * nb)
            harness.rwd_draw_rows(nb, seeds, vals, m, d, rw, plain)
            for i, r in enumerate(cases):
                dk = tw.draws(r["seed"], d + 1)[d]
                assert sc(plain, i) == dk
                assert sc(rw, i) == ((dk - tw.payload(r["v"], r["msg"] if m else None)) % tw.L if d == 0 else dk), (d, i)


def test_stand_alone_harness_is_clean_under_address_and_ub_sanitizers(tmp_path):
    """the harness as a program with its own main, -fsanitize=address,undefined, every buffer at its exact size, run directly"""
    exe = str(tmp_path / "rewind_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DRWD_HARNESS_MAIN", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "rewind harness ok" in out.stdout
