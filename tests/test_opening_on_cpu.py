"""The opening proofs without a GPU: opening.h's lane bodies compiled for the host (tests/opening_harness) and run lane by lane over the
two-generator window table of tests/pedersen_harness -- the variable-time walk at W = 7 and 13, the constant-time walk at W = 4 --
against tests/opening_twin.py (bp_twin's Merlin, chacha_rng's ChaChaRng, the oracle's multiscalar multiplication).  Start states lie at
STROBE positions 0, 100, 150 and 165, so that the separator, C and R each cross the 166-byte rate boundary once.  The same harness
also runs as a stand-alone program under AddressSanitizer and UBSan with every buffer at its exact size."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "opening_harness", "harness.cpp")
FORMS = [(4, 1), (7, 0), (13, 0)]       # (W, constant-time walk)
POSITIONS = (0, 100, 150, 165)
IDS = (C.c_uint32 * 2)(1, 0)            # the table lists [B, B_blinding]: B_blinding is row 1, B row 0
TS = 208


@pytest.fixture(scope="module")
def tw(oracle):
    import opening_twin
    return opening_twin


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("opening") / "libopening.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    lib = C.CDLL(so)
    vp, u32, cp = C.c_void_p, C.c_uint32, C.c_char_p
    lib.ped_table_entries.restype = C.c_uint64
    lib.ped_table_entries.argtypes = [u32, u32]
    lib.ped_build_table.argtypes = [u32, u32, cp, vp]
    lib.opn_create_rows.restype = None
    lib.opn_create_rows.argtypes = [C.c_int, u32, u32, u32, cp, u32, cp, cp, cp, cp, u32, C.POINTER(u32), vp, vp, vp, vp]
    lib.opn_front_rows.restype = None
    lib.opn_front_rows.argtypes = [u32, u32, cp, cp, cp, u32, cp, u32, cp, vp, vp, vp, vp, vp, vp]
    lib.opn_weigh_rows.restype = None
    lib.opn_weigh_rows.argtypes = [u32, cp, vp, vp, vp, vp, vp, vp, vp, vp]
    return lib


@pytest.fixture(scope="module")
def tables(harness, tw):
    B, Bb = tw.bases()
    out = {}
    for W, _ in FORMS:
        buf = C.create_string_buffer(harness.ped_table_entries(W, 2) * harness.ped_table_entry_bytes())
        assert harness.ped_build_table(W, 2, B + Bb, buf) == 0
        out[W] = buf
    return out


@pytest.fixture(scope="module")
def cases(tw):
    """One batch per form, shared by the tests and left unchanged: rows over the four start positions with values 0, 1, 2^64 - 1 and a
    few more below 2^64 (so that both value widths can carry them), the twin's proofs, states and challenges"""
    B, Bb = tw.bases()
    vals = [0, 1, 2**64 - 1, 0x0123456789abcdef, 7, 2**63, 42, 3]
    out = {}
    for form in (tw.FULL, tw.BLINDING):
        rows = []
        for i, v in enumerate(vals):
            state = tw.state_at(POSITIONS[i % 4], b"row%d" % i)
            r = tw.det_scalar(b"r%d" % form, i) if i != 1 else tw.L - 1
            Cc = tw.commit(B, Bb, v, r)
            seed = tw.det_seed(b"f%d" % form, i)
            proof, st, so = tw.create(state, form, B, Bb, Cc, v, r, seed)
            assert st == tw.OK and tw.verify(state, form, B, Bb, proof, Cc, v) == (tw.OK, so, bytes(32))
            rows.append(dict(state=state, v=v, r=r, C=Cc, seed=seed, proof=proof, out=so))
        out[form] = rows
    return dict(B=B, Bb=Bb, rows=out)


def _pack(vals, value_bytes):
    return b"".join(int(v).to_bytes(value_bytes, "little") for v in vals)


def _create(harness, tables, W, ct, form, rows, value_bytes, shared_state=None):
    nb = len(rows)
    pl = 96 if form == 0 else 64
    out = C.create_string_buffer(b"\x5a" * (pl * nb + 1), pl * nb + 1)      # one guard byte behind the last row
    st = C.create_string_buffer(b"\x5a" * (nb + 1), nb + 1)
    to = C.create_string_buffer(b"\x5a" * (TS * nb + 1), TS * nb + 1)
    states = shared_state if shared_state is not None else b"".join(r["state"] for r in rows)
    values = _pack([r["v"] for r in rows], value_bytes) if value_bytes else None
    harness.opn_create_rows(ct, W, form, nb, values, value_bytes // 4, b"".join(r["r"].to_bytes(32, "little") for r in rows), b"".join(r["seed"] for r in rows),
                            b"".join(r["C"] for r in rows), states, 0 if shared_state is not None else TS // 4, IDS, tables[W], out, st, to)
    assert out.raw[pl * nb:] == b"\x5a" and st.raw[nb:] == b"\x5a" and to.raw[TS * nb:] == b"\x5a"
    return [out.raw[pl * i:pl * i + pl] for i in range(nb)], st.raw[:nb], [to.raw[TS * i:TS * i + TS] for i in range(nb)]


def _front(harness, form, proofs, Cs, values, value_bytes, states=None, shared_state=None):
    nb = len(proofs)
    z = lambda n: C.create_string_buffer(n)
    usc, upt, gsc, fst, fto, cs = z(64 * nb), z(64 * nb), z(96 * nb), z(4 * nb), z(TS * nb), z(32 * nb)
    harness.opn_front_rows(form, nb, b"".join(proofs), b"".join(Cs), _pack(values, value_bytes) if values is not None else None,
                           value_bytes // 4 if values is not None else 0, None if states is None else b"".join(states), TS // 4, shared_state, usc, upt, gsc, fst,
                           fto, cs)
    word = lambda buf, i, n=32: buf.raw[n * i:n * i + n]
    return dict(status=[int.from_bytes(word(fst, i, 4), "little") for i in range(nb)], ts=[word(fto, i, TS) for i in range(nb)],
                c=[int.from_bytes(word(cs, i), "little") for i in range(nb)], usc=usc, upt=upt, gsc=gsc, fst=fst,
                neg_c=[int.from_bytes(word(usc, 2 * i), "little") for i in range(nb)], neg_1=[int.from_bytes(word(usc, 2 * i + 1), "little") for i in range(nb)],
                s_r=[int.from_bytes(word(gsc, 3 * i), "little") for i in range(nb)], s_v=[int.from_bytes(word(gsc, 3 * i + 1), "little") for i in range(nb)],
                g0=[word(gsc, 3 * i + 2) for i in range(nb)], pt_C=[word(upt, 2 * i) for i in range(nb)], pt_R=[word(upt, 2 * i + 1) for i in range(nb)])


def test_the_start_positions_put_each_message_across_the_rate_boundary_once(tw, cases):
    """positions 150 and 165: the separator crosses (to 34 and 49); 100: C's message (150 -> 25 in form 0); 0 and 165 in form 1, where the
    public value lies between C and R: R's message (132 -> 7, 131 -> 6)"""
    crossed = {"sep": set(), "C": set(), "R": set()}
    for form in (tw.FULL, tw.BLINDING):
        for row in cases["rows"][form]:
            p0, p1, p2, p3 = tw.positions(row["state"], form, row["C"], row["v"], row["proof"][:32])
            if p1 < p0:
                crossed["sep"].add(p0)
            if p2 < p1 and form == tw.FULL:
                crossed["C"].add(p0)
            if p3 < p2:
                crossed["R"].add(p0)
    assert 165 in crossed["sep"] and crossed["C"] and crossed["R"], crossed
    assert {p for s in crossed.values() for p in s} <= set(POSITIONS)


@pytest.mark.parametrize("W,ct", FORMS)
@pytest.mark.parametrize("form", [0, 1])
def test_created_proofs_status_and_states_equal_the_twin(harness, tables, cases, W, ct, form):
    """both value widths give the twin's bytes, status OK and the twin's advanced states"""
    rows = cases["rows"][form]
    for vb in (8, 32):
        proofs, st, ts = _create(harness, tables, W, ct, form, rows, vb)
        assert st == bytes(len(rows))
        for i, r in enumerate(rows):
            assert proofs[i] == r["proof"], (form, vb, i)
            assert ts[i] == r["out"], (form, vb, i)


@pytest.mark.parametrize("W,ct", [(4, 1), (7, 0)])
def test_one_shared_state_values_beyond_u64_and_rejected_rows(harness, tables, tw, cases, W, ct):
    """stride 0: every row from one state.  32-byte values l - 1 and 2^252; a value or blinding of l voids its row alone: zero bytes,
    status BAD_SCALAR, the input state.  Form 1 without a value buffer is the value 0."""
    B, Bb = cases["B"], cases["Bb"]
    state = tw.state_at(150, b"shared")
    for form in (0, 1):
        vals = [tw.L - 1, 2**252, tw.L, 5, 9]
        rs = [tw.det_scalar(b"rj", i) for i in range(5)]
        rs[3] = tw.L
        rows = []
        for i, (v, r) in enumerate(zip(vals, rs)):
            Cc = tw.commit(B, Bb, v % tw.L, r % tw.L)
            rows.append(dict(state=state, v=v, r=r, C=Cc, seed=tw.det_seed(b"rej", i)))
        proofs, st, ts = _create(harness, tables, W, ct, form, rows, 32, shared_state=state)
        for i, r in enumerate(rows):
            want = tw.create(state, form, B, Bb, r["C"], r["v"], r["r"], r["seed"])
            assert (proofs[i], st[i], ts[i]) == want, (form, i)
        assert st == bytes([0, 0, tw.BAD_SCALAR, tw.BAD_SCALAR, 0]) and proofs[2] == bytes(len(proofs[2])) and ts[3] == state
    zero = [dict(state=state, v=0, r=rs[0], C=tw.commit(B, Bb, 0, rs[0]), seed=tw.det_seed(b"zero", 0))]
    proofs, st, ts = _create(harness, tables, W, ct, 1, zero, 0, shared_state=state)
    assert (proofs[0], st[0], ts[0]) == tw.create(state, 1, B, Bb, zero[0]["C"], 0, rs[0], zero[0]["seed"])


@pytest.mark.parametrize("form", [0, 1])
def test_the_front_end_equals_the_twin(harness, tw, cases, form):
    """c, the staged scalars (-c on C, -1 on R, s_r and s_v in the generator row, 0 on G_0), status and state; then each way to stop:
    s_r = l, s_v = l (form 0), a public value of l (form 1): FormatError and the input state; R = 32 zero bytes: VerificationError and
    the state as of that message"""
    rows = cases["rows"][form]
    nb = len(rows)
    proofs = [r["proof"] for r in rows]
    lb = tw.le32(tw.L)
    proofs[1] = proofs[1][:-32] + lb
    proofs[2] = bytes(32) + proofs[2][32:]
    values = [r["v"] for r in rows]
    vb = 8
    if form == 0:
        proofs[3] = proofs[3][:32] + lb + proofs[3][64:]
    else:
        values[3], vb = tw.L, 32
    proofs[5] = proofs[5][:40] + bytes([proofs[5][40] ^ 4]) + proofs[5][41:]          # a response that is merely wrong: not the front end's business
    f = _front(harness, form, proofs, [r["C"] for r in rows], values if form == 1 else None, vb, states=[r["state"] for r in rows])
    for i, r in enumerate(rows):
        st, so, c, s_v, s_r = tw.front(r["state"], form, proofs[i], r["C"], values[i])
        assert f["status"][i] == st and f["ts"][i] == so, (form, i)
        if st:
            assert (f["neg_c"][i], f["neg_1"][i], f["s_r"][i], f["s_v"][i], f["pt_C"][i], f["pt_R"][i]) == (0, 0, 0, 0, bytes(32), bytes(32)), (form, i)
            continue
        assert f["c"][i] == c and f["neg_c"][i] == (tw.L - c) % tw.L and f["neg_1"][i] == tw.L - 1
        assert f["s_r"][i] == s_r and f["s_v"][i] == s_v and f["g0"][i] == bytes(32)
        assert f["pt_C"][i] == r["C"] and f["pt_R"][i] == proofs[i][:32]
    assert [f["status"][i] for i in (1, 2, 3)] == [tw.FORMAT_ERROR, tw.VERIFICATION_ERROR, tw.FORMAT_ERROR]
    assert f["ts"][1] == rows[1]["state"] and f["ts"][3] == rows[3]["state"] and f["ts"][2] not in (rows[2]["state"], rows[2]["out"])
    assert f["ts"][0] == rows[0]["out"]                                                 # contract (c): the verifier ends where the prover ended
    # one shared start state handed over by value (the shared_transcript of the _dev forms)
    state = rows[0]["state"]
    g = _front(harness, form, proofs[:1] * 2, [rows[0]["C"]] * 2, [rows[0]["v"]] * 2 if form == 1 else None, 8, shared_state=state)
    assert g["ts"] == [rows[0]["out"]] * 2 and g["c"][0] == f["c"][0] == g["c"][1]


@pytest.mark.parametrize("form", [0, 1])
def test_the_weigh_map_sums_what_the_combined_check_needs(harness, tw, cases, form):
    """rho_p from weights64; the combined list holds (-rho c, C), (-rho, R) per proof -- scalar 0 and the identity encoding for a row that
    stopped -- and the two rows sum rho s_r and rho s_v over the rows that went on; the combination of valid proofs is the identity"""
    import hashlib
    rows = cases["rows"][form]
    nb = len(rows)
    B, Bb = cases["B"], cases["Bb"]
    proofs = [r["proof"] for r in rows]
    proofs[4] = bytes(32) + proofs[4][32:]
    f = _front(harness, form, proofs, [r["C"] for r in rows], [r["v"] for r in rows] if form == 1 else None, 8, states=[r["state"] for r in rows])
    w64 = hashlib.shake_256(b"opening weights").digest(64 * nb)
    rho, csc, cpt, rws = (C.create_string_buffer(n) for n in (32 * nb, 64 * nb, 64 * nb, 64))
    harness.opn_weigh_rows(nb, w64, f["fst"], f["gsc"], f["usc"], f["upt"], rho, csc, cpt, rws)
    rhos = [int.from_bytes(w64[64 * i:64 * i + 64], "little") % tw.L for i in range(nb)]
    assert [int.from_bytes(rho.raw[32 * i:32 * i + 32], "little") for i in range(nb)] == rhos
    live = [i for i in range(nb) if i != 4]
    sc = lambda buf, i: int.from_bytes(buf.raw[32 * i:32 * i + 32], "little")
    for i in range(nb):
        if i == 4:
            assert csc.raw[64 * i:64 * i + 64] == bytes(64) and cpt.raw[64 * i:64 * i + 64] == bytes(64)
        else:
            assert sc(csc, 2 * i) == (tw.L - f["c"][i]) * rhos[i] % tw.L and sc(csc, 2 * i + 1) == (tw.L - 1) * rhos[i] % tw.L
            assert cpt.raw[64 * i:64 * i + 64] == rows[i]["C"] + proofs[i][:32]
    assert sc(rws, 0) == sum(rhos[i] * f["s_r"][i] for i in live) % tw.L and sc(rws, 1) == sum(rhos[i] * f["s_v"][i] for i in live) % tw.L
    total = tw.msm([sc(rws, 1), sc(rws, 0)] + [sc(csc, j) for j in range(2 * nb)], [B, Bb] + [cpt.raw[32 * j:32 * j + 32] for j in range(2 * nb)])
    assert total == bytes(32)


def test_stand_alone_harness_is_clean_under_address_and_ub_sanitizers(tmp_path):
    """the harness as a program with its own main, -fsanitize=address,undefined, every buffer at its exact size, run directly"""
    exe = str(tmp_path / "opening_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DOPN_HARNESS_MAIN", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "opening harness ok" in out.stdout
