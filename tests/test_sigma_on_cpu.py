"""The sigma proofs of recorded relations without a GPU: sigma.h's lane bodies compiled for the host (tests/sigma_harness) and run lane by
lane over a ten-generator window table (B_blinding, B, G_0 .. G_7 by base id) -- the variable-time forms at W = 7 and 13, the constant-time
forms at W = 4 -- against tests/sigma_twin.py for the relations R1 .. R5 of tests/sigma_cases.py.  Start states lie at STROBE positions 0,
100, 150 and 165.  The same harness also runs as a stand-alone program under AddressSanitizer and UBSan with every buffer at its exact
size."""
import ctypes as C
import hashlib
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "sigma_harness", "harness.cpp")
FORMS = [(4, 1), (7, 0), (13, 0)]       # (W, constant-time forms)
NAMES = ["R1", "R2", "R3", "R4", "R5"]
NGENS = 10
TS = 208


@pytest.fixture(scope="module")
def tw(oracle):
    import sigma_twin
    return sigma_twin


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sigma") / "libsigma.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    lib = C.CDLL(so)
    vp, u32, cp = C.c_void_p, C.c_uint32, C.c_char_p
    lib.ped_table_entries.restype = C.c_uint64
    lib.ped_table_entries.argtypes = [u32, u32]
    lib.ped_build_table.argtypes = [u32, u32, cp, vp]
    lib.sig_rel_from_desc.argtypes = [cp, u32, u32, vp]
    lib.sig_kP.argtypes = [C.c_int, cp, cp, vp]
    lib.sig_create_rows.restype = None
    lib.sig_create_rows.argtypes = [C.c_int, u32, u32, vp, u32, u32, cp, cp, cp, cp, u32, vp, vp, vp, vp]
    lib.sig_front_rows.restype = None
    lib.sig_front_rows.argtypes = [vp, u32, cp, cp, cp, u32, cp, vp, vp, vp, vp, vp, vp]
    lib.sig_weigh_rows.restype = None
    lib.sig_weigh_rows.argtypes = [vp, u32, cp, vp, vp, vp, vp, cp, vp, vp, vp, vp]
    return lib


@pytest.fixture(scope="module")
def bases(tw):
    return tw.shared_bases(8)


@pytest.fixture(scope="module")
def tables(harness, bases):
    gens = b"".join(bases[i] for i in range(NGENS))
    out = {}
    for W, _ in FORMS:
        buf = C.create_string_buffer(harness.ped_table_entries(W, NGENS) * harness.ped_table_entry_bytes())
        assert harness.ped_build_table(W, NGENS, gens, buf) == 0
        out[W] = buf
    return out


@pytest.fixture(scope="module")
def rels(harness, tw):
    import sigma_cases
    out = {}
    for name, rel in sigma_cases.RELATIONS.items():
        buf = C.create_string_buffer(harness.sig_rel_bytes())
        desc = tw.descriptor(rel)
        assert harness.sig_rel_from_desc(desc, len(desc), 8, buf) == 0
        out[name] = buf
    return out


@pytest.fixture(scope="module")
def cases(tw, bases):
    """Per relation one batch over the four start positions, shared by the tests and left unchanged"""
    import sigma_cases
    return {name: sigma_cases.rows(tw, bases, name, 4 if name == "R5" else 6) for name in NAMES}


def _shape(rel):
    return rel[0], rel[1], len(rel[2])


def _create(harness, tables, rels, name, rel, W, ct, rows, slice_=64, shared_state=None):
    S, P, E = _shape(rel)
    nb, pl = len(rows), 32 * (E + S)
    out = C.create_string_buffer(b"\x5a" * (pl * nb + 1), pl * nb + 1)      # one guard byte behind the last row
    st = C.create_string_buffer(b"\x5a" * (nb + 1), nb + 1)
    to = C.create_string_buffer(b"\x5a" * (TS * nb + 1), TS * nb + 1)
    states = shared_state if shared_state is not None else b"".join(r["state"] for r in rows)
    harness.sig_create_rows(ct, W, NGENS, rels[name], nb, slice_, b"".join(x.to_bytes(32, "little") for r in rows for x in r["secrets"]),
                            b"".join(r["seed"] for r in rows), b"".join(b"".join(r["points"]) for r in rows), states,
                            0 if shared_state is not None else TS // 4, tables[W], out, st, to)
    assert out.raw[pl * nb:] == b"\x5a" and st.raw[nb:] == b"\x5a" and to.raw[TS * nb:] == b"\x5a"
    return [out.raw[pl * i:pl * i + pl] for i in range(nb)], st.raw[:nb], [to.raw[TS * i:TS * i + TS] for i in range(nb)]


def _front(harness, rels, name, rel, proofs, points, states=None, shared_state=None):
    S, P, E = _shape(rel)
    nb, U, GR = len(proofs), P + 1, 2 + max([b - 1 for _, t in rel[2] for _, b in t if 2 <= b < 16] + [1])
    z = lambda n: C.create_string_buffer(n)
    esc, ept, gsc, fst, fto, cs = z(32 * U * E * nb), z(32 * U * E * nb), z(32 * GR * E * nb), z(4 * nb), z(TS * nb), z(32 * nb)
    harness.sig_front_rows(rels[name], nb, b"".join(proofs), b"".join(b"".join(p) for p in points), None if states is None else b"".join(states), TS // 4,
                           shared_state, esc, ept, gsc, fst, fto, cs)
    w = lambda buf, i, n=32: buf.raw[n * i:n * i + n]
    n = lambda buf, i: int.from_bytes(w(buf, i), "little")
    return dict(status=[int.from_bytes(w(fst, i, 4), "little") for i in range(nb)], ts=[w(fto, i, TS) for i in range(nb)], c=[n(cs, i) for i in range(nb)],
                esc=esc, ept=ept, gsc=gsc, fst=fst, U=U, GR=GR,
                eq_sc=lambda p, k, u: n(esc, (p * E + k) * U + u), eq_pt=lambda p, k, u: w(ept, (p * E + k) * U + u), gen=lambda p, k, b: n(gsc, (p * E + k) * GR + b))


def test_the_start_positions_put_each_kind_of_message_across_the_rate_boundary(tw, cases):
    """over the cases the separator, the digest, an instance point and a T_k each cross the 166-byte rate boundary at least once.  A guard on
    the fixtures (it runs the twin alone and says nothing about the code): the tests below compare states byte for byte, and only cases that
    cross the boundary reach the absorb loop's wrap"""
    import sigma_cases
    crossed = set()
    for name in NAMES:
        rel = sigma_cases.RELATIONS[name]
        E = len(rel[2])
        for row in cases[name]:
            for kind, before, after in tw.positions(row["state"], rel, row["points"], [row["proof"][32 * k:32 * k + 32] for k in range(E)]):
                if after < before:
                    crossed.add(kind)
    assert crossed == {"sep", "digest", "P", "T"}, crossed


def test_the_descriptor_digest_equals_the_twin(harness, tw, rels):
    import sigma_cases
    for name, rel in sigma_cases.RELATIONS.items():
        assert rels[name].raw[16:48] == tw.digest(tw.descriptor(rel)), name       # sig_rel: S, P, E, G, then the digest's 8 words


@pytest.mark.parametrize("W,ct", FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_created_proofs_status_and_states_equal_the_twin(harness, tables, rels, cases, name, W, ct):
    import sigma_cases
    rel = sigma_cases.RELATIONS[name]
    rows = cases[name]
    proofs, st, ts = _create(harness, tables, rels, name, rel, W, ct, rows)
    assert st == bytes(len(rows))
    for i, r in enumerate(rows):
        assert proofs[i] == r["proof"], (name, i)
        assert ts[i] == r["out"], (name, i)


@pytest.mark.parametrize("W,ct", [(4, 1), (7, 0)])
def test_one_shared_state_and_rejected_rows(harness, tables, rels, tw, bases, cases, W, ct):
    """stride 0: every row from one state.  A secret of l, and an instance BASE that does not decode, void their rows alone: zero bytes,
    the status, the input state.  An lhs that does not decode is the verifier's business, not the prover's."""
    import sigma_cases
    rel = sigma_cases.RELATIONS["R4"]
    state = tw.state_at(150, b"shared")
    rows = [dict(r, state=state) for r in cases["R4"][:5]]
    rows[1] = dict(rows[1], secrets=[rows[1]["secrets"][0], tw.L, rows[1]["secrets"][2]])
    rows[2] = dict(rows[2], points=rows[2]["points"][:2] + [b"\xff" * 32])
    rows[3] = dict(rows[3], points=[b"\xff" * 32] + rows[3]["points"][1:])
    proofs, st, ts = _create(harness, tables, rels, "R4", rel, W, ct, rows, shared_state=state)
    for i, r in enumerate(rows):
        assert (proofs[i], st[i], ts[i]) == tw.create(state, rel, bases, r["points"], r["secrets"], r["seed"]), i
    assert st == bytes([0, tw.BAD_SCALAR, tw.BAD_POINT, 0, 0]) and proofs[1] == proofs[2] == bytes(160) and ts[1] == ts[2] == state


def test_slices_give_the_bytes_of_one_launch(harness, tables, rels, cases):
    """70 rows of R3 in slices of 64 (a second slice of 6 rows on the same workspace) equal the same rows one by one"""
    import sigma_cases
    rel = sigma_cases.RELATIONS["R3"]
    rows = (cases["R3"] * 12)[:70]
    proofs, st, ts = _create(harness, tables, rels, "R3", rel, 7, 0, rows, slice_=64)
    assert st == bytes(70)
    for i, r in enumerate(rows):
        assert proofs[i] == r["proof"] and ts[i] == r["out"], i


def test_k_times_p_per_lane_equals_the_oracle_in_both_forms(harness, tw, bases):
    """0, 1, l - 1, 2^252 and a scalar of 0xf nibbles (in a carry-propagating recoding every window carries, out of the top one too); a
    point that does not decode is reported and the lane walks on the identity"""
    P = tw.msm([tw.det_scalar(b"kP", 0)], [bases[1]])
    ks = [0, 1, tw.L - 1, 2**252, (1 << 252) - 1, tw.det_scalar(b"kP", 1)]
    for k in ks:
        want = tw.msm([k], [P])
        for ct in (0, 1):
            out = C.create_string_buffer(32)
            assert harness.sig_kP(ct, tw.le32(k), P, out) == 1
            assert out.raw == want, (k, ct)
    out = C.create_string_buffer(32)
    assert harness.sig_kP(1, tw.le32(5), b"\xff" * 32, out) == 0 and out.raw == bytes(32)


@pytest.mark.parametrize("name", NAMES)
def test_the_front_end_equals_the_twin(harness, rels, tw, cases, name):
    """c, the staged coefficients per (row, equation) -- the sums of s over a slot's and a shared base's terms, - c on the lhs, - 1 on T_k,
    scalar 0 and the identity encoding for a slot the equation does not touch -- status and state; then each way to stop: an s_j of l
    (FormatError, the input state), a T_k of 32 zero bytes (VerificationError, the state as of that message)"""
    import sigma_cases
    rel = sigma_cases.RELATIONS[name]
    S, P, E = _shape(rel)
    rows = cases[name]
    proofs = [r["proof"] for r in rows]
    lb = tw.le32(tw.L)
    proofs[1] = proofs[1][:-32] + lb                                     # the last s_j = l
    kz = E - 1
    proofs[2] = proofs[2][:32 * kz] + bytes(32) + proofs[2][32 * kz + 32:]   # the last T_k zero: the earlier ones are absorbed
    proofs[3] = proofs[3][:32 * E + 8] + bytes([proofs[3][32 * E + 8] ^ 4]) + proofs[3][32 * E + 9:]   # a response that is merely wrong
    f = _front(harness, rels, name, rel, proofs, [r["points"] for r in rows], states=[r["state"] for r in rows])
    for i, r in enumerate(rows):
        st, so, c, s = tw.front(r["state"], rel, proofs[i], r["points"])
        assert f["status"][i] == st and f["ts"][i] == so, (name, i)
        for k in range(E):
            if st:
                assert all(f["eq_sc"](i, k, u) == 0 and f["eq_pt"](i, k, u) == bytes(32) for u in range(P + 1))
                assert all(f["gen"](i, k, b) == 0 for b in range(f["GR"]))
                continue
            slots, gens = tw.staged(rel, c, s, k)
            for u in range(P):
                assert f["eq_sc"](i, k, u) == slots.get(u, 0) and f["eq_pt"](i, k, u) == (r["points"][u] if u in slots else bytes(32)), (name, i, k, u)
            assert f["eq_sc"](i, k, P) == tw.L - 1 and f["eq_pt"](i, k, P) == proofs[i][32 * k:32 * k + 32]
            for b in range(f["GR"]):
                assert f["gen"](i, k, b) == gens.get(b, 0), (name, i, k, b)
        if not st:
            assert f["c"][i] == c
    assert [f["status"][i] for i in (1, 2, 3)] == [tw.FORMAT_ERROR, tw.VERIFICATION_ERROR, tw.OK]
    assert f["ts"][1] == rows[1]["state"] and f["ts"][2] not in (rows[2]["state"], rows[2]["out"]) and f["ts"][0] == rows[0]["out"]
    # one shared start state handed over by value (the shared_transcript of the _dev forms)
    g = _front(harness, rels, name, rel, [rows[0]["proof"]] * 2, [rows[0]["points"]] * 2, shared_state=rows[0]["state"])
    assert g["ts"] == [rows[0]["out"]] * 2 and g["c"][0] == g["c"][1] == f["c"][0]


@pytest.mark.parametrize("name", NAMES)
def test_the_weigh_map_sums_what_the_combined_check_needs(harness, rels, tw, bases, cases, name):
    """one weight per (row, equation); the combined list holds P + E terms per row -- scalar 0 and the identity encoding for a row that
    stopped -- and with the 2 + G shared rows it sums to the identity for valid rows"""
    import sigma_cases
    rel = sigma_cases.RELATIONS[name]
    S, P, E = _shape(rel)
    rows = cases[name]
    nb = len(rows)
    proofs = [r["proof"] for r in rows]
    proofs[2] = bytes(32) + proofs[2][32:]
    points = [r["points"] for r in rows]
    f = _front(harness, rels, name, rel, proofs, points, states=[r["state"] for r in rows])
    w64 = hashlib.shake_256(b"sigma weights" + name.encode()).digest(64 * nb * E)
    NU, GR = P + E, f["GR"]
    rho, csc, cpt, rws = (C.create_string_buffer(n) for n in (32 * nb * E, 32 * NU * nb, 32 * NU * nb, 32 * GR))
    harness.sig_weigh_rows(rels[name], nb, w64, f["fst"], f["gsc"], f["esc"], f["ept"], b"".join(b"".join(p) for p in points), rho, csc, cpt, rws)
    rhos = [int.from_bytes(w64[64 * i:64 * i + 64], "little") % tw.L for i in range(nb * E)]
    sc = lambda buf, i: int.from_bytes(buf.raw[32 * i:32 * i + 32], "little")
    assert [sc(rho, i) for i in range(nb * E)] == rhos
    for i in range(nb):
        if i == 2:
            assert csc.raw[32 * NU * i:32 * NU * (i + 1)] == bytes(32 * NU) == cpt.raw[32 * NU * i:32 * NU * (i + 1)]
            continue
        assert cpt.raw[32 * NU * i:32 * NU * (i + 1)] == b"".join(points[i]) + proofs[i][:32 * E]
        for u in range(P):
            assert sc(csc, NU * i + u) == sum(rhos[i * E + k] * f["eq_sc"](i, k, u) for k in range(E)) % tw.L
        for k in range(E):
            assert sc(csc, NU * i + P + k) == (tw.L - rhos[i * E + k]) % tw.L
    for b in range(GR):
        assert sc(rws, b) == sum(rhos[i * E + k] * f["gen"](i, k, b) for i in range(nb) if i != 2 for k in range(E)) % tw.L
    total = tw.msm([sc(rws, b) for b in range(GR)] + [sc(csc, j) for j in range(NU * nb)],
                   [bases[b] for b in range(GR)] + [cpt.raw[32 * j:32 * j + 32] for j in range(NU * nb)])
    assert total == bytes(32)


def test_stand_alone_harness_is_clean_under_address_and_ub_sanitizers(tmp_path):
    """the harness as a program with its own main, -fsanitize=address,undefined, every buffer at its exact size, run directly"""
    exe = str(tmp_path / "sigma_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DSIG_HARNESS_MAIN", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sigma harness ok" in out.stdout
