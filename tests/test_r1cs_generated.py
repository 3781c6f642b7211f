"""Generated R1CS gadgets without a GPU (tests/r1cs_corpus.py): the named cases reach what they are meant to reach (asserted from
the recorded descriptors), the twin proves and verifies every case and rejects the proof under the next seed's circuit, the
product's recorders agree with the twin (descriptor, flattening, witness program), and the library accepts every recording.
Then the verifier's device code on the host (tests/r1cs_harness): status, transcript and every scalar of the mega-check, row by row,
against the twin's terms; once more as a sanitized executable whose buffers have their exact sizes; and the prover's witness lane
(r1p_witness_thread / r1p_eval_row) against the twin prover's a_L, a_R, a_O.

What the harness tests were seen to catch (each fault planted alone in a scratch copy of r1cs.h / r1cs_prover.h; [x] = the case of
test_verifier_device_code_on_the_host, "large" = ..._on_the_host_large, w[x] = test_witness_device_code_on_the_host):
  ladder start 30 - clz(pw) -> 31 / 29 (r1_weight_range)   [n2 n5 n64 n65 q63_one31 q64_one32 q65_one33 q127_one64 q129_one0 powers ch256 edge open_ends] large
  the same two in r1p_eval_row                              w[the same cases and large]
  pw = (chal >> 16) & 0x7f                                  [n5 n64 q64_one32 q65_one33 powers ch256]; in r1p_eval_row w[the same]
                                                            (pw = 0 is __builtin_clz(0): the sanitized child reports it; unsanitized the lane spins)
  nzhi = Q >> 6                                             [n64 n65 q64_one32 q65_one33 q127_one64 q128_one65 q129_one0] large
  (e >> 6) & 63 in r1_pow_from_tables                       large only (it takes Q >= 4 096 or padded_n > 4 096)
  last ONE chunk's end not clamped to b1                    19 cases, as an AddressSanitizer heap-buffer-overflow report (ONE is the last column)
  chunk start c * 31                                        [n64 n65 q65_one33 q127_one64 q128_one65 edge] large
  one_chunks rounded down                                   [n64 n65 q65_one33 q128_one65 edge] large
  sign fold of V / ONE dropped in r1cs_build_lists          every case with a V or ONE term (19)
Two planted faults pass, and are meant to: j = chal & 0xff instead of & 0xffff changes nothing while BPGPU_R1CS_MAX_CHALLENGES is 256
(j <= 255; the ch256 case uses challenge 255), and the fill order of one column reversed changes no weight -- the comparison is of
sums, and the order within a list is deliberately not pinned."""
import ctypes as C
import hashlib
import os
import random
import subprocess

import pytest

import r1cs_corpus as G
import r1cs_prover_twin as P
import r1cs_rlc_twin as RT
import r1cs_twin as R

HARNESS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "r1cs_harness", "harness.cpp")

L = R.L
SWEEP = [G.sweep_case(s) for s in range(1000, 1200)]           # 200 further seeds over random shape parameters


@pytest.fixture(scope="module")
def gens(oracle):
    return oracle.Gens(128, 1).export()


@pytest.fixture(scope="module")
def gens_large(oracle):
    return oracle.Gens(2048, 1).export()


# ---- what the named cases reach -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def named_features():
    return {c.name: G.features(G.record_verifier(c).descriptor()) for c in G.NAMED}


def test_named_cases_reach_the_listed_features(named_features):
    F = named_features
    small = [F[c.name] for c in G.SMALL]
    have = lambda key: {f[key] for f in small}
    powers, powers_coeff = set().union(*[f["powers"] for f in small]), set().union(*[f["powers_coeff"] for f in small])
    for kind in range(5):
        for p in G.POWERS:
            assert (kind, p) in powers and (kind, p) in powers_coeff, ("LROV1"[kind], p)
    assert {2, 8, 256} <= have("nch")
    f256 = F["ch256"]
    assert f256["nch"] == 256 and {0, 1, 1024} <= f256["label_lens"] and {0, 128, 255} <= f256["challenges"]
    assert any((kind, 255) in f256["powers"] and 255 in f256["challenges"] for kind in range(5))
    assert {0, 1, 63, 64, 65, 127, 128, 129} <= have("Q")
    assert {0, 1, 31, 32, 33, 64, 65} <= have("ones")
    assert {0, 1, 2, 3, 4, 5, 64, 65} <= have("n")
    pn = lambda n: 1 << max(n - 1, 0).bit_length()
    assert {pn(f["n"]) for f in small} >= {1, 2, 4, 8, 64, 128}
    assert any(f["n1"] == 0 and f["n2"] > 0 for f in small)
    assert any(f["two_phase"] and f["n2"] == 0 and f["nch"] > 0 and f["powers"] for f in small)
    assert any(f["two_phase"] and f["n2"] == 0 and f["nch"] == 0 for f in small)
    assert any(f["m"] == 0 and f["n"] > 0 for f in small) and any(f["m"] > 0 and f["n"] == 0 for f in small)
    assert any(f["empty"] for f in small) and any(f["zero_coeff"] for f in small) and any(f["repeated"] for f in small)
    assert any(f["widest"] >= 64 for f in small)
    assert any(not f["two_phase"] for f in small)
    big = F["large"]
    assert big["n"] == 1025 and big["Q"] >= 4160 and big["ones"] >= 2049 + 32
    # the exact targets of the cases that pin them
    for c in G.NAMED:
        if c.Q is not None:
            assert F[c.name]["Q"] == c.Q, c
        if c.ones is not None:
            assert F[c.name]["ones"] == c.ones, c


# ---- twin round trips and the recorders -------------------------------------------------------------------------------------
def _equivalent(a, b):
    """two cases record the same circuit as far as a verifier can tell: same shape and labels and, at one random point (z, challenges),
    the same weights (the weights are polynomials in z and the challenges: Schwartz-Zippel)"""
    from bulletproofs_amd import r1cs
    da, db = G.record_verifier(a).descriptor(), G.record_verifier(b).descriptor()
    if da[:5] != db[:5]:
        return False
    rnd = random.Random("equivalent")
    z, ch = rnd.randrange(L), [rnd.randrange(L) for _ in da[4]]
    return r1cs.flattened_constraints(da, z, ch) == r1cs.flattened_constraints(db, z, ch)


def _round_trip(case, gens):
    from bulletproofs_amd import r1cs
    st0 = G.st0_of(case)
    pf, Vs, twin = G.twin_prove(case, gens)
    proof = pf.to_bytes()
    code, mc, _ = R.verify_with(G.verifier_gadget(case), gens, case.cap, st0, proof, Vs, bytes(32))
    assert code == R.OK and mc == R.IDENTITY, case              # a valid proof, and it reached the mega-check
    other = case.with_seed(case.seed + 1)
    code2 = R.verify_with(G.verifier_gadget(other), gens, case.cap, st0, proof, Vs, bytes(32))[0]
    same = _equivalent(case, other)
    assert (code2 == R.OK) == same, (case, code2, same)
    # the recorders
    rp, rv = G.record_prover(case), G.record_verifier(case)
    d = rv.descriptor()
    assert rp.descriptor() == d
    assert (d[0], d[3], d[4]) == (case.m, case.two_phase, case.labels)
    assert P.eval_witness(rp, twin.challenges) == (twin.a_L, twin.a_R, twin.a_O), case
    rnd = random.Random(case.seed)
    z = rnd.randrange(L)
    assert r1cs.flattened_constraints(d, z, twin.challenges) == R.flattened_with(G.verifier_gadget(case), case.m, z, twin.challenges), case
    # the library accepts the recording
    circ = rv.circuit()
    n = d[1] + d[2]
    pn = 1 << max(n - 1, 0).bit_length()
    assert n == len(twin.a_L) and (circ.padded_n, circ.n_unique) == (pn, 11 + case.m + 2 * (pn.bit_length() - 1)), case
    assert len(proof) == 1 + 32 * ((14 if proof[0] else 11) + 2 * (pn.bit_length() - 1) + 2)
    rp.witness()
    return same


@pytest.mark.parametrize("case", G.SMALL, ids=[c.name for c in G.SMALL])
def test_named_case(gens, case):
    same = _round_trip(case, gens)
    assert not same or G.features(G.record_verifier(case).descriptor())["n"] == 0    # only a circuit with no multiplier may be seed-independent


def test_large_case(gens_large):
    assert not _round_trip(G.LARGE, gens_large)


@pytest.mark.parametrize("chunk", range(8))
def test_sweep(gens, chunk):
    same = [_round_trip(c, gens) for c in SWEEP[chunk::8]]
    assert sum(same) <= len(same) // 4          # (circuits without a tie -- no multiplier -- do not depend on the seed)


def test_sweep_is_varied():
    fs = [G.features(G.record_verifier(c).descriptor()) for c in SWEEP]
    assert len({(f["m"], f["n1"], f["n2"], f["nch"]) for f in fs}) >= 100
    assert sum(1 for f in fs if f["two_phase"]) >= 50 and sum(1 for f in fs if not f["two_phase"]) >= 20
    assert {p for f in fs for _, p in f["powers"]} >= set(G.POWERS)


# ---- the verifier's device code on the host (tests/r1cs_harness) ------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("r1h")
    so = str(d / "libr1h.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, HARNESS])
    lib = C.CDLL(so)
    lib.r1h_run_file.argtypes = [C.c_char_p, C.c_char_p]
    return lib, d


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    """the same harness as a standalone executable under AddressSanitizer and UBSan (host code only; run as a child process)"""
    exe = str(tmp_path_factory.mktemp("r1h-asan") / "harness")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DR1H_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-o", exe, HARNESS], capture_output=True, text=True)
    if r.returncode and os.path.exists("/dev/kfd") and ("asan" in r.stderr or "ubsan" in r.stderr):
        pytest.skip("no sanitizer runtime for g++ on this GPU machine")
    assert r.returncode == 0, r.stderr
    return exe


def _pad4(b):
    return bytes(b) + bytes(-len(b) % 4)


def _u32s(xs):
    return b"".join(int(x).to_bytes(4, "little") for x in xs)


def _case_file(d, proofs, coms, transcripts, rng32, gens_capacity):
    """the harness's input: the descriptor as Circuit() hands it to bpgpu_r1cs_circuit_create, then the batch"""
    m, n1, n2, two_phase, labels, cons = d
    row, kind, index, chal, power, coeff = [0], [], [], [], [], []
    for terms in cons:
        for (k_, i_), ch, pw, cf in terms:
            kind.append(k_)
            index.append(i_)
            chal.append(0xffffffff if ch is None else ch)
            power.append(0 if ch is None else pw)
            coeff.append((cf % L).to_bytes(32, "little"))
        row.append(len(kind))
    nb = len(proofs)
    stride = (max(len(p) for p in proofs) + 3) & ~3
    lbl = b"".join(labels)
    per_proof = len(transcripts) == 208 * nb and nb > 1
    assert len(transcripts) in (208, 208 * nb) and len(rng32) == 32 * nb and len(coms) == 32 * m * nb
    return b"".join([b"R1H1", _u32s([m, n1, n2, 1 if two_phase else 0, len(labels), len(cons), len(kind), nb, stride, 1 if per_proof else 0, gens_capacity, len(lbl)]),
                     _u32s(len(x) for x in labels), _pad4(lbl), _u32s(row), _pad4(bytes(kind)), _u32s(index), _u32s(chal), _u32s(power), b"".join(coeff),
                     _u32s(len(p) for p in proofs), b"".join(p + bytes(stride - len(p)) for p in proofs), coms, transcripts, rng32])


def _parse_output(out, nb, m):
    pn, k, U, one_chunks = (int.from_bytes(out[4 * i:4 * i + 4], "little") for i in range(4))
    off = 16
    status = [int.from_bytes(out[off + 4 * b:off + 4 * b + 4], "little") for b in range(nb)]
    off += 4 * nb
    ts = [out[off + 208 * b:off + 208 * b + 208] for b in range(nb)]
    off += 208 * nb
    ngen = 2 * pn + 2
    rows = lambda base, b, cnt: [out[base + 32 * (b * cnt + i):base + 32 * (b * cnt + i) + 32] for i in range(cnt)]
    gen = [rows(off, b, ngen) for b in range(nb)]
    off += 32 * ngen * nb
    usc = [rows(off, b, U) for b in range(nb)]
    off += 32 * U * nb
    upt = [rows(off, b, U) for b in range(nb)]
    assert off + 32 * U * nb == len(out) and U == 11 + m + 2 * k
    return pn, k, one_chunks, status, ts, gen, usc, upt


def _device_order(terms, pn, k, m):
    """the twin's mega-check terms (its own order: A_I1..S2, V, T, B, B_blinding, g, h, u^2, u^-2) as (name, (buffer, row), scalar, point):
    the row of each in the device's generator rows ("g") / per-proof rows ("u")"""
    sc, pt = terms
    assert len(sc) == len(pt) == 13 + m + 2 * pn + 2 * k
    names = ["A_I1", "A_O1", "S1", "A_I2", "A_O2", "S2"] + ["V_%d" % j for j in range(m)] + ["T_1", "T_3", "T_4", "T_5", "T_6"] + ["B", "B_blinding"] + \
            ["G_%d" % i for i in range(pn)] + ["H_%d" % i for i in range(pn)] + ["L_%d" % i for i in range(k)] + ["R_%d" % i for i in range(k)]
    where = [("u", i) for i in range(11 + m)] + [("g", 1), ("g", 0)] + [("g", 2 + i) for i in range(2 * pn)] + [("u", 11 + m + i) for i in range(2 * k)]
    return list(zip(names, where, sc, pt))


def _harness_inputs(case, gens, few=False):
    """(proofs, commitments): the tampered variants of the valid proof in each serialization it has; the valid proof is the last.
    few: a flipped t_x, a flipped a and the valid proof only"""
    pf, Vs, _ = G.twin_prove(case, gens)
    good = pf.to_bytes()
    if few:
        b1, b2 = bytearray(good), bytearray(good)
        b1[1 + 32 * ((6 if good[0] else 3) + 5) + 5] ^= 4
        b2[-40] ^= 1
        return [bytes(b1), bytes(b2), good], [b"".join(Vs)] * 3
    cases = G.tamper_cases(good, Vs)
    if good[0] == 0:
        cases = G.tamper_cases(pf.to_bytes(force_two_phase=True), Vs) + cases
    return [p for p, _ in cases], [cm for _, cm in cases]


def _run_both(lib, sanitized, fin, fout, fout2, case):
    """the sanitized build first, as a child process with a time limit (undefined behaviour that would make a lane spin is reported there),
    then the shared library in this process: both clean, the same bytes"""
    r = subprocess.run([sanitized, fin, fout2], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    if r.returncode:
        print(r.stderr[:8000])                    # (the head of a sanitizer report names the error and the line)
    assert r.returncode == 0, (case, r.stderr[:600])
    assert lib.r1h_run_file(fin.encode(), fout.encode()) == 0
    out = open(fout, "rb").read()
    assert open(fout2, "rb").read() == out, case
    return out


def _run_and_compare(harness, sanitized, case, gens, cap, per_proof, few=False):
    lib, tmp = harness
    proofs, coms = _harness_inputs(case, gens, few)
    nb, m = len(proofs), case.m
    st0 = G.st0_of(case)
    if per_proof:   # every other proof starts from a transcript with one message more
        t1 = R.transcript_from_state(st0)
        t1.append_message(b"extra", b"message")
        st0s = [R.transcript_state(t1) if (nb - 1 - i) % 2 else st0 for i in range(nb)]
    else:
        st0s = [st0] * nb
    rng32 = hashlib.shake_256(b"harness rng " + case.name.encode()).digest(32 * nb)
    rv = G.record_verifier(case)
    blob = _case_file(rv.descriptor(), proofs, b"".join(coms), b"".join(st0s) if per_proof else st0, rng32, cap)
    fin, fout, fout2 = (str(tmp / ("%s-%d%s" % (case.name, cap, x))) for x in (".bin", ".out", ".asan.out"))
    with open(fin, "wb") as f:
        f.write(blob)
    out = _run_both(lib, sanitized, fin, fout, fout2, case)
    pn, k, one_chunks, status, ts, gen, usc, upt = _parse_output(out, nb, m)
    circ = rv.circuit()
    assert (pn, 11 + m + 2 * k) == (circ.padded_n, circ.n_unique)
    reached = 0
    for b in range(nb):
        code, mc, ets, terms = RT.verify_terms(G.verifier_gadget(case), gens, cap, st0s[b], proofs[b], [coms[b][32 * j:32 * j + 32] for j in range(m)],
                                               rng32[32 * b:32 * b + 32])
        assert ts[b] == ets, (case, b)
        if terms is None:
            assert status[b] == code != 0, (case, b, status[b], code)
            continue
        reached += 1
        assert status[b] == 0, (case, b, status[b])
        for name, (buf, row), s, pt in _device_order(terms, pn, k, m):
            got = (gen if buf == "g" else usc)[b][row]
            assert int.from_bytes(got, "little") == s % L, (case, "proof %d" % b, name)
            if buf == "u":
                assert upt[b][row] == pt, (case, "proof %d" % b, name, "point")
    return reached, status


@pytest.mark.parametrize("case", G.SMALL, ids=[c.name for c in G.SMALL])
def test_verifier_device_code_on_the_host(harness, sanitized, gens, case):
    reached, status = _run_and_compare(harness, sanitized, case, gens, 128, per_proof=G.SMALL.index(case) % 2 == 1)
    assert reached >= 3 and status[-1] == 0            # the valid proof reaches the mega-check: no comparison is skipped


@pytest.mark.parametrize("name", ["powers", "ch256"])
def test_verifier_device_code_on_the_host_too_few_generators(harness, sanitized, gens, name):
    """gens_short: InvalidGeneratorsLength after the phase-2 challenge draws (3 and 256 of them), the transcript as of that moment"""
    case = next(c for c in G.SMALL if c.name == name)
    reached, status = _run_and_compare(harness, sanitized, case, gens, 8, per_proof=False)
    assert reached == 0 and status[-1] == 4 and set(status) <= {1, 2, 4}


def test_verifier_device_code_on_the_host_large(harness, sanitized, gens_large):
    """the large case (beyond what the issue asks of the harness): z^(q+1) with (q + 1) >> 6 >= 64, 66 ONE chunks, padded_n = 2 048"""
    reached, status = _run_and_compare(harness, sanitized, G.LARGE, gens_large, 2048, per_proof=False, few=True)
    assert reached == 3 and status == [0, 0, 0]


# ---- the prover's witness lane on the host ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.NAMED, ids=[c.name for c in G.NAMED])
def test_witness_device_code_on_the_host(harness, sanitized, gens, gens_large, case):
    """r1p_witness_thread / r1p_eval_row over the recorded witness program of two proofs, the challenge fields filled from the twin's
    draws: a_L, a_R, a_O equal the twin prover's"""
    lib, tmp = harness
    g = gens_large if case is G.LARGE else gens
    recs = [G.record_prover(case, idx) for idx in range(2)]
    twins = [G.twin_prove(case, g, idx)[2] for idx in range(2)]
    rp = recs[0]
    assert recs[1].structure() == rp.structure()
    d = rp.descriptor()
    n = d[1] + d[2]
    row, kind, index, chal, power, coeff = [0], [], [], [], [], []
    for terms in rp.rows:
        for (k_, i_), ch, pw, cf in terms:
            kind.append(k_)
            index.append(i_)
            chal.append(0xffffffff if ch is None else ch)
            power.append(0 if ch is None else pw)
            coeff.append((cf % L).to_bytes(32, "little"))
        row.append(len(kind))
    ins = [r.inputs() for r in recs]
    chv = b"".join(c.to_bytes(32, "little") for t in twins for c in t.challenges)
    assert all(len(t.challenges) == len(d[4]) for t in twins)
    blob = b"".join([b"R1W1", _u32s([d[0], d[1], d[2], len(d[4]), len(d[5]), len(rp.free), len(rp.rows), len(kind), 2]), _u32s(rp.src_left), _u32s(rp.src_right),
                     _u32s(row), _pad4(bytes(kind)), _u32s(index), _u32s(chal), _u32s(power), b"".join(coeff), b"".join(i[0] for i in ins),
                     b"".join(i[2] for i in ins), chv])
    fin, fout, fout2 = (str(tmp / ("%s-witness%s" % (case.name, x))) for x in (".bin", ".out", ".asan.out"))
    with open(fin, "wb") as f:
        f.write(blob)
    out = _run_both(lib, sanitized, fin, fout, fout2, case)
    assert len(out) == 2 * 3 * n * 32, case
    for b, t in enumerate(twins):
        got = [int.from_bytes(out[32 * (b * 3 * n + i):32 * (b * 3 * n + i) + 32], "little") for i in range(3 * n)]
        for name, want, have in (("a_L", t.a_L, got[:n]), ("a_R", t.a_R, got[n:2 * n]), ("a_O", t.a_O, got[2 * n:])):
            assert have == want, (case, "proof %d" % b, name, [i for i in range(n) if have[i] != want[i]][:8])
