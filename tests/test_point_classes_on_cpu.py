"""Every copy of the ristretto255 decoder and encoder in the device headers, by name, on the corpus of point_corpus.py: encodings
that fail exactly ONE of RFC 9496's five checks (non-canonical, negative s, not a square, negative t, y = 0), the valid ends of
the range, and all four Edwards representatives of each valid element.  Host build of the device code (tests/cpu_harness); the
expected values come from point_corpus.failed_checks (big ints), the twin and the C oracle.  Then the same members through the
lane-by-lane emulations of the MSM pipelines, one rejected member per MSM among valid neighbours: status 1 and a zero encoding
for exactly those MSMs; a member of each class at every point position of a range proof through the whole verification pipeline and
the batch-combined one (the decode role, and the second-table role beside it); members as the bases of the inner-product and linear
proof front ends.  A decoder copy that lost any one term of its conjunction fails here (test_gpu_point_classes.py and
test_gpu_point_classes_proofs.py send the same corpus through the shipped code objects)."""
import ctypes as C
import hashlib

import pytest

import bp_twin as T
import harness_lib
import point_corpus as PC

P = T.P
DECODERS = {0: "ristretto_decompress", 1: "ristretto_decompress_lp", 2: "hw_ristretto_decode"}
ENCODERS = {0: "ristretto_compress", 1: "compress_front+fe_invsqrt_raw+fix+back", 2: "bk2_tail_t4a+hw_invsqrt_raw_fe+bk2_tail_t4b", 3: "ristretto_compress_lp"}


@pytest.fixture(scope="module")
def H():
    return harness_lib.lib()


def _coords(buf, i):
    return tuple(int.from_bytes(buf[128 * i + 32 * k:128 * i + 32 * k + 32], "little") for k in range(4))


def _pt_bytes(q):
    return b"".join((c % P).to_bytes(32, "little") for c in q)


@pytest.mark.parametrize("which", sorted(DECODERS))
def test_each_decoder_copy_decides_and_decodes_as_rfc_9496(H, which):
    """verdict == (no check failed) on every member; the coordinates are the RFC's formulas carried to the end, accepted or not
    (the wavefront copy gives no verdict, and the narrow chain goes on to double whatever it leaves 128 times)."""
    enc = PC.ALL_ENC
    n = len(enc)
    xyzt, ok = C.create_string_buffer(128 * n), C.create_string_buffer(n)
    assert H.h_decode_copy(which, n, b"".join(enc), xyzt, ok) == 0
    for i, e in enumerate(enc):
        failed, pt = PC.decode_full(e)
        if which != 2:
            assert ok.raw[i] == (0 if failed else 1), (DECODERS[which], e.hex(), "".join(sorted(failed)))
        assert _coords(xyzt.raw, i) == pt, (DECODERS[which], e.hex())
        if not failed:
            assert T.decompress(e) == pt


@pytest.mark.parametrize("which", sorted(ENCODERS))
def test_each_encoder_copy_maps_all_four_representatives_to_the_member(H, which):
    reps, want = [], []
    for _, e in PC.ACCEPT:
        for q in PC.coset(PC.decode_full(e)[1]):
            reps.append(q)
            want.append(e)
    for q in PC.coset(T.IDENT):
        reps.append(q)
        want.append(bytes(32))
    # and the affine representatives themselves (Z = 1), as a decoder leaves them
    for _, e in PC.ACCEPT:
        reps.append(PC.decode_full(e)[1])
        want.append(e)
    out = C.create_string_buffer(32 * len(reps))
    assert H.h_encode_copy(which, len(reps), b"".join(_pt_bytes(q) for q in reps), out) == 0
    for i, e in enumerate(want):
        assert out.raw[32 * i:32 * i + 32] == e, (ENCODERS[which], i, e.hex())


# ---- the lane-by-lane pipelines ----------------------------------------------------------------------------------------
def _vb(H):
    def call(nt, S, Pp):
        out, st = C.create_string_buffer(32 * len(nt)), C.create_string_buffer(len(nt))
        H.h_msm_vb(len(nt), (C.c_uint32 * len(nt))(*nt), S, Pp, out, st)
        return out.raw, st.raw
    return call


def _narrow(H, levels):
    def call(nt, S, Pp):
        out, st = C.create_string_buffer(32 * len(nt)), C.create_string_buffer(len(nt))
        H.h_msm_vb_narrow(len(nt), (C.c_uint32 * len(nt))(*nt), 4, levels, S, Pp, out, st)
        return out.raw, st.raw
    return call


def _bucket(H, c, nsub):
    def call(nt, S, Pp):
        out, st = C.create_string_buffer(32 * len(nt)), C.create_string_buffer(len(nt))
        assert H.h_msm_bucket(len(nt), (C.c_uint32 * len(nt))(*nt), S, Pp, c, None, 0, nsub, out, st) == 0
        return out.raw, st.raw
    return call


def _bucket2(H, lanes):
    def call(nt, S, Pp):
        out, st = C.create_string_buffer(32 * len(nt)), C.create_string_buffer(len(nt))
        assert H.h_msm_bucket2(len(nt), (C.c_uint32 * len(nt))(*nt), S, Pp, lanes, out, st, None) == 0
        return out.raw, st.raw
    return call


def test_members_through_the_straus_pipeline(H, oracle):
    PC.check_msm_form(_vb(H), oracle, 5, b"vb")


@pytest.mark.parametrize("levels", [2, 4])
def test_members_through_the_narrow_pipeline_and_its_second_tables(H, oracle, levels):
    PC.check_msm_form(_narrow(H, levels), oracle, 5, b"narrow%d" % levels)


@pytest.mark.parametrize("c,nsub", [(8, 1), (8, 3), (12, 1), (12, 3)])
def test_members_through_the_old_bucket_chain(H, oracle, c, nsub):
    PC.check_msm_form(_bucket(H, c, nsub), oracle, 6, b"bucket%d-%d" % (c, nsub))


@pytest.mark.parametrize("lanes", [1, 7, 64, 256])
def test_members_through_the_fused_bucket_chain_and_its_short_register_decoder(H, oracle, lanes):
    PC.check_msm_form(_bucket2(H, lanes), oracle, 6, b"bucket2-%d" % lanes)


def test_members_through_the_shared_generator_pipeline(H, oracle):
    """Own points: one MSM per member.  Generator tables: a member of each class as a generator is refused by the table build."""
    W, nsplit, n, m = 4, 3, 8, 2
    G, Hh, B, Bb = oracle.Gens(n, m).export()
    gens = Bb + B + G + Hh
    ngen = 2 * n * m + 2
    ids = list(range(ngen))
    idv = (C.c_uint32 * ngen)(*ids)
    nu = 5
    US, UP, flags = PC.reject_batch(nu, b"shared")
    nb = len(flags)
    GS = b"".join(PC.scalars(ngen * nb, b"shared-g"))
    out, st, vd = C.create_string_buffer(32 * nb), C.create_string_buffer(nb), C.create_string_buffer(nb)
    assert H.h_msm_shared(W, nsplit, ngen, gens, ngen, idv, nb, nu, GS, US, UP, out, st, vd) == 0
    for b, rej in enumerate(flags):
        if rej:
            assert st.raw[b] == 1 and out.raw[32 * b:32 * b + 32] == bytes(32), b
        else:
            exp = oracle.msm(GS[32 * ngen * b:32 * ngen * (b + 1)] + US[32 * nu * b:32 * nu * (b + 1)], gens + UP[32 * nu * b:32 * nu * (b + 1)])
            assert exp[0] == 0 and st.raw[b] == 0 and out.raw[32 * b:32 * b + 32] == exp[1], b
    for k, (cls, e) in enumerate(PC.one_per_class()):
        for pos in (0, 1, 2, ngen - 1, 2 + (3 * k) % (ngen - 2)):
            bad = gens[:32 * pos] + e + gens[32 * pos + 32:]
            assert H.h_msm_shared(W, nsplit, ngen, bad, ngen, idv, 1, 0, GS[:32 * ngen], b"", b"", out, st, vd) == -5, (cls, pos)
    # every non-identity ACCEPT member as a generator
    acc = PC.ACCEPT_ENC[1:]
    g2 = b"".join(acc) + gens[32 * len(acc):]
    assert H.h_msm_shared(W, nsplit, ngen, g2, ngen, idv, 2, 0, GS[:64 * ngen], b"", b"", out, st, vd) == 0
    for b in range(2):
        assert st.raw[b] == 0 and out.raw[32 * b:32 * b + 32] == oracle.msm(GS[32 * ngen * b:32 * ngen * (b + 1)], g2)[1]


# ---- the range-proof decode role (rangeproof.h rp_points_thread) and the second-table role beside it ---------------------------
@pytest.mark.parametrize("form", ["64 lanes", "second tables", "four table levels"])
@pytest.mark.parametrize("n,m", [(8, 1), (8, 2)])
def test_members_at_every_point_position_of_a_range_proof(H, oracle, golden, n, m, form):
    """One mutated proof per (class, position) with valid proofs in between through the whole verification pipeline, lane by lane:
    verdict == oracle, the valid neighbours verify with a zero mega-check.  A verdict cannot show a wrong accept (the mega-check
    of a wrongly accepted point fails as well); the batch-combined pipeline can: a proof rejected by the decoder is left out of
    R, so valid proofs plus one mutated proof must combine to the identity."""
    case = [c for c in golden["cases"] if (c["n"], c["m"]) == (n, m)][0]
    pr, coms, label = bytes.fromhex(case["proof"]), golden["vc_bytes"][:32 * m], golden["label"]
    gg = oracle.Gens(n, m)
    G2, H2, B2, Bb2 = gg.export()
    gens = Bb2 + B2 + G2 + H2
    batch = PC.rp_mutants(pr, coms, n, m)
    rlc = [(name, p_, c_) for name, rej, p_, c_ in batch if rej and name.split()[0] in ("S", "L_1", "R_0", "V_%d" % (m - 1))]
    assert len(rlc) == 20
    H.h_set_horner_lanes(64)
    if form != "64 lanes":     # the narrow chain's forms: parked coefficients, split scalar role, second tables built by hw_ristretto_decode
        H.h_set_defer_emit(1)
        H.h_set_coop_split(1)
        H.h_set_narrow_hi(2 if form == "second tables" else 4)
    try:
        nb = len(batch)
        proofs, cc = b"".join(x[2] for x in batch), b"".join(x[3] for x in batch)
        rng = hashlib.shake_256(b"classes-host-%d-%d" % (n, m)).digest(64 * nb)
        vd, mo = C.create_string_buffer(nb), C.create_string_buffer(32 * nb)
        assert H.h_rp_verify(4, 3, n, m, gens, n, m, nb, proofs, len(pr), cc, label, len(label), rng, vd, mo) == 0
        for b, (name, rej, p_, c_) in enumerate(batch):
            erc, emsm = oracle.verify(gg, p_, c_, n, label, rng[64 * b:64 * b + 64])
            assert erc == (1 if rej else 0) and vd.raw[b] == erc, (form, name, vd.raw[b])
            if not rej:
                assert mo.raw[32 * b:32 * b + 32] == bytes(32) == emsm, (form, b)
        for k, (name, p_, c_) in enumerate(rlc):
            at = k % 4
            ps, cs = [pr] * at + [p_] + [pr] * (3 - at), [coms] * at + [c_] + [coms] * (3 - at)
            rng = hashlib.shake_256(b"classes-host-rlc-%d" % k).digest(64 * 4)
            wts = hashlib.shake_256(b"classes-host-wts-%d" % k).digest(64 * 4)
            vd, bo = C.create_string_buffer(4), C.create_string_buffer(33)
            assert H.h_rp_verify_rlc(4, 3, n, m, gens, n, m, 4, b"".join(ps), len(pr), b"".join(cs), label, len(label), rng, wts, vd, bo) == 0
            assert bo.raw == bytes(33), (form, name)                 # R = identity: the mutated proof is not in the combination
            assert list(vd.raw) == [1 if i == at else 0 for i in range(4)], (form, name, list(vd.raw))
    finally:
        H.h_set_horner_lanes(4)    # (the harness's default)
        H.h_set_defer_emit(0)
        H.h_set_coop_split(0)
        H.h_set_narrow_hi(0)


# ---- callers that report a status for a base that is in no transcript ------------------------------------------------------------
def test_members_as_bases_of_the_inner_product_and_linear_proof_front_ends(H, oracle):
    """InnerProductProof::verify takes P, Q, G, H from its caller and absorbs none of them: a member there must turn Ok into
    VerificationError by the decoder alone -- also the RIGHT point with bit 255 set, which a decoder without the canonical check
    accepts.  LinearProof::verify (C, G, F, B) and InnerProductProof::create (status BPGPU_MSM_BAD_POINT = 1) likewise."""
    label = b"innerproducttest"
    n = 4
    inst = oracle.ipp_test_instance(n, label, b"classes-host-ipp")
    pl = len(inst["proof"])
    names, variants = PC.ipp_verify_variants(inst, n)
    nb = len(variants)
    cat = lambda key: b"".join(v[key] for v in variants)
    vd, mo = C.create_string_buffer(nb), C.create_string_buffer(32 * nb)
    assert H.h_ipp_verify(n, nb, cat("proof"), pl, label, len(label), cat("Gf"), cat("Hf"), cat("P"), cat("Q"), cat("G"), cat("H"), vd, mo) == 0
    for j, (nm, x) in enumerate(zip(names, variants)):
        rc = oracle.ipp_verify(n, x["proof"], label, x["Gf"], x["Hf"], x["P"], x["Q"], x["G"], x["H"])[0]
        assert rc == (0 if nm == "valid" else 1) and vd.raw[j] == rc, (nm, vd.raw[j], rc)
    # InnerProductProof::create: a member among Q, G, H voids that proof alone
    a, b = b"".join(PC.scalars(n, b"host-create-a")), b"".join(PC.scalars(n, b"host-create-b"))
    rc, want = oracle.ipp_create(n, label, inst["Q"], inst["Hf"], inst["G"], inst["H"], a, b)
    assert rc == 0
    Q, G, Hh, expect = PC.ipp_create_cases(inst, n)
    nb = len(expect)
    cpl = len(want)
    out, st = C.create_string_buffer(cpl * nb), C.create_string_buffer(nb)
    assert H.h_ipp_create(n, nb, oracle.transcript_new(label), Q, inst["Gf"] * nb, inst["Hf"] * nb, G, Hh, 0, a * nb, b * nb, out, st) == 0
    assert list(st.raw) == expect
    for j in range(nb):
        if not expect[j]:
            assert out.raw[cpl * j:cpl * (j + 1)] == want, j
    # LinearProof::verify
    n = 16
    li = oracle.linear_test_instance(n, b"classes-host-linear")
    pl = len(li["proof"])
    st0 = oracle.transcript_new(li["label"])
    for nm, x in PC.linear_verify_cases(li, n):
        Cs = li["C"] + x["C"] + li["C"]
        vd = C.create_string_buffer(3)
        assert H.h_lin_verify(n, 3, li["proof"] * 3, pl, li["label"], len(li["label"]), Cs, x["G"], x["F"], x["B"], li["b"], 1, vd, None) == 0
        exp = [oracle.linear_verify(n, li["proof"], st0, Cs[32 * j:32 * j + 32], x["G"], x["F"], x["B"], li["b"])[0] for j in range(3)]
        assert list(vd.raw) == exp and exp[1] == (0 if nm == "valid" else 1), (nm, list(vd.raw), exp)


def test_members_as_commitments_of_an_audited_share(H, oracle):
    """ProofShare::audit_share (audit.h): a member of each class as V_j, A_j, S_j, T_1j or T_2j fails that share, and only it.  A
    member is another point, so such a share fails whatever the decoder decides; the decoder's own decision shows where the
    share's OWN commitments carry bit 255: no transcript absorbs them, a decoder without the canonical check would answer Ok."""
    cap, parties, n, m = 64, 4, 8, 2
    g = oracle.Gens(cap, parties)
    Gc, Hc, Bp, Bb = g.export()
    gens = Bb + Bp + Gc + Hc
    bl = b"".join(hashlib.shake_256(b"classes-host-aud-bl%d" % i).digest(31) + b"\x00" for i in range(m))
    r = oracle.prove_shares(g, [200, 17], bl, n, b"mpc audit", b"classes-host-audit")
    names, idx, sh, bc, pc = PC.audit_share_cases(r, n, m)
    ns = len(idx)
    vd = C.create_string_buffer(ns)
    assert H.h_audit_shares(n, ns, cap, parties, gens, (C.c_uint32 * ns)(*idx), b"".join(sh), b"".join(bc), b"".join(pc), r["challenges"], 1, vd, None) == 0
    for k, nm in enumerate(names):
        rc = oracle.audit_share(g, n, idx[k], sh[k], bc[k], pc[k], r["challenges"])[0]
        assert rc == (0 if nm == "valid" else 1) and vd.raw[k] == rc, (nm, vd.raw[k], rc)
