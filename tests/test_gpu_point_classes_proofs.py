"""Each rejection class of the ristretto255 decoder ALONE (tests/point_corpus.py: C a valid encoding with bit 255 set, N negative s,
Q not a square, T negative t, Y y = 0) at every point of a range proof, and at the bases of the callers that report a status for a
point that is in no transcript.

Range proofs.  One mutated proof per (class, position) for EVERY point position -- A, S, T_1, T_2, every L_j and R_j, every V_j --
of the golden shapes (8, 1), (8, 2), (64, 1), in batches of 1, 2, 5 and 33 with valid proofs in between, on four forms of the launch
chain (round 5's, the rebuilt one without second tables, with second tables, with four table levels: the second-table role,
hw_ristretto_decode, then builds its tables from every class, t = 0 and y = 0 included, next to valid proofs).  Against
oracle.verify_ts: the verdict, the transcript handed back (an undecodable non-identity point is absorbed and found after the whole
replay), the valid neighbours' verdicts 0 and mega-check encodings zero; all forms equal each other.

WHAT A VERDICT CANNOT SHOW: a point that is wrongly ACCEPTED still ends in VerificationError, because the mega-check then fails (for
class C the transcript absorbed other bytes than the prover's; for the others the point is not the prover's).  The accept / reject
DECISION of the range-proof decode role (rangeproof.h rp_points_thread) shows in the batch-combined check: a proof rejected by the
decoder is left out of R = sum rho_i MegaCheck_i, so a batch of valid proofs plus one mutated proof must hand back batch_out =
00 + compress(identity); a wrongly accepted point would put its failing proof into R.

Callers whose bases are in no transcript (a missing check is a WRONG ACCEPT there, visible in the status alone), and the decode
site each reaches:
  ipp_verify_batch (P, Q, G_i, H_i)              Straus prepare (msm_vb.h) -- one MSM of 2n + 2 lg n + 2 terms per proof
  linear_verify_batch (C, G_i, F, B)             Straus prepare; the bases ARE absorbed by the transcript here
  rangeproof_audit_shares (V_j, A_j, S_j, T_1j, T_2j)   Straus prepare (two MSMs per share); in no transcript either
  ipp_create_batch / linear_create_batch (G, H, Q / G, F, B)   Straus prepare of the provers' MSMs
  R1CS verify (V, proof points)                  fused bucket chain (bucket2.h, the _lp copy) from bucket_min_terms on, else Straus
  R1CS verify_batch_combined (proof point)       falls back to the per-proof path: the same sites
For ipp_verify_batch and rangeproof_audit_shares a VALID encoding of the right point with bit 255 set turns Ok into VerificationError: the canonical check is
the only thing between that input and a wrong accept."""
import hashlib

import pytest

import point_corpus as PC

pytestmark = pytest.mark.gpu

TS = 208
SHAPES = [(8, 1), (8, 2), (64, 1)]
CHAIN_FORMS = [   # four of test_gpu_narrow_chain.py's FORMS
    {"coop_split": 0, "exp_single": 0, "narrow_chunk": 32, "narrow_walk": 0, "narrow_hi_max": 0},   # round 5's chain
    {"narrow_hi_max": 0},                      # the rebuilt chain, no second tables
    {"narrow_hi_max": 256},                    # second tables (2^128 multiples) for every batch size used here
    {"narrow_hi4_max": 256},                   # four table levels up to 32 proofs, two above
]


def _case(golden, n, m):
    c = [c_ for c_ in golden["cases"] if (c_["n"], c_["m"]) == (n, m)][0]
    return bytes.fromhex(c["proof"]), golden["vc_bytes"][:32 * m]


@pytest.fixture
def chain_contexts():
    """four (64, 8) contexts, one per form, alive for one test only"""
    import bulletproofs_amd as bp
    out = []
    for f in CHAIN_FORMS:
        c = bp.Context(0)
        for k, v in f.items():
            c.set_option(k, v)
        c.gens_create(64, 8)
        out.append(c)
    yield out
    for c in out:
        c.close()


@pytest.mark.parametrize("n,m", SHAPES)
def test_every_class_at_every_point_position_verdict_and_transcript(chain_contexts, oracle, oracle_gens_64_8, golden, n, m):
    pr, coms = _case(golden, n, m)
    label = golden["label"]
    st0 = oracle.transcript_new(label)
    seq = [(name, p_, c_) for name, _, p_, c_ in PC.rp_mutants(pr, coms, n, m)]
    sizes, at, b = (1, 2, 5, 33), 0, 0
    seen_sizes = set()
    while at < len(seq):
        nb = min(sizes[b % 4], len(seq) - at)
        if b >= 4 and nb not in sizes:           # the tail: pad with valid proofs to a size of the matrix
            want = min(s for s in sizes if s >= nb)
            seq += [("valid", pr, coms)] * (want - nb)
            nb = want
        batch = seq[at:at + nb]
        at, b = at + nb, b + 1
        seen_sizes.add(nb)
        proofs, cc = b"".join(x[1] for x in batch), b"".join(x[2] for x in batch)
        rng = hashlib.shake_256(b"classes-%d-%d-%d" % (n, m, b)).digest(64 * nb)
        exp = [oracle.verify_ts(oracle_gens_64_8, batch[i][1], batch[i][2], n, st0, rng[64 * i:64 * i + 64]) for i in range(nb)]
        res = [c.rangeproof_verify_batch_ts(n, m, proofs, len(pr), cc, st0, rng, want_msm=True, want_transcripts=True) for c in chain_contexts]
        for f, r in zip(CHAIN_FORMS[1:], res[1:]):
            assert r == res[0], (n, m, b, f)
        v, enc, ts = res[0]
        for i, (name, _, _) in enumerate(batch):
            rc, eenc, ets = exp[i]
            assert v[i] == rc and ts[TS * i:TS * (i + 1)] == ets, (n, m, b, name, v[i], rc)
            if name == "valid":
                assert rc == 0 and enc[32 * i:32 * i + 32] == bytes(32) == eenc, (n, m, b, i)
            else:
                assert rc == 1, (n, m, b, name)
                assert ets != st0                 # (absorbed: found after the replay, not at the point's own message)
    assert seen_sizes == set(sizes)


@pytest.mark.parametrize("variant", ["lookup", "bucket"])
def test_batch_combined_check_leaves_every_rejected_point_out_of_the_combination(oracle, oracle_gens_64_8, golden, variant):
    """batch_out == 00 + compress(identity) for valid proofs plus ONE mutated proof, per (class, position class): the decision of
    the range-proof decode role itself.  Verdicts == the per-proof entry point == the oracle."""
    import bulletproofs_amd as bp
    c = bp.Context(0)
    c.set_option("bucket_min_terms", 1 if variant == "bucket" else 2**31 - 1)
    c.gens_create(64, 8)
    label = golden["label"]
    for n, m in SHAPES:
        pr, coms = _case(golden, n, m)
        pos = PC.rp_positions(n, m)
        picks = [pos[1], [p for p in pos if p[1] == "L"][-1], [p for p in pos if p[1] == "R"][0], [p for p in pos if p[1] == "V"][-1]]
        picks += [pos[0], pos[2], pos[3]]          # (A, T_1, T_2 as well: they cost a call each)
        for k, (name, _, where, off) in enumerate(picks):
            for cls, e in PC.one_per_class():
                mp, mc = PC.rp_mutate(pr, coms, where, off, e)
                at = (k + "CNQTY".index(cls)) % 5
                batch = [(pr, coms)] * at + [(mp, mc)] + [(pr, coms)] * (4 - at)
                nb = len(batch)
                proofs, cc = b"".join(x[0] for x in batch), b"".join(x[1] for x in batch)
                rng = hashlib.shake_256(b"classes-rlc-%d-%d-%s" % (n, m, name.encode())).digest(64 * nb)
                wts = hashlib.shake_256(b"classes-wts-%d-%d-%s" % (n, m, name.encode())).digest(64 * nb)
                verdict, ok, enc = c.rangeproof_verify_rlc(n, m, proofs, len(pr), cc, label, rng, wts)
                assert ok and enc == bytes(32), (variant, n, m, name, cls)
                assert list(verdict) == [1 if i == at else 0 for i in range(nb)], (variant, n, m, name, cls)
                assert verdict == c.rangeproof_verify_batch(n, m, proofs, len(pr), cc, label, rng)
                assert oracle.verify(oracle_gens_64_8, mp, mc, n, label, rng[64 * at:64 * at + 64])[0] == 1
    c.close()


def test_pool_combined_form_leaves_every_rejected_point_out_of_the_combination(golden):
    """bpgpu_pool_rangeproof_submit_rlc_dev: the same batches through the pool's combining queue (device pointers): every chain's
    batch_out is 00 + the identity, the mutated proof alone carries VerificationError."""
    import torch
    import bulletproofs_amd as bp
    dev = torch.device("cuda", 0)
    pool = bp.Pool((0,), 4)
    pool.gens_create(64, 8)
    label = golden["label"]
    to_dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    for n, m in SHAPES:
        pr, coms = _case(golden, n, m)
        pos = PC.rp_positions(n, m)
        picks = [pos[1], [p for p in pos if p[1] == "L"][0], [p for p in pos if p[1] == "R"][-1], [p for p in pos if p[1] == "V"][0]]
        jobs = []
        for k, (name, _, where, off) in enumerate(picks):
            for cls, e in PC.one_per_class():
                mp, mc = PC.rp_mutate(pr, coms, where, off, e)
                at = (k + 2 * "CNQTY".index(cls)) % 6
                batch = [(pr, coms)] * at + [(mp, mc)] + [(pr, coms)] * (5 - at)
                jobs.append((at, b"".join(x[0] for x in batch), b"".join(x[1] for x in batch)))
        nb = 6
        d_p, d_c = to_dev(b"".join(j[1] for j in jobs)), to_dev(b"".join(j[2] for j in jobs))
        d_r = to_dev(hashlib.shake_256(b"classes-pool-%d-%d" % (n, m)).digest(64 * nb * len(jobs)))
        d_v = torch.full((nb * len(jobs),), 255, dtype=torch.uint8, device=dev)
        d_b = torch.full((len(jobs), 36), 255, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        tickets = []
        for i in range(len(jobs)):
            tickets.append(pool.submit_rlc_dev(0, n, m, nb, d_p.data_ptr() + i * nb * len(pr), len(pr), d_c.data_ptr() + i * nb * 32 * m, label,
                                               d_r.data_ptr() + i * nb * 64, d_v.data_ptr() + i * nb, d_b[i].data_ptr(), want_ticket=True))
        for t in tickets:
            t.wait()
        v, b = bytes(d_v.cpu().numpy()), d_b.cpu().numpy()
        for i, (at, _, _) in enumerate(jobs):
            assert bytes(b[i][:33]) == bytes(33), (n, m, i)
            assert list(v[nb * i:nb * i + nb]) == [1 if j == at else 0 for j in range(nb)], (n, m, i)
    pool.close()


# ---- callers that report a status for a base that is in no transcript -------------------------------------------------------------
def test_ipp_verify_batch_bases(oracle):
    import bulletproofs_amd as bp
    ctx = bp.Context(0)
    label = b"innerproducttest"
    for n in (4, 32):
        inst = oracle.ipp_test_instance(n, label, b"classes-ipp-%d" % n)
        pl = len(inst["proof"])
        names, variants = PC.ipp_verify_variants(inst, n)
        cat = lambda key: b"".join(i[key] for i in variants)
        verdict = ctx.ipp_verify_batch(n, cat("proof"), pl, label, cat("Gf"), cat("Hf"), cat("P"), cat("Q"), cat("G"), cat("H"))
        for j, (nm, x) in enumerate(zip(names, variants)):
            rc = oracle.ipp_verify(n, x["proof"], label, x["Gf"], x["Hf"], x["P"], x["Q"], x["G"], x["H"])[0]
            assert rc == (0 if nm == "valid" else 1), (n, nm, rc)
            assert verdict[j] == rc, (n, nm, verdict[j])
    ctx.close()


def test_linear_verify_batch_bases(oracle):
    import bulletproofs_amd as bp
    ctx = bp.Context(0)
    n = 16
    inst = oracle.linear_test_instance(n, b"classes-linear")
    pl = len(inst["proof"])
    st = oracle.transcript_new(inst["label"])
    cases = PC.linear_verify_cases(inst, n)
    for nm, x in cases:   # G, F, B are shared by a batch: one call per case, the valid proof beside it where C is the member
        nb = 3
        Cs = inst["C"] + x["C"] + inst["C"]
        verdict = ctx.linear_verify_batch(n, inst["proof"] * nb, pl, Cs, x["G"], x["F"], x["B"], inst["b"], label=inst["label"])
        exp = [oracle.linear_verify(n, inst["proof"], st, Cs[32 * j:32 * j + 32], x["G"], x["F"], x["B"], inst["b"])[0] for j in range(nb)]
        assert list(verdict) == exp, (nm, list(verdict), exp)
        assert exp[1] == (0 if nm == "valid" else 1), (nm, exp)
        if nm.endswith(" C"):
            assert exp == [0, 1, 0], nm
    ctx.close()


def test_audit_shares_commitments(oracle):
    """A member of each class as V_j, A_j, S_j, T_1j, T_2j fails that share (another point: it fails whatever the decoder decides);
    the share's OWN commitments with bit 255 set must fail it too -- no transcript absorbs them, so there the verdict is the
    decoder's canonical check and nothing else."""
    import bulletproofs_amd as bp
    ctx = bp.Context(0)
    ctx.gens_create(64, 4)
    g = oracle.Gens(64, 4)
    n, m = 8, 2
    bl = b"".join(hashlib.shake_256(b"classes-aud-bl%d" % i).digest(31) + b"\x00" for i in range(m))
    r = oracle.prove_shares(g, [200, 17], bl, n, b"mpc audit", b"classes-audit")
    names, idx, sh, bc, pc = PC.audit_share_cases(r, n, m)
    verdict = ctx.rangeproof_audit_shares(n, idx, b"".join(sh), b"".join(bc), b"".join(pc), r["challenges"])
    for k, nm in enumerate(names):
        rc = oracle.audit_share(g, n, idx[k], sh[k], bc[k], pc[k], r["challenges"])[0]
        assert verdict[k] == rc, (nm, verdict[k], rc)
        assert rc == (0 if nm == "valid" else 1), nm
    ctx.close()


def test_provers_bases(oracle):
    """ipp_create_batch / linear_create_batch: a member among the bases voids that proof alone (status BPGPU_MSM_BAD_POINT)."""
    import bulletproofs_amd as bp
    ctx = bp.Context(0)
    n = 8
    label = b"innerproducttest"
    inst = oracle.ipp_test_instance(n, label, b"classes-create")
    a = b"".join(PC.scalars(n, b"create-a"))
    b = b"".join(PC.scalars(n, b"create-b"))
    rc, want = oracle.ipp_create(n, label, inst["Q"], inst["Hf"], inst["G"], inst["H"], a, b)
    assert rc == 0
    pl = len(want)
    Q, G, H, expect = PC.ipp_create_cases(inst, n)
    nb = len(expect)
    proofs, st = ctx.ipp_create_batch(n, Q, inst["Gf"] * nb, inst["Hf"] * nb, G, H, a * nb, b * nb, label=label)
    assert list(st) == expect
    for j in range(nb):
        if not expect[j]:
            assert proofs[pl * j:pl * (j + 1)] == want, j
    # LinearProof::create: G, F, B are shared by a batch -- one call per case
    n = 16
    li = oracle.linear_test_instance(n, b"classes-lcreate")
    made, st = ctx.linear_create_batch(n, li["C"], li["r"], li["a"], li["b"], li["G"], li["F"], li["B"], label=li["label"], rng=li["rng"])
    assert list(st) == [0] and made == li["proof"]
    for k, (cls, e) in enumerate(PC.one_per_class()):
        for nm, x in (("G", dict(li, G=PC.put(li["G"], (5 * k + 1) % n, e))), ("F", dict(li, F=e)), ("B", dict(li, B=e))):
            made, st = ctx.linear_create_batch(n, li["C"], li["r"], li["a"], li["b"], x["G"], x["F"], x["B"], label=li["label"], rng=li["rng"])
            assert list(st) == [1], (cls, nm, list(st))
    made, st = ctx.linear_create_batch(n, li["C"], li["r"], li["a"], li["b"], li["G"], li["F"], li["B"], label=li["label"], rng=li["rng"])
    assert list(st) == [0] and made == li["proof"]
    ctx.close()


def test_r1cs_verify_and_combined_verify_commitments_and_proof_points(oracle):
    """An R1CS verify (a k = 4 shuffle: 8 commitments, 11 proof points, 3 rounds of L_j / R_j) with a member as a V, as a proof point
    and as an L_j / R_j: verdict, mega-check and transcript == the twin.  verify_batch_combined with a member as a proof point falls
    back: verdicts and transcripts == the per-proof path == the twin."""
    import random
    import bulletproofs_amd as bp
    from bulletproofs_amd import r1cs
    import r1cs_twin as R
    from test_gpu_r1cs import CAP, _check, _record, _shuffle_gadget
    gens = oracle.Gens(CAP, 1).export()
    k = 4
    rnd = random.Random(4004)
    inp = [rnd.getrandbits(64) for _ in range(k)]
    outp = inp[:]
    rnd.shuffle(outp)
    pf, Vs, st0 = R.prove_shuffle(gens, CAP, b"ShuffleProofTest", inp, outp, b"classes-shuffle")
    good = pf.to_bytes()
    coms = b"".join(Vs)
    assert good[0] == 1 and len(Vs) == 2 * k                       # two-phase: 11 points, t_x, t_x_blinding, e_blinding, then the IPP
    npts, ipp = 11, 1 + 32 * 14
    rounds = (len(good) - ipp - 64) // 64
    assert rounds == 3
    gadget = _shuffle_gadget(k)
    for bucket_min in (None, 1):        # the default chain for this size, and the fused bucket chain's short-register decoder
        c = bp.Context(0)
        if bucket_min is not None:
            c.set_option("bucket_min_terms", bucket_min)
        c.gens_create(CAP, 1)
        circuit = _record(gadget, 2 * k, st0)
        proofs, cc = [good], [coms]
        for j, (cls, e) in enumerate(PC.one_per_class()):
            proofs.append(good); cc.append(PC.put(coms, (3 * j + 1) % (2 * k), e))            # a V
            el = (2 * j + 1) % npts                                                         # one of the 11 proof points (A_I1 .. T_6)
            proofs.append(good[:1 + 32 * el] + e + good[1 + 32 * (el + 1):]); cc.append(coms)
            o = ipp + 32 * (j % (2 * rounds))                                               # an L_j / R_j
            proofs.append(good[:o] + e + good[o + 32:]); cc.append(coms)
        proofs.append(good); cc.append(coms)
        nb = len(proofs)
        rng = hashlib.shake_256(b"classes-r1cs-rng").digest(32 * nb)
        v = _check(c, circuit, gadget, gens, CAP, proofs, cc, [st0] * nb, rng)
        assert list(v) == [0] + [1] * (nb - 2) + [0]
        # the combined check: two valid proofs and one with a member as a proof point, per class
        for j, (cls, e) in enumerate(PC.one_per_class()):
            el = (3 * j + 2) % npts
            bad = good[:1 + 32 * el] + e + good[1 + 32 * (el + 1):]
            ps = [good, bad, good]
            w = hashlib.shake_256(b"classes-r1cs-w%d" % j).digest(64 * 3)
            vv, batch, ts = r1cs.verify_batch_combined(c, [(circuit, ps, coms * 3, st0 * 3)], rng32=rng[:96], weights64=w, want_batch=True, want_transcripts=True)
            pv, pts = circuit.verify_batch(c, ps, coms * 3, st0 * 3, rng32=rng[:96], want_transcripts=True)
            assert list(vv) == [0, 1, 0] and (vv, ts) == (pv, pts), (cls, list(vv))
            assert batch == b"\x01" + bytes(32), cls
            for b_ in range(3):
                code, _, ets = R.verify_with(gadget, gens, CAP, st0, ps[b_], Vs, rng[32 * b_:32 * b_ + 32])
                assert vv[b_] == code and ts[TS * b_:TS * b_ + TS] == ets, (cls, b_)
        c.close()
