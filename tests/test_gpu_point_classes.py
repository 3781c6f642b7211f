"""Each rejection class of the ristretto255 decoder ALONE through the decode sites of the shipped code objects that answer with a
status: encodings that fail exactly one of RFC 9496's five checks -- C non-canonical (a valid encoding with bit 255 set), N
negative s, Q not a square, T negative t, Y y = 0 (s = p - 1) -- from tests/point_corpus.py, where the suite otherwise only
ever flips bit 0 (check N, decided before any field arithmetic).

  Straus prepare (msm_vb.h vb_prepare_thread)        msm_batch with bucket_min_terms out of reach, msm_narrow 0 / 1 (the narrow form
                                                     also builds second tables from the rejected bytes with hw_ristretto_decode),
                                                     the own points of msm_batch_shared, Pool.msm_batch
  fused bucket chain (bucket2.h, the _lp copy)       msm_batch, bucket_min_terms = 1, bucket_chain = 0, lanes 64 / 128 / 256, both tails
  old bucket chain (bucket.h)                        the same with bucket_chain = 1
  generator tables (msm_fixed.h fb_base_thread)      gens_load -> BPGPU_ERR_BAD_GENERATOR

Expected values: point_corpus.failed_checks, the twin and the C oracle -- never another form of the library.  One MSM per
rejected member (the member at a varying position among valid terms) with valid MSMs in between: status 1 and a zero encoding
for exactly the members' MSMs.  The valid ends of the range (s = 4 .. 30, p - 3 .. p - 21) and the hashed members go through
every form and every tail as 1 P (the member's own bytes come back) and P - P (zeros).  A decoded point always takes rotate = 0,
negate = 0 in the encoder: the taken branches of the tails' encoders are reached by the random sums of the valid MSMs and, in
the bucket forms, by the multiples of l stirred into the scalars (by name: the host encoder test).  The range-proof decode
role and the callers that report a status for a base are in test_gpu_point_classes_proofs.py."""
import hashlib

import pytest

import point_corpus as PC

pytestmark = pytest.mark.gpu

BAD_GENERATOR = -5   # include/bpgpu.h BPGPU_ERR_BAD_GENERATOR


@pytest.mark.parametrize("narrow", [0, 1])
def test_members_msm_batch_straus_and_narrow_forms(oracle, narrow):
    import bulletproofs_amd as bp
    c = bp.Context(0)
    c.set_option("msm_narrow", narrow)
    c.set_option("bucket_min_terms", 2**31 - 1)
    # the narrow form takes a few small MSMs per call (at most 16): the members go through it in calls of 15 MSMs, and a batch of all
    # of them takes the batch form whatever the option says
    na = len(PC.ACCEPT_ENC)
    for j, k in enumerate(range(0, len(PC.REJECT_ENC), 10)):   # (7 calls x 5 ACCEPT members: every member at least twice)
        PC.check_msm_form(c.msm_batch, oracle, 5, b"gpu-straus%d-%d" % (narrow, k), PC.REJECT_ENC[k:k + 10], [PC.ACCEPT_ENC[(5 * j + i) % na] for i in range(5)])
    PC.check_msm_form(c.msm_batch, oracle, 5, b"gpu-straus%d" % narrow)
    c.close()


def test_members_every_bucket_form(oracle):
    import bulletproofs_amd as bp
    c = bp.Context(0)
    c.set_option("msm_narrow", 0)
    c.set_option("bucket_min_terms", 1)
    for chain in (0, 1):
        for lanes in (64, 128, 256):
            for tail in (0, 1):
                c.set_option("bucket_chain", chain)
                c.set_option("bucket_lanes", lanes)
                c.set_option("bucket_fast_tail", tail)
                PC.check_msm_form(c.msm_batch, oracle, 6, b"gpu-bucket%d-%d-%d" % (chain, lanes, tail))
                # a narrow batch (fewer MSMs than the fast tail's limit): one member of each class
                PC.check_msm_form(c.msm_batch, oracle, 6, b"gpu-bucket-few%d-%d-%d" % (chain, lanes, tail), [e for _, e in PC.one_per_class()], PC.ACCEPT_ENC[8:])
    c.close()


def test_members_pool_msm_batch(oracle):
    import bulletproofs_amd as bp
    pool = bp.Pool((0,), 2)
    PC.check_msm_form(pool.msm_batch, oracle, 5, b"gpu-pool")
    pool.close()


def _gens(oracle, n, m):
    G, H, B, Bb = oracle.Gens(n, m).export()
    return G, H, B, Bb


@pytest.mark.parametrize("W", [5, 17])
def test_members_among_the_own_points_of_msm_batch_shared(oracle, W):
    import bulletproofs_amd as bp
    n, m = 8, 1
    ngen = 2 * n * m + 2
    G, H, B, Bb = _gens(oracle, n, m)
    gen_pts = Bb + B + G + H
    nu = 5
    US, UP, flags = PC.reject_batch(nu, b"gpu-shared%d" % W)
    nb = len(flags)
    GS = b"".join(PC.scalars(ngen * nb, b"gpu-shared-g%d" % W))
    for fork in (0, 1):
        c = bp.Context(0, fixed_window_bits=W)
        c.set_option("msm_fork", fork)
        c.gens_load(n, m, G, H, B, Bb)
        out, st = c.msm_batch_shared(n, m, nb, nu, GS, US, UP)
        for b, rej in enumerate(flags):
            if rej:
                assert st[b] == 1 and out[32 * b:32 * b + 32] == bytes(32), (W, fork, b)
            else:
                exp = oracle.msm(GS[32 * ngen * b:32 * ngen * (b + 1)] + US[32 * nu * b:32 * nu * (b + 1)], gen_pts + UP[32 * nu * b:32 * nu * (b + 1)])
                assert exp[0] == 0 and st[b] == 0 and out[32 * b:32 * b + 32] == exp[1], (W, fork, b)
        # a few MSMs (the narrow form: second tables from the same bytes, the lane role decides): one member of each class
        us, up, fl = PC.reject_batch(nu, b"gpu-shared-few%d" % W, [e for _, e in PC.one_per_class()])
        assert len(fl) <= 16
        out, st = c.msm_batch_shared(n, m, len(fl), nu, GS[:32 * ngen * len(fl)], us, up)
        for b, rej in enumerate(fl):
            if rej:
                assert st[b] == 1 and out[32 * b:32 * b + 32] == bytes(32), (W, fork, "few", b)
            else:
                exp = oracle.msm(GS[32 * ngen * b:32 * ngen * (b + 1)] + us[32 * nu * b:32 * nu * (b + 1)], gen_pts + up[32 * nu * b:32 * nu * (b + 1)])
                assert exp[0] == 0 and st[b] == 0 and out[32 * b:32 * b + 32] == exp[1], (W, fork, "few", b)
        c.close()


def test_gens_load_refuses_a_member_of_each_class_and_leaves_the_context_good(oracle, golden):
    """One member of each class in turn as G[0], G[last], one H, B and B_blinding: BPGPU_ERR_BAD_GENERATOR; afterwards the proper
    generators load into the same context and a golden proof verifies on it."""
    import bulletproofs_amd as bp
    n, m = 8, 2
    G, H, B, Bb = _gens(oracle, n, m)
    case = [c_ for c_ in golden["cases"] if (c_["n"], c_["m"]) == (n, m)][0]
    pr = bytes.fromhex(case["proof"])
    c = bp.Context(0)
    L_ = c._L
    tot = n * m

    put = PC.put
    for cls, e in PC.one_per_class():
        assert PC.failed_checks(e) == frozenset(cls)
        variants = [("G[0]", put(G, 0, e), H, B, Bb), ("G[last]", put(G, tot - 1, e), H, B, Bb), ("H[5]", G, put(H, 5, e), B, Bb),
                    ("B", G, H, e, Bb), ("B_blinding", G, H, B, e)]
        for name, g_, h_, b_, bb_ in variants:
            assert L_.bpgpu_gens_load(c.h, n, m, g_, h_, b_, bb_) == BAD_GENERATOR, (cls, name)
            with pytest.raises(bp.BpgpuError, match="BAD_GENERATOR"):
                c.gens_load(n, m, g_, h_, b_, bb_)
        c.gens_load(n, m, G, H, B, Bb)
        assert c.gens_export() == (G, H, B, Bb)
        v, enc = c.rangeproof_verify_batch(n, m, pr, len(pr), golden["vc_bytes"][:32 * m], golden["label"], hashlib.shake_256(b"classes-gens-" + cls.encode()).digest(64), want_msm=True)
        assert v == bytes(1) and enc == bytes(32), cls
    c.close()


def test_every_valid_end_of_the_range_as_a_generator(oracle):
    """Every non-identity ACCEPT member as a generator (G of an (8, 2) set): msm_batch_shared == oracle."""
    import bulletproofs_amd as bp
    n, m = 8, 2
    ngen = 2 * n * m + 2
    G, H, B, Bb = _gens(oracle, n, m)
    acc = PC.ACCEPT_ENC[1:]
    assert len(acc) == 16 and all(not PC.failed_checks(e) for e in acc)
    G2 = b"".join(acc)
    c = bp.Context(0)
    c.gens_load(n, m, G2, H, acc[3], acc[-1])
    nb = 3
    GS = b"".join(PC.scalars(ngen * nb, b"gpu-accept-gens"))
    out, st = c.msm_batch_shared(n, m, nb, 0, GS, b"", b"")
    pts = acc[-1] + acc[3] + G2 + H
    for b in range(nb):
        exp = oracle.msm(GS[32 * ngen * b:32 * ngen * (b + 1)], pts)
        assert exp[0] == 0 and st[b] == 0 and out[32 * b:32 * b + 32] == exp[1], b
    c.close()
