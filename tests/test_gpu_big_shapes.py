"""Range proofs of 32 to 1024 parties on every verification path (big_shapes.py lists the shapes and the branch of launch 1,
k_rp_stage1_coop, each is there for; test_big_shapes_on_cpu.py asserts that they still lie there).  Every assertion is verdict bytes and,
where the oracle produced one, the 32-byte mega-check encoding, against the oracle on the same rng bytes.

Window tables: fixed_window_bits = 4 for the (64, 128) and (8, 1024) generator sets (16386 generators x 64 windows x 8 entries x 128 B =
1.0 GiB each, shared by the contexts of the process) and 2 for (64, 1024) (131074 x 128 x 2 x 128 B = 4.0 GiB)."""
import hashlib
import threading

import pytest

import big_shapes as B
from rlc_ts_cases import L

pytestmark = pytest.mark.gpu
W = 4


def _context(options=(), capacity=(64, 128), window_bits=W):
    import bulletproofs_amd as bp
    c = bp.Context(0, fixed_window_bits=window_bits)
    for k, v in dict(options).items():
        c.set_option(k, v)
        assert c.get_option(k) == v, (k, v)          # the option took
    c.gens_create(*capacity)
    return c


@pytest.fixture(scope="module")
def ctx():
    c = _context()
    yield c
    c.close()


def _encodings_equal(got, want):
    """the mega-check encodings are the oracle's wherever it produced one (0xff x 32: a point did not decode, there is no sum)"""
    assert len(got) == len(want)
    return all(want[o:o + 32] in (got[o:o + 32], b"\xff" * 32) for o in range(0, len(want), 32))


def _check(c, n, m, nb, tag, also_verdict_only=True, batch=None, label=B.LABEL):
    """nb tiled proofs through rangeproof_verify_batch on context c: verdicts and encodings are the oracle's"""
    proofs, coms = batch or B.batch(n, m, nb)
    rng = B.rng64(b"%s-%d-%d-%d" % (tag, n, m, nb), nb)
    got = c.rangeproof_verify_batch(n, m, proofs, B.O.proof_len(n, m), coms, label, rng, want_msm=True)
    ev, em = B.expected(n, m, proofs, coms, rng, label)
    assert got[0] == ev, (tag, n, m, nb, list(got[0]), list(ev))
    assert _encodings_equal(got[1], em), (tag, n, m, nb)
    if also_verdict_only:   # the crate's call: no encodings wanted (narrow chains then finish inside launch 4)
        assert bytes(c.rangeproof_verify_batch(n, m, proofs, B.O.proof_len(n, m), coms, label, rng)) == ev, (tag, n, m, nb)
    return got


# ---- narrow chains, defaults ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [s for s in B.SHAPES if s != (64, 1024)])
def test_narrow_chains_with_default_options(ctx, n, m):
    """1, 2, 3: an idle second group in the last workgroup of launch 1; 4 / 5: last chain with four table levels, first with two;
    narrow_hi_max + 1: first 64-window chain; 65; 256 / 257: last 32-lanes-per-proof launch, first lane-per-proof one"""
    c = ctx if m <= 128 else _context(capacity=(n, m))
    try:
        hi = c.get_option("narrow_hi_max")
        assert hi == 32 and c.get_option("narrow_hi4_max") == 4 and c.get_option("transcript_coop") == 1 and c.get_option("coop_split") == 1
        assert c.get_option("coop_defer_emit") == 1 and c.get_option("split_stage3") == -1
        sizes = [1, 2, 3, 4, 5, hi + 1, 65, 256, 257]
        if m == 1024:
            sizes = sizes[:6]
        seen = set()
        for nb in sizes:
            v, _ = _check(c, n, m, nb, b"narrow")
            seen |= set(v)
        assert seen == {0, 1, 2}
    finally:
        if c is not ctx:
            c.close()


# ---- every launch-1 option on both sides of each capacity ------------------------------------------------------------------------
OPTIONS = [("coop_defer_emit", 0), ("coop_defer_emit", 1), ("coop_split", 0), ("coop_split", 1), ("transcript_coop", 0), ("transcript_coop", 1),
           ("transcript_script", 0), ("transcript_script", 1), ("narrow_hi_max", 0), ("narrow_hi_max", 256), ("narrow_hi4_max", 256),
           ("narrow_fused_finish", 0)]


@pytest.fixture(scope="module")
def option_contexts():
    out = [_context([o]) for o in OPTIONS]
    yield out
    for c in out:
        c.close()


@pytest.mark.parametrize("n,m", [B.CONTROL, (16, 32), (32, 32), (8, 64), (8, 128)])
def test_every_launch_1_option_alone_against_the_default(ctx, option_contexts, n, m):
    pl = B.O.proof_len(n, m)
    for nb in (3, 40):
        proofs, coms = B.batch(n, m, nb)
        rng = B.rng64(b"opt-%d-%d-%d" % (n, m, nb), nb)
        ref = ctx.rangeproof_verify_batch(n, m, proofs, pl, coms, B.LABEL, rng, want_msm=True)
        ev, em = B.expected(n, m, proofs, coms, rng)
        assert ref[0] == ev and _encodings_equal(ref[1], em), (n, m, nb)
        for o, c in zip(OPTIONS, option_contexts):
            assert c.rangeproof_verify_batch(n, m, proofs, pl, coms, B.LABEL, rng, want_msm=True) == ref, (n, m, nb, o)
            assert bytes(c.rangeproof_verify_batch(n, m, proofs, pl, coms, B.LABEL, rng)) == ev, (n, m, nb, o)


# ---- callers' own transcripts -----------------------------------------------------------------------------------------------------
def _on_states(n, m, states):
    """proof i made on states[i]; the third one with a wrong t_x, the fifth one malformed"""
    proofs, coms = [], []
    for i, st in enumerate(states):
        pr, cm, _ = B.proof_on(n, m, i % 3, st)
        if i == 2:
            pr = B.tamper(n, m, pr, cm)["t_x"][0]
        if i == 4:
            pr = B.tamper(n, m, pr, cm)["t_x_blinding_noncanonical"][0]
        proofs.append(pr)
        coms.append(cm)
    return b"".join(proofs), b"".join(coms)


@pytest.mark.parametrize("n,m", B.TS_SHAPES)
def test_callers_own_transcripts(ctx, n, m):
    """one shared bound state; one state per proof at one STROBE position -- at the two positions where a (32, 32) script has
    RP_COOP_MASKS_CAP masks and one more; states at differing positions (byte-wise replay).  Verdicts, encodings and returned states are
    oracle.verify_ts's; the malformed proof gets its state back untouched."""
    pl, nb = B.O.proof_len(n, m), 6
    lo, hi = B.session_lengths_32_32()
    shared = B.padded_state([60])
    cases = [("shared", [shared] * nb)]
    cases += [("uniform-%d" % ln, [B.session_state(i, ln) for i in range(nb)]) for ln in (lo, hi)]
    cases += [("differing", [B.session_state(i, 3 + 29 * i) for i in range(nb)])]
    for name, states in cases:
        proofs, coms = _on_states(n, m, states)
        rng = B.rng64(b"ts-%d-%d-%s" % (n, m, name.encode()), nb)
        arg = shared if name == "shared" else b"".join(states)
        got = ctx.rangeproof_verify_batch_ts(n, m, proofs, pl, coms, arg, rng, want_msm=True, want_transcripts=True)
        ev, em, et = B.expected_ts(n, m, proofs, coms, b"".join(states), rng)
        assert list(ev) == [0, 0, 1, 0, 2, 0], name
        assert got[0] == ev and _encodings_equal(got[1], em), (n, m, name, list(got[0]))
        assert got[2] == et, (n, m, name)
        assert got[2][208 * 4:208 * 5] == states[4], (n, m, name)
        if name != "shared" and name != "differing":
            assert len({s[200:203] for s in states}) == 1 and len({s[:200] for s in states}) == nb


# ---- wide forms without thousands of proofs ---------------------------------------------------------------------------------------
WIDE = [{"horner_lanes": 0}, {"horner_lanes": 1, "a_outside": 0}, {"horner_lanes": 1, "a_outside": 1}, {"horner_lanes": 4}, {"horner_lanes": 64},
        {"horner_lanes": 0, "exponent_pairs": 0}, {"horner_lanes": 1, "exponent_pairs": 0}, {"horner_lanes": 1, "per_proof_radix": 32}]


@pytest.mark.parametrize("n,m", [(8, 64), (8, 128)])
def test_wide_chain_forms_on_300_proofs(n, m):
    """split_stage3 = 1 makes a chain of 300 proofs take the wide forms: window sums as a launch of their own, the Horner chain on 64, 4
    or one lane (the one-lane chain with A outside or not, in radix 32), the generator exponents in mirrored pairs or not"""
    nb = 300
    batch = B.batch(n, m, nb)
    ref = None
    for f in WIDE:
        c = _context(dict(f, split_stage3=1))
        try:
            got = _check(c, n, m, nb, b"wide", also_verdict_only=False, batch=batch)
        finally:
            c.close()
        ref = ref or got
        assert got == ref, f


def test_the_chain_above_2048_proofs_with_split_stage3_off():
    n, m, nb = 8, 64, 2100
    c = _context({"split_stage3": 0})
    try:
        v, _ = _check(c, n, m, nb, b"nowide", also_verdict_only=False)
        assert set(v) == {0, 1, 2}
    finally:
        c.close()


# ---- explicit splits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [1, 3, 8, 65, 4096])
def test_explicit_splits(splits, golden):
    """the partition of the (generator, window) pairs over the splits of the table walk, with split counts that are no multiple of 8.
    (Chains of up to 256 proofs round the count to whole wavefronts; the chain of 260 takes it as given.)"""
    c = _context({"fixed_splits": splits})
    try:
        case = [q for q in golden["cases"] if q["n"] == 64 and q["m"] == 1][0]
        pr = bytes.fromhex(case["proof"])
        bad = bytearray(pr)
        bad[128] ^= 1
        for nb in (5, 130, 260):
            proofs = b"".join(bytes(bad) if i % 5 == 2 else pr for i in range(nb))
            _check(c, 64, 1, nb, b"splits%d" % splits, batch=(proofs, golden["vc_bytes"][:32] * nb), label=golden["label"])
            _check(c, 8, 64, nb, b"splits%d" % splits)
    finally:
        c.close()


# ---- combined checks ----------------------------------------------------------------------------------------------------------------
def _combination(encs, verdicts, wts):
    """R = sum rho_i MegaCheck_i over the proofs that reach the final check, as one oracle MSM over the oracle's encodings"""
    sc, pt = b"", b""
    for i, v in enumerate(verdicts):
        if v in (0, 1) and (v == 0 or encs[32 * i:32 * i + 32] != bytes(32)):
            sc += (int.from_bytes(wts[64 * i:64 * i + 64], "little") % L).to_bytes(32, "little")
            pt += encs[32 * i:32 * i + 32]
    st, out = B.O.msm(sc, pt)
    assert st == 0
    return out


def _one_bad(n, m, nb, at):
    good, bad = B.proofs(n, m), B.variants(n, m)["t_x"]
    items = [bad if i == at else good[i % len(good)] for i in range(nb)]
    return b"".join(i[0] for i in items), b"".join(i[1] for i in items)


def test_combined_check_of_70_proofs_of_64_parties(ctx):
    n, m, nb = 8, 64, 70
    pl = B.O.proof_len(n, m)
    rng, wts = B.rng64(b"rlc-r", nb), B.rng64(b"rlc-w", nb)
    for at in (None, 41):
        proofs, coms = _one_bad(n, m, nb, at)
        verdict, ok, enc = ctx.rangeproof_verify_rlc(n, m, proofs, pl, coms, B.LABEL, rng, wts)
        per_proof = ctx.rangeproof_verify_batch(n, m, proofs, pl, coms, B.LABEL, rng)
        ev, em = B.expected(n, m, proofs, coms, rng)
        assert verdict == bytes(per_proof) == ev and list(ev) == [1 if i == at else 0 for i in range(nb)]
        assert ok == (at is None) and enc == _combination(em, ev, wts) and (enc == bytes(32)) == ok


def _mixed_groups(golden, bad_group):
    case = [q for q in golden["cases"] if q["n"] == 64 and q["m"] == 1][0]
    groups = [(64, 1, bytes.fromhex(case["proof"]) * 3, len(case["proof"]) // 2, golden["vc_bytes"][:32] * 3, golden["label"])]
    for g, (n, m) in enumerate([(8, 64), (8, 128), (32, 32)]):
        proofs, coms = _one_bad(n, m, 3, 1 if g + 1 == bad_group else None)
        groups.append((n, m, proofs, B.O.proof_len(n, m), coms, B.LABEL))
    return groups


def test_mixed_combined_check_with_64_and_128_parties(ctx, golden):
    for bad_group in (None, 2):
        groups = _mixed_groups(golden, bad_group)
        rng, wts = B.rng64(b"mix-r", 12), B.rng64(b"mix-w", 12)
        verdict, ok, enc = ctx.rangeproof_verify_rlc_mixed(groups, rng, wts)
        ev, em, per_proof = b"", b"", b""
        for g, (n, m, proofs, pl, coms, label) in enumerate(groups):
            r = rng[64 * 3 * g:64 * 3 * (g + 1)]
            v, e = B.expected(n, m, proofs, coms, r, label)
            ev, em = ev + v, em + e
            per_proof += ctx.rangeproof_verify_batch(n, m, proofs, pl, coms, label, r)
        assert verdict == per_proof == ev and list(ev) == [1 if (bad_group and i == 3 * bad_group + 1) else 0 for i in range(12)]
        assert ok == (bad_group is None) and enc == _combination(em, ev, wts) and (enc == bytes(32)) == ok


def test_mixed_combined_check_on_per_proof_states(ctx):
    """... on the callers' own transcripts: one state per proof, the (32, 32) group at the position with RP_COOP_MASKS_CAP + 1 masks"""
    _, hi = B.session_lengths_32_32()
    for bad in (None, 4):
        groups, states_all, ev, em, et = [], [], b"", b"", b""
        rng, wts = B.rng64(b"mixts-r", 9), B.rng64(b"mixts-w", 9)
        for g, (n, m) in enumerate([(8, 64), (8, 128), (32, 32)]):
            states = [B.session_state(10 * g + i, hi if g == 2 else 7 + 40 * i) for i in range(3)]
            proofs, coms = [], []
            for i, st in enumerate(states):
                pr, cm, _ = B.proof_on(n, m, i, st)
                if bad == 3 * g + i:
                    pr = B.tamper(n, m, pr, cm)["t_x"][0]
                proofs.append(pr)
                coms.append(cm)
            groups.append((n, m, b"".join(proofs), B.O.proof_len(n, m), b"".join(coms), b"".join(states)))
            v, e, t = B.expected_ts(n, m, groups[-1][2], groups[-1][4], groups[-1][5], rng[64 * 3 * g:64 * 3 * (g + 1)])
            ev, em, et = ev + v, em + e, et + t
        verdict, ok, enc, ts = ctx.rangeproof_verify_rlc_mixed_ts(groups, rng, wts, want_transcripts=True)
        assert verdict == ev and list(ev) == [1 if i == bad else 0 for i in range(9)]
        assert ts == et
        assert ok == (bad is None) and enc == _combination(em, ev, wts) and (enc == bytes(32)) == ok


# ---- the pool ---------------------------------------------------------------------------------------------------------------------
def test_pool_calls_from_8_threads(golden):
    """single-proof calls of (8, 128) on the callers' transcripts mixed with (64, 1) calls, from 8 threads at once; then one host call
    of 40 proofs of (8, 64)"""
    import bulletproofs_amd as bp
    pool = bp.Pool((0,), 2, fixed_window_bits=W)
    try:
        pool.gens_create(64, 128)
        case = [q for q in golden["cases"] if q["n"] == 64 and q["m"] == 1][0]
        gpr, gst = bytes.fromhex(case["proof"]), B.O.transcript_new(golden["label"])
        errors, results = [], {}

        def worker(t):
            try:
                for j in range(3):
                    if (t + j) % 2 == 0:
                        st = B.session_state(t, 20)
                        pr, cm, _ = B.proof_on(8, 128, t % 3, st)
                        if t == 5:
                            pr = B.tamper(8, 128, pr, cm)["a"][0]
                        n, m = 8, 128
                    else:
                        n, m, pr, cm, st = 64, 1, gpr, golden["vc_bytes"][:32], gst
                    rng = B.rng64(b"pool-%d-%d" % (t, j), 1)
                    got = pool.rangeproof_verify_ts(n, m, pr, len(pr), cm, st, rng, want_msm=True, want_transcripts=True)
                    results[(t, j)] = (got, (n, m, pr, cm, st, rng))
            except Exception as e:   # noqa: BLE001
                errors.append((t, repr(e)))

        B.proofs(8, 128)   # (the oracle's generators and proofs are made before the threads start)
        for t in range(8):
            B.proof_on(8, 128, t % 3, B.session_state(t, 20))
        threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        assert len(results) == 24
        for (t, j), (got, (n, m, pr, cm, st, rng)) in results.items():
            ev, em, et = B.expected_ts(n, m, pr, cm, st, rng)
            assert (got[0], got[2]) == (ev, et) and _encodings_equal(got[1], em), (t, j, n, m)
            assert ev[0] == (1 if (t == 5 and m == 128) else 0)
        n, m, nb = 8, 64, 40
        proofs, coms = B.batch(n, m, nb)
        rng = B.rng64(b"pool-40", nb)
        ev, em = B.expected(n, m, proofs, coms, rng)
        got = pool.rangeproof_verify(n, m, proofs, B.O.proof_len(n, m), coms, B.LABEL, rng, want_msm=True)
        assert got[0] == ev and _encodings_equal(got[1], em)
    finally:
        pool.close()


# ---- the other callers of the shape -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(8, 64), (8, 128)])
@pytest.mark.parametrize("constant_time", [0, 1])
def test_proof_creation_is_byte_identical_to_the_oracle(n, m, constant_time):
    c = _context({"prover_constant_time": constant_time})
    try:
        nb = 3
        vals = [x for p in range(nb) for x in B._values(n, m, p)]
        bl = b"".join(B._blindings(n, m, p) for p in range(nb))
        per = 64 * (m * (2 * n + 2) + 2 * m)
        seeds = [b"bigprove-%d-%d-%d" % (n, m, p) for p in range(nb)]
        rng = b"".join(hashlib.shake_256(sd).digest(per) for sd in seeds)
        st0 = B.padded_state([7])
        pl = B.O.proof_len(n, m)
        proofs, coms, ts = c.rangeproof_prove_batch(n, m, vals, bl, transcript=st0, rng=rng, want_transcripts=True)
        for p in range(nb):
            epr, ecm, ets = B.O.prove_ts(B.gens_for(n, m), vals[p * m:(p + 1) * m], bl[32 * m * p:32 * m * (p + 1)], n, st0, seeds[p])
            assert coms[32 * m * p:32 * m * (p + 1)] == ecm, (n, m, p)
            assert proofs[pl * p:pl * (p + 1)] == epr and ts[208 * p:208 * (p + 1)] == ets, (n, m, p)
    finally:
        c.close()


@pytest.fixture()
def small_ctx():
    c = _context()
    yield c
    c.close()


def test_multi_party_aggregation_of_64_parties(small_ctx):
    """one session of (8, 64): party steps and dealer steps byte-identical to the oracle; then a dishonest party at position 63 (a 64-bit
    value in an 8-bit proof), named by the dealer's audit"""
    import test_gpu_mpc as M
    ctx = small_ctx   # (a context whose arena no verification has grown: the helpers read it back after every step)
    n, m = 8, 64
    g = B.gens_for(n, m)
    s = M._session(B.O, g, n, m, b"big-mpc")
    M._check_parties(ctx, n, M._rows([s]))
    chal, AS, T_, proofs, bad, st4, st5, st6, ts = M._run_dealer(ctx, B.O, g, [s], None)
    assert st4 == st5 == st6 == bytes(1) and bad == bytes(m)
    assert chal == s["challenges"] and AS == s["proof"][:64] and T_ == s["proof"][64:128] and proofs == s["proof"]
    assert ts == B.O.prove_ts(g, s["vals"], s["bl"], n, B.O.transcript_new(M.LABEL), s["seed"])[2]
    vals = list(s["vals"])
    vals[63] = (1 << 63) | 5
    d = M._session(B.O, g, n, m, b"big-mpc-bad", vals, s["bl"])
    M._check_parties(ctx, n, M._rows([d]))
    _, _, _, proofs, named, st4, st5, st6, _ = M._run_dealer(ctx, B.O, g, [d], None)
    assert st4 == st5 == bytes(1) and st6 == bytes([2])              # BPGPU_MPC_MALFORMED_SHARES
    assert [j for j in range(m) if named[j]] == [63] and proofs == bytes(len(d["proof"]))
    sl = 32 * (3 + 2 * n)
    verdict = ctx.rangeproof_audit_shares(n, list(range(m)), d["shares"], d["bit_commitments"], d["poly_commitments"], d["challenges"])
    assert [j for j in range(m) if verdict[j]] == [63]
    assert B.O.audit_share(g, n, 63, d["shares"][sl * 63:sl * 64], d["bit_commitments"][96 * 63:96 * 64], d["poly_commitments"][64 * 63:64 * 64], d["challenges"])[0] == 1


def test_share_audit_of_128_parties(ctx):
    """rangeproof_audit_shares at (8, 128) for parties 0, 1, 64, 127 (y^(j n) up to j = 127), honest and with a tampered share each:
    verdicts and check points are oracle.audit_share's"""
    n, m = 8, 128
    g = B.gens_for(n, m)
    r = B.O.prove_shares(g, B._values(n, m, 0), B._blindings(n, m, 0), n, b"big audit", b"big-audit")
    sl = 32 * (3 + 2 * n)
    idx, sh, bc, pc = [], [], [], []
    for j in (0, 1, 64, 127):
        s_, b_, p_ = r["shares"][sl * j:sl * (j + 1)], r["bit_commitments"][96 * j:96 * j + 96], r["poly_commitments"][64 * j:64 * j + 64]
        t = bytearray(s_)
        t[96 + 7] ^= 1                                                # l_vec tampered: t_x != <l, r>
        e = bytearray(s_)
        e[70] ^= 1                                                    # e_blinding tampered: P_check fails
        for share, party in ((s_, j), (bytes(t), j), (bytes(e), j), (s_, (j + 1) % m)):   # ... and the share audited as its neighbour's
            idx.append(party), sh.append(share), bc.append(b_), pc.append(p_)
    verdict, chk = ctx.rangeproof_audit_shares(n, idx, b"".join(sh), b"".join(bc), b"".join(pc), r["challenges"], want_checks=True)
    assert list(verdict) == [0, 1, 1, 1] * 4
    for k in range(len(idx)):
        rc, out = B.O.audit_share(g, n, idx[k], sh[k], bc[k], pc[k], r["challenges"])
        assert verdict[k] == rc, k
        for h in (0, 1):
            if out[32 * h:32 * h + 32] != b"\xff" * 32:
                assert chk[64 * k + 32 * h:64 * k + 32 * h + 32] == out[32 * h:32 * h + 32], (k, h)


# ---- the documented maximum -------------------------------------------------------------------------------------------------------
def test_the_documented_maximum_64_bits_1024_parties():
    """(64, 1024), k = BP_RP_MAX_K: one valid and one tampered proof through the per-proof path, on a context of its own whose window
    table (fixed_window_bits = 2) takes 4.0 GiB; the device-derived generators are the oracle's"""
    n, m = 64, 1024
    c = _context(capacity=(n, m), window_bits=2)
    try:
        assert c.get_option("fixed_table_bytes") == 131074 * 128 * 2 * 128 < 8 << 30
        assert c.gens_export() == B.gens_for(n, m).export()
        pr, cm = B.proofs(n, m)[0]
        bad = B.tamper(n, m, pr, cm)["a"]
        _check(c, n, m, 2, b"max", batch=(pr + bad[0], cm + bad[1]))
    finally:
        c.close()
