"""GPU tests of the batch-combined InnerProductProof check (bpgpu_ipp_verify_rlc, csrc/ipp_rlc.h): verdicts always those of
bpgpu_ipp_verify_batch, and the combined point R = sum_p rho_p Check_p bit-exact against the oracle -- oracle.ipp_verify gives
compress(Check_p), oracle.msm combines them with the weights reduced in Python; compress(R) is canonical, so the comparison holds
whatever the summation order."""
import hashlib
import random

import pytest

pytestmark = pytest.mark.gpu

ELL = 2 ** 252 + 27742317777372353535851937790883648493
UNDECIDED = 5
LABEL = b"innerproducttest"
BOTH = pytest.mark.parametrize("fixed", [False, True], ids=["explicit", "table"])


@pytest.fixture(scope="module")
def ctx(oracle):
    """gens_create(64, 2): explicit bases and generator-table mode (G = H = None) on one context.  The reference helper's bases are
    BulletproofGens::new(n, 1)'s, which are the context's G(n, 1), H(n, 1): one instance set serves both modes."""
    import bulletproofs_amd as bp
    c = bp.Context(0)
    c.gens_create(64, 2)
    G, H = c.gens_export()[:2]
    inst = oracle.ipp_test_instance(64, LABEL, b"gipp-rlc-bases")
    assert inst["G"] == G[:32 * 64] == oracle.Gens(64, 1).export()[0] and inst["H"] == H[:32 * 64]
    yield c
    c.close()


def _weights(tag, nb):
    return hashlib.shake_256(b"ipp-rlc-weights-" + tag).digest(64 * nb)


def _rho(weights64, j):
    return (int.from_bytes(weights64[64 * j:64 * j + 64], "little") % ELL).to_bytes(32, "little")


def _cat(insts, key):
    return b"".join(i[key] for i in insts)


def _args(n, insts, fixed, G=None, H=None):
    """the positional arguments of Context.ipp_verify_rlc"""
    g0 = insts[0]
    return (n, _cat(insts, "proof"), len(g0["proof"]), _cat(insts, "Gf"), _cat(insts, "Hf"), _cat(insts, "P"), _cat(insts, "Q"),
            None if fixed else (G or g0["G"]), None if fixed else (H or g0["H"]))


def _per_proof(ctx, n, insts, G=None, H=None):
    nb, g0 = len(insts), insts[0]
    return ctx.ipp_verify_batch(n, _cat(insts, "proof"), len(g0["proof"]), LABEL, _cat(insts, "Gf"), _cat(insts, "Hf"), _cat(insts, "P"), _cat(insts, "Q"),
                                (G or g0["G"]) * nb, (H or g0["H"]) * nb)


def _reaches(inst, rc):
    """does the proof reach the final check?  Not with a FormatError (non-canonical a / b), nor with an identity L_j / R_j"""
    pr = inst["proof"]
    return rc != 2 and all(pr[o:o + 32] != bytes(32) for o in range(0, len(pr) - 64, 32))


def _oracle_combination(oracle, n, insts, weights64, G=None, H=None):
    """(per-proof codes, compress(sum_j rho_j Check_j), the indices combined) over the proofs that reach the final check; the point is
    None when a point of an included proof does not decode"""
    codes, scal, pts, undecoded, reach = [], b"", b"", False, []
    for j, i in enumerate(insts):
        rc, em = oracle.ipp_verify(n, i["proof"], LABEL, i["Gf"], i["Hf"], i["P"], i["Q"], G or i["G"], H or i["H"])
        codes.append(rc)
        if not _reaches(i, rc):
            continue
        reach.append(j)
        if em == b"\xff" * 32:
            undecoded = True
        else:
            scal += _rho(weights64, j)
            pts += em
    if undecoded:
        return codes, None, reach
    st_, enc = oracle.msm(scal, pts)
    assert st_ == 0
    return codes, enc, reach


def _dev_call(ctx, n, insts, fixed, label=LABEL, transcript=None, weights64=None, gens_m=1):
    """bpgpu_ipp_verify_rlc_dev on device buffers: (verdict bytes, batch_ok, enc)"""
    import torch
    import bulletproofs_amd as bp
    L = bp.lib()
    dev = torch.device("cuda", 0)
    nb, g0 = len(insts), insts[0]
    to_dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    ptr = lambda t: t.data_ptr() if t is not None else None
    d = {k: to_dev(_cat(insts, k)) for k in ("proof", "Gf", "Hf", "P", "Q")}
    d_g, d_h = (None, None) if fixed else (to_dev(g0["G"]), to_dev(g0["H"]))
    d_w = to_dev(weights64) if weights64 is not None else None
    d_v = torch.full((nb,), 255, dtype=torch.uint8, device=dev)
    d_o = torch.full((64,), 255, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    rc = L.bpgpu_ipp_verify_rlc_dev(ctx.h, n, nb, d["proof"].data_ptr(), len(g0["proof"]), label, len(label) if label else 0, transcript, d["Gf"].data_ptr(),
                                    d["Hf"].data_ptr(), d["P"].data_ptr(), d["Q"].data_ptr(), ptr(d_g), ptr(d_h), gens_m, ptr(d_w), d_v.data_ptr(),
                                    d_o.data_ptr(), s.cuda_stream)
    assert rc == 0
    s.synchronize()
    bo = bytes(d_o.cpu().numpy())
    return bytes(d_v.cpu().numpy()), bo[0] == 0, bo[1:33]


def _five_cases(oracle, n, tag):
    """the cases of test_make_ipp_verify: valid, tampered a, wrong P, non-canonical b, identity L_0 (n > 1; a plain valid proof at n = 1)"""
    insts = [oracle.ipp_test_instance(n, LABEL, b"%s-%d-%d" % (tag, n, j)) for j in range(5)]
    t = bytearray(insts[1]["proof"])
    t[-40] ^= 1
    insts[1] = dict(insts[1], proof=bytes(t))
    insts[2] = dict(insts[2], P=insts[2]["Q"])
    nc = bytearray(insts[3]["proof"])
    nc[-32:] = b"\xff" * 32
    insts[3] = dict(insts[3], proof=bytes(nc))
    if n > 1:
        li = bytearray(insts[4]["proof"])
        li[0:32] = bytes(32)
        insts[4] = dict(insts[4], proof=bytes(li))
    return insts


def _tamper(inst):
    bad = bytearray(inst["proof"])
    bad[-40] ^= 1                                               # a
    return dict(inst, proof=bytes(bad))


@pytest.fixture(scope="module")
def valid16(oracle):
    """130 valid proofs at n = 16 on the helper's bases"""
    return [oracle.ipp_test_instance(16, LABEL, b"rlc-valid-%d" % j) for j in range(130)]


@BOTH
@pytest.mark.parametrize("n", [1, 2, 4, 32, 64])
def test_parity_with_the_per_proof_path_and_the_oracle(ctx, oracle, n, fixed):
    insts = _five_cases(oracle, n, b"gipp-rlc")
    w = _weights(b"cases-%d" % n, 5)
    want = _per_proof(ctx, n, insts)
    verdict, ok, enc = ctx.ipp_verify_rlc(*_args(n, insts, fixed), label=LABEL, weights64=w)
    codes, comb, reach = _oracle_combination(oracle, n, insts, w)
    last = 1 if n > 1 else 0
    assert list(verdict) == [0, 1, 1, 2, last] == codes and verdict == want
    assert ok is False
    assert reach == ([0, 1, 2] if n > 1 else [0, 1, 2, 4])      # 3 (FormatError) and 4 (identity L_0) stop in the front end
    assert comb is not None and enc == comb != bytes(32)
    vd, okd, encd = _dev_call(ctx, n, insts, fixed, weights64=w)
    assert list(vd) == [UNDECIDED, UNDECIDED, UNDECIDED, 2, 1 if n > 1 else UNDECIDED] and okd is False and encd == enc


@BOTH
@pytest.mark.parametrize("nbatch", [1, 63, 64, 65, 130])
def test_all_valid_batches(ctx, oracle, valid16, nbatch, fixed):
    insts = valid16[:nbatch]
    w = _weights(b"valid-%d" % nbatch, nbatch)
    assert ctx.ipp_verify_rlc(*_args(16, insts, fixed), label=LABEL, weights64=w) == (bytes(nbatch), True, bytes(32))
    # a pre-bound shared transcript state instead of the label
    st = oracle.transcript_new(LABEL)
    assert ctx.ipp_verify_rlc(*_args(16, insts, fixed), transcript=st, weights64=w) == (bytes(nbatch), True, bytes(32))
    assert _dev_call(ctx, 16, insts, fixed, label=None, transcript=st, weights64=w) == (bytes(nbatch), True, bytes(32))
    # a state with history: the proofs no longer verify against it
    if nbatch == 65:
        st2 = oracle.transcript_append_message(st, b"x", b"y")
        got = ctx.ipp_verify_rlc(*_args(16, insts, fixed), transcript=st2, weights64=w)
        assert got[0] == bytes([1]) * nbatch and got[1] is False and got[2] != bytes(32)


@BOTH
@pytest.mark.parametrize("pos", [0, 63, 64])
def test_one_bad_proof_among_65(ctx, oracle, valid16, pos, fixed):
    nb = 65
    insts = list(valid16[:nb])
    insts[pos] = _tamper(insts[pos])
    fmt = bytearray(insts[7]["proof"])
    fmt[-32:] = b"\xff" * 32                                    # and a FormatError, which keeps its code
    insts[7] = dict(insts[7], proof=bytes(fmt))
    w = _weights(b"bad-%d" % pos, nb)
    want = _per_proof(ctx, 16, insts)
    assert [j for j in range(nb) if want[j]] == sorted({pos, 7}) and want[pos] == 1 and want[7] == 2
    verdict, ok, enc = ctx.ipp_verify_rlc(*_args(16, insts, fixed), label=LABEL, weights64=w)
    assert verdict == want and ok is False
    codes, comb, reach = _oracle_combination(oracle, 16, insts, w)
    assert bytes(codes) == want and enc == comb != bytes(32) and reach == [j for j in range(nb) if j != 7]
    vd, okd, encd = _dev_call(ctx, 16, insts, fixed, weights64=w)
    assert list(vd) == [2 if j == 7 else UNDECIDED for j in range(nb)] and okd is False and encd == comb


def test_short_weights_and_a_zero_weight(ctx, oracle, valid16):
    nb = 65
    short = hashlib.shake_256(b"ipp-rlc-short").digest(16 * nb)
    w = bytearray(b"".join(short[16 * j:16 * j + 16] + bytes(48) for j in range(nb)))   # 128-bit weights, zero-extended
    w[64 * 3:64 * 4] = bytes(64)                                                        # proof 3: weight zero
    w = bytes(w)
    # only the zero-weighted proof is bad: it is left unchecked, R is the identity
    insts = list(valid16[:nb])
    insts[3] = _tamper(insts[3])
    assert _dev_call(ctx, 16, insts, False, weights64=w) == (bytes(nb), True, bytes(32))
    # a second bad proof with a non-zero weight: R is not the identity; the host call falls back to the per-proof verdicts, proof 3 included
    insts[64] = _tamper(insts[64])
    want = _per_proof(ctx, 16, insts)
    assert [j for j in range(nb) if want[j]] == [3, 64]
    verdict, ok, enc = ctx.ipp_verify_rlc(*_args(16, insts, False), label=LABEL, weights64=w)
    codes, comb, _ = _oracle_combination(oracle, 16, insts, w)
    assert verdict == want == bytes(codes) and ok is False and enc == comb != bytes(32)


@BOTH
def test_library_drawn_weights(ctx, valid16, fixed):
    nb = 65
    insts = list(valid16[:nb])
    assert ctx.ipp_verify_rlc(*_args(16, insts, fixed), label=LABEL) == (bytes(nb), True, bytes(32))
    insts[20] = _tamper(insts[20])
    want = _per_proof(ctx, 16, insts)
    assert [j for j in range(nb) if want[j]] == [20]
    r1 = ctx.ipp_verify_rlc(*_args(16, insts, fixed), label=LABEL)
    r2 = ctx.ipp_verify_rlc(*_args(16, insts, fixed), label=LABEL)
    assert r1[0] == want == r2[0] and r1[1] is False and r2[1] is False
    assert r1[2] != r2[2] and bytes(32) not in (r1[2], r2[2])   # fresh weights per call


def _instance_on(oracle, n, G, H, seed):
    """a valid proof over the given bases with G_factors = 1 and random H_factors: P = <a, G> + <b o h, H> + <a, b> Q"""
    stream = hashlib.shake_256(b"ipp-rlc-inst-" + seed).digest(64 * (3 * n + 1))
    red = lambda i: int.from_bytes(stream[64 * i:64 * i + 64], "little") % ELL
    enc = lambda xs: b"".join(x.to_bytes(32, "little") for x in xs)
    a, b, h = [red(i) for i in range(n)], [red(n + i) for i in range(n)], [red(2 * n + i) for i in range(n)]
    q = red(3 * n).to_bytes(32, "little")
    Q = oracle.msm(q, G[:32])[1]
    c = sum(x * y for x, y in zip(a, b)) % ELL
    P = oracle.msm(enc(a) + enc([x * y % ELL for x, y in zip(b, h)]) + enc([c]), G + H + Q)[1]
    rc, proof = oracle.ipp_create(n, LABEL, Q, enc(h), G, H, enc(a), enc(b))
    assert rc == 0
    inst = dict(proof=proof, P=P, Q=Q, Gf=enc([1] * n), Hf=enc(h), G=G, H=H)
    assert oracle.ipp_verify(n, proof, LABEL, inst["Gf"], inst["Hf"], P, Q, G, H)[0] == 0
    return inst


def test_gens_m_2_chains_the_parties_generators(ctx, oracle):
    """n = 16 as bp_gens.G(8, 2) / H(8, 2): party 0's first 8 generators, then party 1's (range_proof/mod.rs:439-442)"""
    n, nb = 16, 5
    Gall, Hall = ctx.gens_export()[:2]
    pick = lambda buf: buf[:32 * 8] + buf[32 * 64:32 * 72]
    G, H = pick(Gall), pick(Hall)
    eg = oracle.Gens(8, 2).export()
    assert G == eg[0] and H == eg[1]
    insts = [_instance_on(oracle, n, G, H, b"m2-%d" % j) for j in range(nb)]
    w = _weights(b"m2", nb)
    assert ctx.ipp_verify_rlc(*_args(n, insts, True), label=LABEL, gens_m=2, weights64=w) == (bytes(nb), True, bytes(32))
    assert ctx.ipp_verify_rlc(*_args(n, insts, False), label=LABEL, weights64=w) == (bytes(nb), True, bytes(32))
    # against G(16, 1) the same proofs fail
    assert ctx.ipp_verify_rlc(*_args(n, insts, True), label=LABEL, gens_m=1, weights64=w)[0] == bytes([1]) * nb
    insts[2] = _tamper(insts[2])
    insts[4] = dict(insts[4], P=insts[4]["Q"])
    tab = ctx.ipp_verify_rlc(*_args(n, insts, True), label=LABEL, gens_m=2, weights64=w)
    exp = ctx.ipp_verify_rlc(*_args(n, insts, False), label=LABEL, weights64=w)
    codes, comb, _ = _oracle_combination(oracle, n, insts, w)
    assert tab == exp == (bytes(codes), False, comb) and codes == [0, 0, 1, 0, 1] and comb != bytes(32)
    assert _dev_call(ctx, n, insts, True, weights64=w, gens_m=2) == (bytes([UNDECIDED]) * nb, False, comb)


def test_a_shared_base_that_does_not_decode(ctx, oracle, valid16):
    """explicit bases with G_3 = 0xff..ff: the one MSM reports it, batch_out is 1 || zeros, and the host verdicts are the per-proof path's"""
    nb = 5
    insts = list(valid16[:nb])
    G = bytearray(insts[0]["G"])
    G[32 * 3:32 * 4] = b"\xff" * 32
    G = bytes(G)
    assert oracle.msm(bytes(32), G[96:128])[0] != 0
    w = _weights(b"undecodable", nb)
    want = _per_proof(ctx, 16, insts, G=G)
    verdict, ok, enc = ctx.ipp_verify_rlc(*_args(16, insts, False, G=G), label=LABEL, weights64=w)
    assert verdict == want == bytes([1]) * nb and ok is False and enc == bytes(32)
    assert _oracle_combination(oracle, 16, insts, w, G=G)[:2] == ([1] * nb, None)


def test_n256_explicit_bases_one_tampered(ctx, oracle):
    """8 proofs of n = 256 with the caller's bases: ONE variable-base MSM of 512 + 8 * 18 terms"""
    n = 256
    insts = [oracle.ipp_test_instance(n, LABEL, b"gipp256-rlc-%d" % j) for j in range(8)]
    insts[5] = _tamper(insts[5])
    w = _weights(b"n256", 8)
    want = _per_proof(ctx, n, insts)
    verdict, ok, enc = ctx.ipp_verify_rlc(*_args(n, insts, False), label=LABEL, weights64=w)
    codes, comb, _ = _oracle_combination(oracle, n, insts, w)
    assert list(verdict) == [0, 0, 0, 0, 0, 1, 0, 0] == codes and verdict == want
    assert ok is False and enc == comb != bytes(32)
    good = [i for j, i in enumerate(insts) if j != 5]
    assert ctx.ipp_verify_rlc(*_args(n, good, False), label=LABEL, weights64=w[:64 * 7]) == (bytes(7), True, bytes(32))


@BOTH
@pytest.mark.parametrize("nbatch", [8128, 8129])
def test_both_sides_of_the_block_walk_threshold(ctx, oracle, nbatch, fixed):
    """n = 64: 8 128 proofs are 8 128 x 128 < 2^20 (row, proof) pairs, one row per weigh lane; 8 129 proofs pad to 8 192 x 128 = 2^20
    pairs, eight rows per lane in Gray-code order.  Four distinct valid proofs tiled over the batch, the last one tampered: its weighted
    check point is the whole combination"""
    n = 64
    four = [oracle.ipp_test_instance(n, LABEL, b"rlc-walk-%d" % j) for j in range(4)]
    insts = [four[j % 4] for j in range(nbatch)]
    w = _weights(b"walk-%d" % nbatch, nbatch)
    assert ctx.ipp_verify_rlc(*_args(n, insts, fixed), label=LABEL, weights64=w) == (bytes(nbatch), True, bytes(32))
    insts[-1] = _tamper(insts[-1])
    want = _per_proof(ctx, n, insts)
    assert want == bytes(nbatch - 1) + b"\x01"
    verdict, ok, enc = ctx.ipp_verify_rlc(*_args(n, insts, fixed), label=LABEL, weights64=w)
    i = insts[-1]
    rc, em = oracle.ipp_verify(n, i["proof"], LABEL, i["Gf"], i["Hf"], i["P"], i["Q"], i["G"], i["H"])
    assert rc == 1 and verdict == want and ok is False and enc == oracle.msm(_rho(w, nbatch - 1), em)[1] != bytes(32)


def _fuzz_batch(oracle, n, seed):
    """120 seeded mutations of one instance in 8 kinds"""
    rnd = random.Random(seed)
    base = oracle.ipp_test_instance(n, LABEL, b"gipp-fuzz-%d" % n)
    pl, insts = len(base["proof"]), []
    for i in range(120):
        p, pp, hf = bytearray(base["proof"]), bytearray(base["P"]), bytearray(base["Hf"])
        kind = i % 8
        if kind == 1:
            p[rnd.randrange(pl)] ^= 1 << rnd.randrange(8)
        elif kind == 2:
            pp[rnd.randrange(32)] ^= 1 << rnd.randrange(8)
        elif kind == 3:
            off = 32 * rnd.randrange(pl // 32)
            p[off:off + 32] = bytes(rnd.randrange(256) for _ in range(32))
        elif kind == 4:
            off = 32 * rnd.randrange(pl // 32)
            p[off:off + 32] = bytes(32)
        elif kind == 5:
            p[32 * rnd.randrange(pl // 32) + 31] |= 0x80
        elif kind == 6:
            hf[32 * rnd.randrange(n) + rnd.randrange(31)] ^= 1 << rnd.randrange(8)         # stays canonical (top byte untouched)
        elif kind == 7:
            p[pl - 64 + rnd.randrange(64)] ^= 1 << rnd.randrange(8)                        # a or b
        insts.append(dict(base, proof=bytes(p), P=bytes(pp), Hf=bytes(hf)))
    return insts


FUZZ_SEED = 20261019


@pytest.mark.parametrize("n,fixed", [(4, False), (4, True), (16, False), (16, True)])
def test_differential_fuzz_against_the_per_proof_path_and_the_oracle(ctx, oracle, n, fixed):
    insts = _fuzz_batch(oracle, n, FUZZ_SEED + n)
    nb = len(insts)
    w = _weights(b"fuzz-%d" % n, nb)
    # conditions on the inputs, checked with the oracle alone before anything runs on the GPU: all three codes occur, and the sub-batch
    # whose every point decodes keeps at least 45 proofs
    codes, comb, reach = _oracle_combination(oracle, n, insts, w)
    assert set(codes) == {0, 1, 2}
    keep = [j for j, i in enumerate(insts)
            if oracle.ipp_verify(n, i["proof"], LABEL, i["Gf"], i["Hf"], i["P"], i["Q"], i["G"], i["H"])[1] != b"\xff" * 32]
    assert 45 <= len(keep) <= nb
    want = _per_proof(ctx, n, insts)
    verdict, ok, enc = ctx.ipp_verify_rlc(*_args(n, insts, fixed), label=LABEL, weights64=w)
    assert verdict == want == bytes(codes) and ok is False
    assert enc == (comb if comb is not None else bytes(32))
    vd, okd, encd = _dev_call(ctx, n, insts, fixed, weights64=w)
    assert list(vd) == [UNDECIDED if j in reach else codes[j] for j in range(nb)] and okd is False and encd == enc
    # the proofs whose every point decodes, on their own: the combination itself is compared
    sub = [insts[j] for j in keep]
    w2 = b"".join(w[64 * j:64 * j + 64] for j in keep)
    verdict2, ok2, enc2 = ctx.ipp_verify_rlc(*_args(n, sub, fixed), label=LABEL, weights64=w2)
    codes2, comb2, _ = _oracle_combination(oracle, n, sub, w2)
    assert verdict2 == bytes(codes2) == bytes(verdict[j] for j in keep) and ok2 is False
    assert comb2 is not None and enc2 == comb2 != bytes(32)


def test_error_paths(ctx, oracle):
    import bulletproofs_amd as bp
    n = 16
    g0 = oracle.ipp_test_instance(n, LABEL, b"rlc-err")
    two = [g0, g0]
    pl = len(g0["proof"])
    for fixed in (False, True):
        # a length that is no InnerProductProof length: FormatError for every proof, the empty combination
        a = _args(n, two, fixed)
        assert ctx.ipp_verify_rlc(n, g0["proof"][:-1] * 2, pl - 1, *a[3:], label=LABEL) == (bytes([2, 2]), True, bytes(32))
        # wrong n for the proof length: VerificationError from the front end, nothing enters R
        wide = dict(g0, Gf=g0["Gf"] * 2, Hf=g0["Hf"] * 2, G=g0["G"] * 2, H=g0["H"] * 2)
        assert ctx.ipp_verify_rlc(*_args(2 * n, [wide, wide], fixed), label=LABEL) == (bytes([1, 1]), True, bytes(32))
        assert ctx.ipp_verify_batch(2 * n, g0["proof"] * 2, pl, LABEL, wide["Gf"] * 2, wide["Hf"] * 2, g0["P"] * 2, g0["Q"] * 2, wide["G"] * 2, wide["H"] * 2) == \
            bytes([1, 1])
    # gens_m must divide n and lie within the context's parties
    with pytest.raises(bp.BpgpuError, match="^INVALID_ARG"):
        ctx.ipp_verify_rlc(*_args(n, two, True), label=LABEL, gens_m=3)
    with pytest.raises(bp.BpgpuError, match="^INVALID_ARG"):
        ctx.ipp_verify_rlc(*_args(n, two, True), label=LABEL, gens_m=0)
    with pytest.raises(bp.BpgpuError, match="^NO_GENS"):
        ctx.ipp_verify_rlc(*_args(n, two, True), label=LABEL, gens_m=4)
    # more generators than the context holds: an error code, not a verdict
    big = oracle.ipp_test_instance(128, LABEL, b"rlc-err-big")
    with pytest.raises(bp.BpgpuError, match="^NO_GENS"):
        ctx.ipp_verify_rlc(*_args(128, [big], True), label=LABEL)
    # the same proof with its own bases still verifies, and the context is usable after the error
    assert ctx.ipp_verify_rlc(*_args(128, [big], False), label=LABEL) == (bytes(1), True, bytes(32))
    assert ctx.ipp_verify_rlc(*_args(n, two, True), label=LABEL) == (bytes(2), True, bytes(32))
    # a context without generators: generator-table mode is an error, explicit bases work
    bare = bp.Context(0)
    with pytest.raises(bp.BpgpuError, match="^NO_GENS"):
        bare.ipp_verify_rlc(*_args(n, two, True), label=LABEL)
    assert bare.ipp_verify_rlc(*_args(n, two, False), label=LABEL) == (bytes(2), True, bytes(32))
    bare.close()
    # exactly one of G, H missing
    a = _args(n, two, False)
    for G, H in ((None, a[8]), (a[7], None)):
        with pytest.raises(bp.BpgpuError, match="^INVALID_ARG"):
            ctx.ipp_verify_rlc(*a[:7], G, H, label=LABEL)
    # no proofs
    assert ctx.ipp_verify_rlc(n, b"", pl, b"", b"", b"", b"", g0["G"], g0["H"], label=LABEL) == (b"", True, bytes(32))
    assert ctx.ipp_verify_rlc(n, b"", pl, b"", b"", b"", b"", None, None, label=LABEL) == (b"", True, bytes(32))
