"""GPU tests of the batch-combined LinearProof check (bpgpu_linear_verify_rlc, csrc/linear_rlc.h): verdicts always those of
bpgpu_linear_verify_batch, and the combined point R = sum_p rho_p Check_p bit-exact against the oracle -- oracle.linear_verify gives
compress(Check_p), oracle.msm combines them with the weights reduced in Python; compress(R) is canonical, so the comparison holds
whatever the summation order."""
import hashlib
import random

import pytest

from test_device_code_on_cpu import _linear_cases

pytestmark = pytest.mark.gpu

ELL = 2 ** 252 + 27742317777372353535851937790883648493
UNDECIDED = 5


@pytest.fixture(scope="module")
def ctx():
    """gens_create(64, 2): explicit bases and generator-table mode (G = F = B = None) on one context"""
    import bulletproofs_amd as bp
    c = bp.Context(0)
    c.gens_create(64, 2)
    yield c
    c.close()


def _weights(tag, nb):
    return hashlib.shake_256(b"lin-rlc-weights-" + tag).digest(64 * nb)


def _rho(weights64, j):
    return (int.from_bytes(weights64[64 * j:64 * j + 64], "little") % ELL).to_bytes(32, "little")


def _bases(g, fixed):
    return (None, None, None) if fixed else (g["G"], g["F"], g["B"])


def _oracle_combination(oracle, n, proofs, pl, Cs, bs, base, st, weights64):
    """(per-proof codes, compress(sum_j rho_j Check_j)) over the proofs that reach the final check -- a proof that stops before it
    leaves the oracle's output at the identity encoding and adds nothing; None when a point of an included proof does not decode"""
    nb = len(Cs) // 32
    shared = len(bs) == 32 * n and nb != 1
    codes, scal, pts, undecoded = [], b"", b"", False
    for j in range(nb):
        rc, em = oracle.linear_verify(n, proofs[pl * j:pl * (j + 1)], st, Cs[32 * j:32 * j + 32], base["G"], base["F"], base["B"],
                                      bs if shared else bs[32 * n * j:32 * n * (j + 1)])
        codes.append(rc)
        if em == b"\xff" * 32:
            undecoded = True
        elif rc != 2:
            scal += _rho(weights64, j)
            pts += em
    if undecoded:
        return codes, None
    st_, enc = oracle.msm(scal, pts)
    assert st_ == 0
    return codes, enc


def _dev_call(ctx, n, proofs, pl, Cs, bases, bs, label=b"", transcript=None, weights64=None):
    """bpgpu_linear_verify_rlc_dev on device buffers: (verdict bytes, batch_ok, enc)"""
    import torch
    import bulletproofs_amd as bp
    L = bp.lib()
    dev = torch.device("cuda", 0)
    nb = len(Cs) // 32
    to_dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    ptr = lambda t: t.data_ptr() if t is not None else None
    d_pr, d_c, d_b = to_dev(proofs), to_dev(Cs), to_dev(bs)
    d_g, d_f, d_bb = (to_dev(x) if x is not None else None for x in bases)
    d_w = to_dev(weights64) if weights64 is not None else None
    d_v = torch.full((nb,), 255, dtype=torch.uint8, device=dev)
    d_o = torch.full((64,), 255, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    rc = L.bpgpu_linear_verify_rlc_dev(ctx.h, n, nb, d_pr.data_ptr(), pl, label, len(label), transcript, d_c.data_ptr(), ptr(d_g), ptr(d_f), ptr(d_bb),
                                       d_b.data_ptr(), 1 if (len(bs) == 32 * n and nb != 1) else 0, ptr(d_w), d_v.data_ptr(), d_o.data_ptr(), None,
                                       s.cuda_stream)
    assert rc == 0
    s.synchronize()
    bo = bytes(d_o.cpu().numpy())
    return bytes(d_v.cpu().numpy()), bo[0] == 0, bo[1:33]


@pytest.fixture(scope="module")
def valid16(oracle):
    """130 valid proofs at n = 16, twice: `insts` with a public vector per proof (the reference's test shape, one label), and `proofs` /
    `Cs` for one public vector (`base["b"]`) over a caller transcript that already holds a message (`st_app`)"""
    n, nb = 16, 130
    insts = [oracle.linear_test_instance(n, b"rlc-valid-%d" % j) for j in range(nb)]
    base = insts[0]
    st_app = oracle.transcript_append_message(oracle.transcript_new(b"app protocol"), b"ctx", b"session 42")
    proofs, Cs = [], []
    for j in range(nb):
        stream = hashlib.shake_256(b"rlc-many%d" % j).digest(64 * (n + 1 + 2 * 4 + 2))
        red = lambda i: (int.from_bytes(stream[64 * i:64 * i + 64], "little") % ELL).to_bytes(32, "little")
        a = b"".join(red(i) for i in range(n))
        r = red(n)
        c = sum(int.from_bytes(a[32 * i:32 * i + 32], "little") * int.from_bytes(base["b"][32 * i:32 * i + 32], "little") for i in range(n)) % ELL
        rcm, Cc = oracle.msm(a + r + c.to_bytes(32, "little"), base["G"] + base["B"] + base["F"])
        assert rcm == 0
        rc, pr = oracle.linear_create(n, st_app, stream[64 * (n + 1):], Cc, r, a, base["b"], base["G"], base["F"], base["B"])
        assert rc == 0
        proofs.append(pr)
        Cs.append(Cc)
    return dict(n=n, insts=insts, base=base, st_app=st_app, proofs=proofs, Cs=Cs, pl=len(proofs[0]))


@pytest.mark.parametrize("fixed", [False, True], ids=["explicit", "table"])
@pytest.mark.parametrize("n", [1, 2, 16, 64])
def test_parity_with_the_per_proof_path_and_the_oracle(ctx, oracle, n, fixed):
    insts, pl = _linear_cases(oracle, n, b"glin-rlc")
    cat = lambda key: b"".join(i[key] for i in insts)
    g0 = insts[0]
    w = _weights(b"cases-%d" % n, 5)
    bases = _bases(g0, fixed)
    want = ctx.linear_verify_batch(n, cat("proof"), pl, cat("C"), *bases, cat("b"), label=g0["label"])
    verdict, ok, enc = ctx.linear_verify_rlc(n, cat("proof"), pl, cat("C"), *bases, cat("b"), label=g0["label"], weights64=w)
    assert list(verdict) == [0, 1, 2, 1, 1] and verdict == want
    assert ok is False
    st = oracle.transcript_new(g0["label"])
    codes, comb = _oracle_combination(oracle, n, cat("proof"), pl, cat("C"), cat("b"), g0, st, w)
    assert codes == [0, 1, 2, 1, 1]
    if n > 1:
        # cases 0, 1, 4 reach the final check; 2 (FormatError) and 3 (identity L_0) stop in the front end
        em = [oracle.linear_verify(n, insts[j]["proof"], st, insts[j]["C"], g0["G"], g0["F"], g0["B"], insts[j]["b"])[1] for j in (0, 1, 4)]
        assert enc == oracle.msm(b"".join(_rho(w, j) for j in (0, 1, 4)), b"".join(em))[1] == comb
        assert enc != bytes(32)
    else:
        assert comb is None and enc == bytes(32)          # case 3: S does not decode
    vd, okd, encd = _dev_call(ctx, n, cat("proof"), pl, cat("C"), bases, cat("b"), label=g0["label"], weights64=w)
    assert list(vd) == [UNDECIDED, UNDECIDED, 2, 1 if n > 1 else UNDECIDED, UNDECIDED] and okd is False and encd == enc


@pytest.mark.parametrize("fixed", [False, True], ids=["explicit", "table"])
@pytest.mark.parametrize("nbatch", [1, 63, 64, 65, 130])
def test_all_valid_batches(ctx, valid16, nbatch, fixed):
    v = valid16
    n, pl = v["n"], v["pl"]
    bases = _bases(v["base"], fixed)
    w = _weights(b"valid-%d" % nbatch, nbatch)
    # a public vector per proof
    ins = v["insts"][:nbatch]
    cat = lambda key: b"".join(i[key] for i in ins)
    label = ins[0]["label"]
    got = ctx.linear_verify_rlc(n, cat("proof"), len(ins[0]["proof"]), cat("C"), *bases, cat("b"), label=label, weights64=w, want_transcripts=True)
    ref = ctx.linear_verify_batch(n, cat("proof"), len(ins[0]["proof"]), cat("C"), *bases, cat("b"), label=label, want_transcripts=True)
    assert got[0] == bytes(nbatch) == ref[0] and got[1] is True and got[2] == bytes(32) and got[3] == ref[1]
    # one shared vector over a caller transcript that already holds a message
    proofs, Cs = b"".join(v["proofs"][:nbatch]), b"".join(v["Cs"][:nbatch])
    got = ctx.linear_verify_rlc(n, proofs, pl, Cs, *bases, v["base"]["b"], transcript=v["st_app"], weights64=w, want_transcripts=True)
    ref = ctx.linear_verify_batch(n, proofs, pl, Cs, *bases, v["base"]["b"], transcript=v["st_app"], want_transcripts=True)
    assert got[0] == bytes(nbatch) == ref[0] and got[1] is True and got[2] == bytes(32) and got[3] == ref[1]


@pytest.mark.parametrize("fixed", [False, True], ids=["explicit", "table"])
@pytest.mark.parametrize("pos", [0, 63, 64])
def test_one_bad_proof_among_65(ctx, oracle, valid16, pos, fixed):
    v = valid16
    n, pl, nb = v["n"], v["pl"], 65
    bases = _bases(v["base"], fixed)
    pr = list(v["proofs"][:nb])
    bad = bytearray(pr[pos])
    bad[pl - 64] ^= 1                                           # a tampered
    pr[pos] = bytes(bad)
    fmt = bytearray(pr[7])
    fmt[pl - 32:] = b"\xff" * 32                                # and a FormatError, which keeps its code
    pr[7] = bytes(fmt)
    proofs, Cs, b = b"".join(pr), b"".join(v["Cs"][:nb]), v["base"]["b"]
    w = _weights(b"bad-%d" % pos, nb)
    want = ctx.linear_verify_batch(n, proofs, pl, Cs, *bases, b, transcript=v["st_app"])
    assert [j for j in range(nb) if want[j]] == sorted({pos, 7}) and want[pos] == 1 and want[7] == 2
    verdict, ok, enc = ctx.linear_verify_rlc(n, proofs, pl, Cs, *bases, b, transcript=v["st_app"], weights64=w)
    assert verdict == want and ok is False
    codes, comb = _oracle_combination(oracle, n, proofs, pl, Cs, b, v["base"], v["st_app"], w)
    assert bytes(codes) == want and enc == comb != bytes(32)
    vd, okd, encd = _dev_call(ctx, n, proofs, pl, Cs, bases, b, transcript=v["st_app"], weights64=w)
    assert list(vd) == [2 if j == 7 else UNDECIDED for j in range(nb)] and okd is False and encd == comb


def test_short_weights_and_a_zero_weight(ctx, oracle, valid16):
    v = valid16
    n, pl, nb = v["n"], v["pl"], 65
    bases = _bases(v["base"], False)
    pr = list(v["proofs"][:nb])
    for pos in (3, 64):
        bad = bytearray(pr[pos])
        bad[pl - 64] ^= 1
        pr[pos] = bytes(bad)
    Cs, b = b"".join(v["Cs"][:nb]), v["base"]["b"]
    short = hashlib.shake_256(b"lin-rlc-short").digest(16 * nb)
    w = bytearray(b"".join(short[16 * j:16 * j + 16] + bytes(48) for j in range(nb)))   # 128-bit weights, zero-extended
    w[64 * 3:64 * 4] = bytes(64)                                                        # proof 3: weight zero
    w = bytes(w)
    # only the zero-weighted proof is bad: it is left unchecked, R is the identity
    one_bad = b"".join(pr[:64] + [v["proofs"][64]])
    vd, okd, encd = _dev_call(ctx, n, one_bad, pl, Cs, bases, b, transcript=v["st_app"], weights64=w)
    assert vd == bytes(nb) and okd is True and encd == bytes(32)
    # a second bad proof with a non-zero weight: R is not the identity; the host call falls back to the per-proof verdicts, proof 3 included
    proofs = b"".join(pr)
    want = ctx.linear_verify_batch(n, proofs, pl, Cs, *bases, b, transcript=v["st_app"])
    assert [j for j in range(nb) if want[j]] == [3, 64]
    verdict, ok, enc = ctx.linear_verify_rlc(n, proofs, pl, Cs, *bases, b, transcript=v["st_app"], weights64=w)
    codes, comb = _oracle_combination(oracle, n, proofs, pl, Cs, b, v["base"], v["st_app"], w)
    assert verdict == want == bytes(codes) and ok is False and enc == comb != bytes(32)


@pytest.mark.parametrize("fixed", [False, True], ids=["explicit", "table"])
def test_library_drawn_weights(ctx, valid16, fixed):
    v = valid16
    n, pl, nb = v["n"], v["pl"], 65
    bases = _bases(v["base"], fixed)
    proofs, Cs, b = b"".join(v["proofs"][:nb]), b"".join(v["Cs"][:nb]), v["base"]["b"]
    assert ctx.linear_verify_rlc(n, proofs, pl, Cs, *bases, b, transcript=v["st_app"]) == (bytes(nb), True, bytes(32))
    bad = bytearray(proofs)
    bad[pl * 20 + pl - 64] ^= 1
    bad = bytes(bad)
    want = ctx.linear_verify_batch(n, bad, pl, Cs, *bases, b, transcript=v["st_app"])
    assert [j for j in range(nb) if want[j]] == [20]
    r1 = ctx.linear_verify_rlc(n, bad, pl, Cs, *bases, b, transcript=v["st_app"])
    r2 = ctx.linear_verify_rlc(n, bad, pl, Cs, *bases, b, transcript=v["st_app"])
    assert r1[0] == want == r2[0] and r1[1] is False and r2[1] is False
    assert r1[2] != r2[2] and bytes(32) not in (r1[2], r2[2])   # fresh weights per call


def test_n256_explicit_bases_one_tampered(ctx, oracle):
    """8 proofs of n = 256 with the caller's bases: ONE variable-base MSM of 258 + 8 * 18 terms"""
    n = 256
    insts = [oracle.linear_test_instance(n, b"glin256-rlc-%d" % j) for j in range(8)]
    bad = bytearray(insts[5]["proof"])
    bad[-1 - 32] ^= 1
    insts[5] = dict(insts[5], proof=bytes(bad))
    cat = lambda key: b"".join(i[key] for i in insts)
    g0 = insts[0]
    pl = len(g0["proof"])
    w = _weights(b"n256", 8)
    want = ctx.linear_verify_batch(n, cat("proof"), pl, cat("C"), g0["G"], g0["F"], g0["B"], cat("b"), label=g0["label"])
    verdict, ok, enc = ctx.linear_verify_rlc(n, cat("proof"), pl, cat("C"), g0["G"], g0["F"], g0["B"], cat("b"), label=g0["label"], weights64=w)
    codes, comb = _oracle_combination(oracle, n, cat("proof"), pl, cat("C"), cat("b"), g0, oracle.transcript_new(g0["label"]), w)
    assert list(verdict) == [0, 0, 0, 0, 0, 1, 0, 0] == codes and verdict == want
    assert ok is False and enc == comb != bytes(32)
    good = [i for j, i in enumerate(insts) if j != 5]
    cat = lambda key: b"".join(i[key] for i in good)
    assert ctx.linear_verify_rlc(n, cat("proof"), pl, cat("C"), g0["G"], g0["F"], g0["B"], cat("b"), label=g0["label"], weights64=w[:64 * 7]) == \
        (bytes(7), True, bytes(32))


@pytest.mark.parametrize("n,fixed", [(4, False), (4, True), (16, False), (16, True)])
def test_differential_fuzz_against_the_per_proof_path_and_the_oracle(ctx, oracle, n, fixed):
    """the mutation scheme of test_linear_differential_fuzz_against_oracle: seeded single-bit / 32-byte mutations anywhere in the
    proof, the commitment or the public vector"""
    rnd = random.Random(20260924 + n)
    base = oracle.linear_test_instance(n, b"glin-fuzz-%d" % n)
    pl, nb = len(base["proof"]), 120
    proofs, Cs, bs = bytearray(), bytearray(), bytearray()
    for i in range(nb):
        p, cc, b = bytearray(base["proof"]), bytearray(base["C"]), bytearray(base["b"])
        kind = i % 8
        if kind == 1:
            p[rnd.randrange(pl)] ^= 1 << rnd.randrange(8)
        elif kind == 2:
            cc[rnd.randrange(32)] ^= 1 << rnd.randrange(8)
        elif kind == 3:
            off = 32 * rnd.randrange(pl // 32)
            p[off:off + 32] = bytes(rnd.randrange(256) for _ in range(32))
        elif kind == 4:
            off = 32 * rnd.randrange(pl // 32)
            p[off:off + 32] = bytes(32)
        elif kind == 5:
            p[32 * rnd.randrange(pl // 32) + 31] |= 0x80
        elif kind == 6:
            b[32 * rnd.randrange(n) + rnd.randrange(31)] ^= 1 << rnd.randrange(8)          # stays canonical (top byte untouched)
        elif kind == 7:
            p[pl - 64 + rnd.randrange(64)] ^= 1 << rnd.randrange(8)                        # a or r
        proofs += p
        Cs += cc
        bs += b
    proofs, Cs, bs = bytes(proofs), bytes(Cs), bytes(bs)
    bases = _bases(base, fixed)
    w = _weights(b"fuzz-%d" % n, nb)
    want = ctx.linear_verify_batch(n, proofs, pl, Cs, *bases, bs, label=base["label"])
    verdict, ok, enc = ctx.linear_verify_rlc(n, proofs, pl, Cs, *bases, bs, label=base["label"], weights64=w)
    assert verdict == want and set(verdict) == {0, 1, 2} and ok is False
    st = oracle.transcript_new(base["label"])
    codes, comb = _oracle_combination(oracle, n, proofs, pl, Cs, bs, base, st, w)
    assert bytes(codes) == verdict
    assert enc == (comb if comb is not None else bytes(32))
    # the proofs whose every point decodes, on their own: the combination itself is compared
    keep = [i for i in range(nb) if oracle.linear_verify(n, proofs[pl * i:pl * (i + 1)], st, Cs[32 * i:32 * i + 32], base["G"], base["F"], base["B"],
                                                         bs[32 * n * i:32 * n * (i + 1)])[1] != b"\xff" * 32]
    assert 45 <= len(keep) <= nb
    sub = lambda buf, sz: b"".join(buf[sz * i:sz * (i + 1)] for i in keep)
    p2, c2, b2, w2 = sub(proofs, pl), sub(Cs, 32), sub(bs, 32 * n), sub(w, 64)
    verdict2, ok2, enc2 = ctx.linear_verify_rlc(n, p2, pl, c2, *bases, b2, label=base["label"], weights64=w2)
    codes2, comb2 = _oracle_combination(oracle, n, p2, pl, c2, b2, base, st, w2)
    assert verdict2 == bytes(codes2) == bytes(verdict[i] for i in keep) and ok2 is False
    assert comb2 is not None and enc2 == comb2 != bytes(32)


def test_error_paths(ctx, oracle):
    import bulletproofs_amd as bp
    n = 16
    g0 = oracle.linear_test_instance(n, b"rlc-err")
    pl = len(g0["proof"])
    # a length that is no LinearProof length: FormatError for every proof, the empty combination
    assert ctx.linear_verify_rlc(n, g0["proof"][:-1] * 2, pl - 1, g0["C"] * 2, g0["G"], g0["F"], g0["B"], g0["b"] * 2, label=g0["label"]) == \
        (bytes([2, 2]), True, bytes(32))
    # wrong n for the proof length: VerificationError from the front end, nothing enters R
    assert ctx.linear_verify_rlc(2 * n, g0["proof"] * 2, pl, g0["C"] * 2, g0["G"] * 2, g0["F"], g0["B"], g0["b"] * 4, label=g0["label"]) == \
        (bytes([1, 1]), True, bytes(32))
    assert ctx.linear_verify_rlc(2 * n, g0["proof"] * 2, pl, g0["C"] * 2, None, None, None, g0["b"] * 4, label=g0["label"])[0] == bytes([1, 1])
    # more generators than the context holds: an error, not a verdict
    big = oracle.linear_test_instance(128, b"rlc-err-big")
    with pytest.raises(bp.BpgpuError):
        ctx.linear_verify_rlc(128, big["proof"], len(big["proof"]), big["C"], None, None, None, big["b"], label=big["label"])
    # the same proof with its own bases still verifies, and the context is usable after the error
    assert ctx.linear_verify_rlc(128, big["proof"], len(big["proof"]), big["C"], big["G"], big["F"], big["B"], big["b"], label=big["label"]) == \
        (bytes(1), True, bytes(32))
    # no proofs
    assert ctx.linear_verify_rlc(n, b"", pl, b"", g0["G"], g0["F"], g0["B"], g0["b"], label=g0["label"]) == (b"", True, bytes(32))


def test_api_verify_batch_combined(ctx, valid16):
    from bulletproofs_amd.api import LinearProof, Transcript, VerificationError
    v = valid16
    n, nb = v["n"], 5
    split = lambda buf: [buf[32 * i:32 * i + 32] for i in range(len(buf) // 32)]
    pr = list(v["proofs"][:nb])
    bad = bytearray(pr[2])
    bad[v["pl"] - 64] ^= 1
    pr[2] = bytes(bad)
    t = Transcript(b"app protocol")
    t.append_message(b"ctx", b"session 42")
    assert t.state == v["st_app"]
    args = (ctx, t, [LinearProof.from_bytes(p) for p in pr], v["Cs"][:nb], split(v["base"]["G"]), v["base"]["F"], v["base"]["B"], split(v["base"]["b"]))
    got, ref = LinearProof.verify_batch_combined(*args), LinearProof.verify_batch(*args)
    assert [type(x) for x in got] == [type(x) for x in ref] == [type(None), type(None), VerificationError, type(None), type(None)]
