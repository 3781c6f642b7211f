"""R1CS proof creation on the GPU (bpgpu_r1cs_prove_batch) against the twin prover with the reference's TranscriptRng
(tests/r1cs_prover_twin.py): proof bytes, V commitments and the transcript each proof leaves, bit for bit; and every proof
through the GPU verifier."""
import hashlib
import random

import pytest

import r1cs_prover_twin as P
import r1cs_twin as R

pytestmark = pytest.mark.gpu

CAP = 128


@pytest.fixture(scope="module")
def gens(oracle):
    return oracle.Gens(CAP, 1).export()


@pytest.fixture(scope="module")
def ctx():
    import bulletproofs_amd as bp
    c = bp.Context(0)
    c.gens_create(CAP, 1)
    yield c
    c.close()


def _scalars(tag, n):
    return [int.from_bytes(hashlib.shake_256(tag + b"%d" % i).digest(64), "little") % R.L for i in range(n)]


def _shuffle(k, seed, permute=True):
    rnd = random.Random(seed)
    inp = [rnd.getrandbits(64) for _ in range(k)]
    out = inp[:]
    rnd.shuffle(out)
    if not permute:
        out[0] += 1
    return inp + out


def _sg(k):
    return lambda cs, v: R.shuffle_gadget(cs, v[:k], v[k:])


def _range_p(vals, n):
    return lambda cs, x: R.range_gadget(cs, x[0], vals[0], n)


def _range_v(n):
    return lambda cs, x: R.range_gadget(cs, x[0], None, n)


def _prove(c, gadget_p, gadget_v, vals_list, st0s, rng32, shared=False, gens=None, cap=CAP, check_twin=True):
    """prove len(vals_list) proofs on the GPU; compare with the twin; verify them on the GPU.  Returns (proofs, coms, status)."""
    from bulletproofs_amd import r1cs
    nb = len(vals_list)
    provers, bls = [], []
    for b, vals in enumerate(vals_list):
        cs = r1cs.Prover(st0s[0] if shared else st0s[b])
        bl = _scalars(b"bl%d-" % b, len(vals))
        bls.append(bl)
        xs = [cs.commit(v, x) for v, x in zip(vals, bl)]
        gadget_p(cs, xs)
        provers.append(cs)
    assert all(p.structure() == provers[0].structure() for p in provers)
    ins = [p.inputs() for p in provers]
    circuit = provers[0].circuit()
    ts = st0s[0] if shared else b"".join(st0s)
    proofs, coms, status, tso = provers[0].witness().prove_batch(c, circuit, nb, b"".join(i[0] for i in ins), b"".join(i[1] for i in ins),
                                                                  b"".join(i[2] for i in ins), ts, rng32, want_transcripts=True)
    m = circuit.m
    if check_twin:
        for b in range(nb):
            if status[b]:
                continue
            st0 = st0s[0] if shared else st0s[b]
            pf, Vs, twin = P.prove(gens, cap, st0, vals_list[b], bls[b], gadget_p, rng32[32 * b:32 * b + 32])
            assert proofs[b] == pf.to_bytes(), b
            assert coms[32 * m * b:32 * m * (b + 1)] == b"".join(Vs), b
            assert tso[208 * b:208 * (b + 1)] == R.transcript_state(twin.t), b
    # the GPU verifier over the same gadget
    ver = r1cs.Verifier(st0s[0])
    vs = [ver.commit(bytes(32)) for _ in range(m)]
    gadget_v(ver, vs)
    verdict = ver.circuit().verify_batch(c, proofs, coms, ts, rng32=hashlib.shake_256(b"vrng").digest(32 * nb))
    return proofs, coms, status, verdict


def _st0s(tag, nb):
    return [R.transcript_state(R.T.Transcript(tag + b"%d" % b)) for b in range(nb)]


def _rng(tag, nb):
    return hashlib.shake_256(b"r1cs-prove-rng" + tag).digest(32 * nb)


@pytest.mark.parametrize("ct", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 8, 16])
def test_shuffle_proofs_match_twin(ctx, gens, k, ct):
    ctx.set_option("prover_constant_time", ct)
    try:
        nb = 3
        vals = [_shuffle(k, 100 * k + b) for b in range(nb)]
        shared = k % 2 == 0
        _, _, status, verdict = _prove(ctx, _sg(k), _sg(k), vals, _st0s(b"ShuffleProof%d-" % k, nb), _rng(b"s%d" % k, nb), shared=shared, gens=gens)
        assert status == bytes(nb) and verdict == bytes(nb)
    finally:
        ctx.set_option("prover_constant_time", 0)


@pytest.mark.parametrize("ct", [0, 1])
def test_example_gadget_is_version_0(ctx, gens, ct):
    ctx.set_option("prover_constant_time", ct)
    try:
        g = lambda cs, v: R.example_gadget(cs, v[0], v[1], v[2], v[3], v[4], 9)
        vals = [[3, 4, 6, 1, 40], [1, 2, 3, 0, 0]]
        proofs, _, status, verdict = _prove(ctx, g, g, vals, _st0s(b"R1CSExampleGadget", 2), _rng(b"ex%d" % ct, 2), gens=gens)
        assert status == bytes(2) and verdict == bytes(2)
        assert all(p[0] == 0 and len(p) == 1 + 32 * 11 + 64 for p in proofs)
    finally:
        ctx.set_option("prover_constant_time", 0)


@pytest.mark.parametrize("n", [8, 64])
def test_range_gadget_proofs_match_twin(ctx, gens, n):
    vals = [[random.Random(n + b).getrandbits(n)] for b in range(2)]
    for b in range(2):   # (one gadget function per proof: the assignments differ; the structure does not)
        _, _, status, verdict = _prove(ctx, _range_p(vals[b], n), _range_v(n), [vals[b]], _st0s(b"RangeProofTest%d-" % b, 1), _rng(b"r%d%d" % (n, b), 1),
                                       gens=gens)
        assert status == bytes(1) and verdict == bytes(1)


@pytest.mark.parametrize("ct", [0, 1])
@pytest.mark.parametrize("which", ["split", "open"])
def test_allocate_pair_gadgets_match_twin(ctx, gens, which, ct):
    ctx.set_option("prover_constant_time", ct)
    try:
        gp = P.split_gadget if which == "split" else P.open_gadget
        vals = (7, 11)
        _, _, status, verdict = _prove(ctx, lambda cs, x: gp(cs, x, vals), lambda cs, x: gp(cs, x, None), [list(vals)] * 2, _st0s(which.encode(), 2),
                                       _rng(which.encode(), 2), shared=True, gens=gens)
        assert status == bytes(2) and verdict == bytes(2)
    finally:
        ctx.set_option("prover_constant_time", 0)


def test_os_rng_proofs_verify(ctx):
    from bulletproofs_amd import r1cs
    k = 5
    st0 = R.transcript_state(R.T.Transcript(b"ShuffleProofOS"))
    provers = []
    for b in range(3):
        cs = r1cs.Prover(st0)
        xs = [cs.commit(v, x) for v, x in zip(_shuffle(k, b), _scalars(b"os%d" % b, 2 * k))]
        R.shuffle_gadget(cs, xs[:k], xs[k:])
        provers.append(cs)
    out = r1cs.prove_batch(ctx, provers)
    one, V1 = provers[0].prove(ctx)
    assert one.to_bytes() != out[0][0].to_bytes()      # fresh thread_rng bytes per call
    ver = r1cs.Verifier(st0)
    vs = [ver.commit(bytes(32)) for _ in range(2 * k)]
    R.shuffle_gadget(ver, vs[:k], vs[k:])
    circ = ver.circuit()
    proofs = [p.to_bytes() for p, _ in out] + [one.to_bytes()]
    coms = b"".join(b"".join(V) for _, V in out) + b"".join(V1)
    assert circ.verify_batch(ctx, proofs, coms, st0, rng32=None) == bytes(4)


def test_unsatisfied_witness_is_proved_and_rejected(ctx, gens):
    k = 4
    vals = [_shuffle(k, 7, permute=False)]
    _, _, status, verdict = _prove(ctx, _sg(k), _sg(k), vals, _st0s(b"NotAShuffle", 1), _rng(b"bad", 1), gens=gens)
    assert status == bytes(1) and list(verdict) == [R.VERIFICATION_ERROR]


def test_non_canonical_input_voids_that_proof_only(ctx, gens):
    from bulletproofs_amd import r1cs
    k = 3
    st0 = R.transcript_state(R.T.Transcript(b"noncanon"))
    provers = []
    for b in range(3):
        cs = r1cs.Prover(st0)
        xs = [cs.commit(v, x) for v, x in zip(_shuffle(k, b), _scalars(b"bl%d-" % b, 2 * k))]
        R.shuffle_gadget(cs, xs[:k], xs[k:])
        provers.append(cs)
    ins = [p.inputs() for p in provers]
    v = bytearray(b"".join(i[0] for i in ins))
    v[32 * 2 * k + 31] = 0xff                          # proof 1, v_0 >= l
    rng = _rng(b"nc", 3)
    proofs, coms, status = provers[0].witness().prove_batch(ctx, provers[0].circuit(), 3, bytes(v), b"".join(i[1] for i in ins),
                                                             b"".join(i[2] for i in ins), st0, rng)
    assert list(status) == [0, 2, 0]
    for b in (0, 2):
        pf, Vs, _ = P.prove(gens, CAP, st0, _shuffle(k, b), _scalars(b"bl%d-" % b, 2 * k), _sg(k), rng[32 * b:32 * b + 32])
        assert proofs[b] == pf.to_bytes()


def test_generators_too_small(gens):
    import bulletproofs_amd as bp
    from bulletproofs_amd import r1cs
    small = bp.Context(0)
    small.gens_create(8, 1)
    cs = r1cs.Prover(bytes(208))
    x = cs.commit(0x1234, 5)
    R.range_gadget(cs, x, 0x1234, 16)                 # padded_n = 16 > 8
    with pytest.raises(bp.BpgpuError, match="NO_GENS"):
        cs.prove(small)
    assert small.get_option("staging_residue") == 0
    small.close()


def test_prover_leaves_no_secrets_in_the_staging_buffers(ctx):
    """as test_prover_entry_points_leave_no_secrets_in_the_staging_buffers: nothing non-zero left in the pinned block, the IO
    buffer, the working sets or the MSM arena after a call (`staging_residue`)"""
    from bulletproofs_amd import r1cs
    st0 = R.transcript_state(R.T.Transcript(b"zeroize"))
    for ct in (0, 1):
        ctx.set_option("prover_constant_time", ct)
        try:
            provers = []
            for b in range(33):
                cs = r1cs.Prover(st0)
                P.open_gadget(cs, [cs.commit(5, 17 + b), cs.commit(13, 23 + b)], (5, 13))
                provers.append(cs)
            out = r1cs.prove_batch(ctx, provers, _rng(b"z%d" % ct, 33))
            assert ctx.get_option("staging_residue") == 0 and len(out) == 33
        finally:
            ctx.set_option("prover_constant_time", 0)


def test_shuffle_1024_batch(oracle):
    """k = 1024 (padded_n = 2048, m = 2048 commitments per proof): a batch of 4 against the twin, verified on the GPU"""
    import bulletproofs_amd as bp
    g = oracle.Gens(2048, 1).export()
    c = bp.Context(0)
    c.gens_create(2048, 1)
    k = 1024
    vals = [_shuffle(k, 9000 + b) for b in range(4)]
    _, _, status, verdict = _prove(c, _sg(k), _sg(k), vals, _st0s(b"ShuffleProof1024-", 1), _rng(b"big", 4), shared=True, gens=g, cap=2048)
    assert status == bytes(4) and verdict == bytes(4)
    c.close()
