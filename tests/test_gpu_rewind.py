"""Rewindable range proofs on the GPU (bpgpu_rangeproof_prove_batch_rw / _rewind_batch, RangeProof.prove_batch(rewind=True) /
rewind_batch / rewind_single / rewind_seeds, bulletproofs.hpp) at n = 8 and n = 64.
CONTRACT (include/bpgpu.h): row p of the rewindable prover equals bpgpu_rangeproof_prove_batch(nbatch = 1, shared_transcript =
transcripts[p], rng = keystream blocks 0 .. 2n+3 of the seed with block 0 replaced by the canonical bytes of (d_0 - e) mod l); at n = 8
the bytes are also tests/rewind_twin.py's.  Batches have 1, 63, 65 and 130 rows: lane 0 alone, the lanes past the batch, a second and a
third workgroup.  One state per row over STROBE positions 0, 100, 150 and 165, and one shared state."""
import ctypes as C
import hashlib
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1
SIZES = [1, 63, 65, 130]
NB = 130
POSITIONS = (0, 100, 150, 165)
TS = 208
NS = [8, 64]
TWIN_ROWS = 12          # rows of the n = 8 batch that are also proved by the Python twin
OK, NOT_FOUND, FORMAT = 0, 1, 2


def _pl(n):
    return 32 * (9 + 2 * (n.bit_length() - 1))


@pytest.fixture(scope="module")
def tw(oracle):
    import rewind_twin
    return rewind_twin


@pytest.fixture(scope="module")
def contexts():
    """prover_constant_time -> a context with gens_create(64, 1), made once per module"""
    import bulletproofs_amd as bp
    made = {}

    def get(ct=0):
        if ct not in made:
            ctx = bp.Context(0)
            if ct:
                ctx.set_option("prover_constant_time", 1)
            ctx.gens_create(64, 1)
            made[ct] = ctx
        return made[ct]
    yield get
    for ctx in made.values():
        ctx.close()


@pytest.fixture(scope="module")
def ref(tw, contexts):
    """Per n: 130 statements, computed once and left unchanged -- values 0, 1, 2^n - 1 (and 2^63 at n = 64) and others below 2^n,
    blindings 0, 1, l - 1 and random ones, the message absent, zero, sixteen 0xff bytes and random ones, row 0 = (0, 0) whose V is 32
    zero bytes; one of four states per row -- with the rewindable prover's proofs and commitments from ONE call on the default context"""
    states = [tw.state_at(pos, b"wallet") for pos in POSITIONS]
    out = {"states": states, "shared": tw.state_at(150, b"shared")}
    for n in NS:
        vs = [0, 1, 2**n - 1] + ([2**63] if n == 64 else [])
        gs = [0, 1, tw.L - 1]
        ms = [None, bytes(16), b"\xff" * 16]
        rows = []
        for i in range(NB):
            v = vs[i] if i < len(vs) else tw.det_scalar(b"v%d" % n, i) % 2**n
            g = gs[i] if i < 3 else tw.det_scalar(b"g%d" % n, i)
            msg = ms[i % 3] if i < 9 else hashlib.sha256(b"msg%d" % i).digest()[:16]
            if i == 4:
                v, g, msg = 2**n - 1, tw.L - 1, b"\xff" * 16
            rows.append(dict(v=v, g=g, msg=msg, state=states[i % 4], seed=tw.det_seed(b"n%d" % n, i)))
        proofs, coms = _prove(contexts(), n, rows)
        pl = _pl(n)
        for i, r in enumerate(rows):
            r["proof"], r["V"] = proofs[pl * i:pl * i + pl], coms[32 * i:32 * i + 32]
        assert rows[0]["V"] == bytes(32)
        out[n] = rows
    return out


def _msgs(rows):
    return b"".join(r["msg"] or bytes(16) for r in rows)


def _prove(ctx, n, rows, states=None, messages=True):
    return ctx.rangeproof_prove_batch_rw(n, 1, [r["v"] for r in rows], b"".join(r["g"].to_bytes(32, "little") for r in rows),
                                         states if states is not None else b"".join(r["state"] for r in rows), b"".join(r["seed"] for r in rows),
                                         _msgs(rows) if messages else None)


def _rewind(ctx, n, rows, states=None):
    st, vals, msgs, bls = ctx.rangeproof_rewind_batch(n, b"".join(r["proof"] for r in rows), _pl(n), b"".join(r["V"] for r in rows),
                                                      states if states is not None else b"".join(r["state"] for r in rows), b"".join(r["seed"] for r in rows))
    return [(st[i], vals[i], msgs[16 * i:16 * i + 16], int.from_bytes(bls[32 * i:32 * i + 32], "little")) for i in range(len(rows))]


def _want(rows):
    return [(OK, r["v"], r["msg"] or bytes(16), r["g"]) for r in rows]


# ---- the prover -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_rewindable_proofs_equal_the_contract_call(contexts, tw, ref, n):
    """the contract: bpgpu_rangeproof_prove_batch with the seed's keystream and block 0 replaced -- nbatch = 1 for the first rows, and
    every row in one call per start state; prover_constant_time gives the same bytes; so do the prefixes of 1, 63 and 65 rows"""
    rows, ctx = ref[n], contexts()
    pl = _pl(n)
    rng = [tw.contract_rng(n, r["seed"], tw.payload(r["v"], r["msg"])) for r in rows]
    bl = [r["g"].to_bytes(32, "little") for r in rows]
    for i in range(5):
        p, c = ctx.rangeproof_prove_batch(n, 1, [rows[i]["v"]], bl[i], transcript=rows[i]["state"], rng=rng[i])
        assert (p, c) == (rows[i]["proof"], rows[i]["V"]), i
    for s in range(4):
        idx = list(range(s, NB, 4))
        p, c = ctx.rangeproof_prove_batch(n, 1, [rows[i]["v"] for i in idx], b"".join(bl[i] for i in idx), transcript=ref["states"][s],
                                          rng=b"".join(rng[i] for i in idx))
        for k, i in enumerate(idx):
            assert (p[pl * k:pl * k + pl], c[32 * k:32 * k + 32]) == (rows[i]["proof"], rows[i]["V"]), i
    want = (b"".join(r["proof"] for r in rows), b"".join(r["V"] for r in rows))
    assert _prove(contexts(1), n, rows) == want
    for nb in SIZES[:3]:
        assert _prove(ctx, n, rows[:nb]) == (want[0][:pl * nb], want[1][:32 * nb]), nb


def test_rewindable_proofs_equal_the_twin_at_n_8(tw, ref):
    T = tw.T
    bp_gens, pc = T.BulletproofGens(8, 1), T.PedersenGens()
    for i, r in enumerate(ref[8][:TWIN_ROWS]):
        assert tw.prove(bp_gens, pc, r["state"], r["v"], r["g"], 8, r["seed"], r["msg"])[:2] == (r["proof"], r["V"]), i


@pytest.mark.parametrize("n", NS)
def test_one_shared_state_no_messages_and_the_dev_prover(contexts, tw, ref, n):
    """stride 0 equals per-row copies of the state; messages = NULL equals zero messages; the _dev form equals the host form"""
    import torch
    ctx, rows = contexts(), ref[n][:65]
    shared = ref["shared"]
    a = _prove(ctx, n, rows, states=shared)
    assert a == _prove(ctx, n, rows, states=shared * len(rows))
    zero = [dict(r, msg=None) for r in rows]
    assert _prove(ctx, n, zero, messages=False) == _prove(ctx, n, zero)
    dev = torch.device("cuda:0")
    up = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)
    nb, pl = len(rows), _pl(n)
    d_v = torch.tensor([r["v"] - (1 << 64) if r["v"] >> 63 else r["v"] for r in rows], dtype=torch.int64, device=dev)
    d_bl, d_ts, d_seed, d_msg = up(b"".join(r["g"].to_bytes(32, "little") for r in rows)), up(shared), up(b"".join(r["seed"] for r in rows)), up(_msgs(rows))
    d_pr, d_cm = torch.full((pl * nb,), 255, dtype=torch.uint8, device=dev), torch.full((32 * nb,), 255, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.rangeproof_prove_batch_rw_dev(n, 1, nb, d_v.data_ptr(), d_bl.data_ptr(), d_ts.data_ptr(), 0, d_seed.data_ptr(), d_msg.data_ptr(), d_pr.data_ptr(),
                                      d_cm.data_ptr())
    ctx.synchronize()
    assert (bytes(d_pr.cpu().numpy()), bytes(d_cm.cpu().numpy())) == a


@pytest.mark.parametrize("n", NS)
def test_rewindable_proofs_verify(contexts, oracle, ref, n):
    """ordinary proofs: verdict Ok from bpgpu_rangeproof_verify_batch_ts and from the oracle's verify_ts"""
    rows = ref[n]
    v = contexts().rangeproof_verify_batch_ts(n, 1, b"".join(r["proof"] for r in rows), _pl(n), b"".join(r["V"] for r in rows), b"".join(r["state"] for r in rows))
    assert bytes(v) == bytes(NB)
    g = oracle.Gens(64, 1)
    rng64 = hashlib.shake_256(b"rewind verify").digest(64)
    for i, r in enumerate(rows):
        assert oracle.verify_ts(g, r["proof"], r["V"], n, r["state"], rng64)[0] == 0, i


# ---- the rewinder -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", SIZES)
@pytest.mark.parametrize("n", NS)
def test_rewind_returns_every_row(contexts, ref, n, nb):
    """(v, gamma, msg) of every row, on the default context and with prover_constant_time, and from the _dev form"""
    import torch
    rows = ref[n][:nb]
    want = _want(rows)
    assert _rewind(contexts(), n, rows) == want
    assert _rewind(contexts(1), n, rows) == want
    dev = torch.device("cuda:0")
    up = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)
    d_pr, d_cm, d_ts, d_seed = (up(b"".join(r[k] for r in rows)) for k in ("proof", "V", "state", "seed"))
    d_st, d_m, d_g = (torch.full((k * nb,), 255, dtype=torch.uint8, device=dev) for k in (1, 16, 32))
    d_v = torch.full((nb,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    for ct in (0, 1):
        ctx = contexts(ct)
        ctx.rangeproof_rewind_batch_dev(n, nb, d_pr.data_ptr(), _pl(n), d_cm.data_ptr(), d_ts.data_ptr(), TS, d_seed.data_ptr(), d_st.data_ptr(), d_v.data_ptr(),
                                        d_m.data_ptr(), d_g.data_ptr())
        ctx.synchronize()
        st, m, g = (bytes(t.cpu().numpy()) for t in (d_st, d_m, d_g))
        vals = [x % 2**64 for x in d_v.cpu().tolist()]
        assert [(st[i], vals[i], m[16 * i:16 * i + 16], int.from_bytes(g[32 * i:32 * i + 32], "little")) for i in range(nb)] == want, ct


@pytest.mark.parametrize("n", NS)
def test_rewind_from_one_shared_state(contexts, ref, n):
    rows = [dict(r) for r in ref[n][:65]]
    shared = ref["shared"]
    proofs, coms = _prove(contexts(), n, rows, states=shared)
    pl = _pl(n)
    for i, r in enumerate(rows):
        r["proof"], r["V"] = proofs[pl * i:pl * i + pl], coms[32 * i:32 * i + 32]
    for ct in (0, 1):
        assert _rewind(contexts(ct), n, rows, states=shared) == _want(rows)
    assert _rewind(contexts(), n, rows[:1], states=shared) == _want(rows[:1])


@pytest.mark.parametrize("n", NS)
def test_each_way_to_miss_stands_alone_among_good_rows(contexts, tw, ref, n):
    """One bad row per batch of 130, at the batch's start, a workgroup edge or its end; every other row's result must not move, and a row
    that is not OK has all-zero outputs.  e_blinding + 1 sits on a row with v >= 1: step 3 passes (e - 1 < 2^192), step 5 does not."""
    good = ref[n]
    pl = _pl(n)
    lb = tw.L.to_bytes(32, "little")
    bump = lambda b, off: b[:off] + ((int.from_bytes(b[off:off + 32], "little") + 1) % tw.L).to_bytes(32, "little") + b[off + 32:]
    seeded = contexts().rangeproof_prove_batch_ts(n, 1, [good[64]["v"]], good[64]["g"].to_bytes(32, "little"), good[64]["state"], good[64]["seed"])
    cases = [
        ("wrong seed", 0, lambda r: r.update(seed=tw.det_seed(b"other", 0)), NOT_FOUND),
        ("e_blinding + 1", 4, lambda r: r.update(proof=bump(r["proof"], 192)), NOT_FOUND),
        ("t_x_blinding + 1", 63, lambda r: r.update(proof=bump(r["proof"], 160)), NOT_FOUND),
        ("wrong transcript", 64, lambda r: r.update(state=tw.state_at(100, b"someone else")), NOT_FOUND),
        ("another row's commitment", 65, lambda r: r.update(V=good[66]["V"]), NOT_FOUND),
        ("A of 32 zero bytes", 129, lambda r: r.update(proof=bytes(32) + r["proof"][32:]), NOT_FOUND),
        ("e_blinding = l", 1, lambda r: r.update(proof=r["proof"][:192] + lb + r["proof"][224:]), FORMAT),
        ("a = l", 128, lambda r: r.update(proof=r["proof"][:pl - 64] + lb + r["proof"][pl - 32:]), FORMAT),
        ("an ordinary seeded proof under its own seed", 64, lambda r: r.update(proof=seeded[0], V=seeded[1]), NOT_FOUND),
    ]
    assert good[4]["v"] >= 1 and (tw.payload(good[4]["v"], good[4]["msg"]) - 1) >> 192 == 0
    want = _want(good)
    for name, at, change, status in cases:
        rows = [dict(r) for r in good]
        change(rows[at])
        for ct in (0, 1):
            got = _rewind(contexts(ct), n, rows)
            assert got[at] == (status, 0, bytes(16), 0), (name, ct)
            assert got[:at] + got[at + 1:] == want[:at] + want[at + 1:], (name, ct)
    if n == 8:   # the twin agrees on every miss
        pc = tw.T.PedersenGens()
        for name, at, change, status in cases:
            r = dict(good[at])
            change(r)
            assert tw.rewind(pc, r["state"], r["proof"], r["V"], n, r["seed"])[0] == status, name


def test_a_batch_where_no_row_is_the_wallets(contexts, tw, ref):
    """wrong seeds everywhere: whole wavefronts skip the walk; every status NOT_FOUND, every output zero"""
    rows = [dict(r, seed=tw.det_seed(b"stranger", i)) for i, r in enumerate(ref[64])]
    for ct in (0, 1):
        assert _rewind(contexts(ct), 64, rows) == [(NOT_FOUND, 0, bytes(16), 0)] * NB


# ---- arguments ----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_anything_is_staged(contexts, ref):
    import bulletproofs_amd as bp
    ctx, L = contexts(), bp.lib()
    b = lambda n: C.create_string_buffer(n)
    r = ref[8][1]
    ts, pr, cm, seed = r["state"], r["proof"], r["V"], r["seed"]
    st, vo, mo, go = b(1), (C.c_uint64 * 1)(), b(16), b(32)
    va = (C.c_uint64 * 2)(1, 1)
    assert L.bpgpu_rangeproof_rewind_batch(ctx.h, 8, 1, pr, len(pr), cm, ts, 0, seed, st, vo, mo, go) == 0 and st.raw[0] == OK and vo[0] == r["v"]
    for n, pl, stride in ((8, len(pr) + 32, 0), (8, len(pr) - 64, 0), (8, len(pr), 104), (7, len(pr), 0), (64, len(pr), 0)):
        assert L.bpgpu_rangeproof_rewind_batch(ctx.h, n, 1, pr, pl, cm, ts, stride, seed, st, vo, mo, go) == INVALID_ARG, (n, pl, stride)
        assert L.bpgpu_rangeproof_rewind_batch_dev(ctx.h, n, 1, 256, pl, 512, 768, stride, 1024, 1280, 1536, 1792, 2048, None) == INVALID_ARG, (n, pl, stride)
    bad = ts[:200] + bytes([200]) + ts[201:]
    assert L.bpgpu_rangeproof_rewind_batch(ctx.h, 8, 1, pr, len(pr), cm, bad, 0, seed, st, vo, mo, go) == INVALID_ARG
    assert L.bpgpu_rangeproof_rewind_batch(ctx.h, 8, 0, None, len(pr), None, ts, 0, None, None, None, None, None) == 0
    assert L.bpgpu_rangeproof_rewind_batch(ctx.h, 8, 1, pr, len(pr), cm, ts, 0, None, st, vo, mo, go) == INVALID_ARG
    po, co = b(64 * 32), b(64)
    for m in (2, 4, 0):
        assert L.bpgpu_rangeproof_prove_batch_rw(ctx.h, 8, m, 1, va, bytes(64), ts, 0, seed, None, po, co, None) == INVALID_ARG, m
        assert L.bpgpu_rangeproof_prove_batch_rw_dev(ctx.h, 8, m, 1, 256, 512, 768, 0, 1024, None, 1280, 1536, None, None) == INVALID_ARG, m
    assert L.bpgpu_rangeproof_prove_batch_rw(ctx.h, 8, 1, 1, va, bytes(32), ts, 0, None, None, po, co, None) == INVALID_ARG      # no seed: nothing to rewind with
    assert L.bpgpu_rangeproof_prove_batch_rw(ctx.h, 8, 1, 1, va, bytes(32), ts, 104, seed, None, po, co, None) == INVALID_ARG
    assert L.bpgpu_rangeproof_prove_batch_rw(ctx.h, 8, 1, 0, None, None, None, 0, None, None, None, None, None) == 0
    empty = bp.Context(0)
    try:
        assert L.bpgpu_rangeproof_rewind_batch(empty.h, 8, 1, pr, len(pr), cm, ts, 0, seed, st, vo, mo, go) == -3      # BPGPU_ERR_NO_GENS
    finally:
        empty.close()


# ---- the Python surface -------------------------------------------------------------------------------------------------------------
def test_rewind_seeds_equal_the_host_transcript_helpers(contexts, tw, ref):
    import bulletproofs_amd as bp
    from bulletproofs_amd._lib import transcript_append_message, transcript_challenge_bytes, transcript_new
    key = hashlib.sha256(b"wallet key").digest()
    coms = [r["V"] for r in ref[64][:65]]
    seeds = bp.RangeProof.rewind_seeds(contexts(), key, coms)
    assert len(seeds) == 32 * len(coms)
    for i, c in enumerate(coms):
        st = transcript_append_message(transcript_append_message(transcript_new(b"bpgpu rewind seed v1"), b"key", key), b"C", c)
        assert transcript_challenge_bytes(st, b"seed", 32)[1] == seeds[32 * i:32 * i + 32], i
        if i < 3:
            assert tw.seed_for(key, c) == seeds[32 * i:32 * i + 32]
    assert bp.RangeProof.rewind_seeds(contexts(), key, []) == b""


def test_api_prove_rewind_and_format_errors(tw):
    """RangeProof.prove_batch(rewind=True) / rewind_batch / rewind_single over a list of Transcript, one bound Transcript and a
    TranscriptBatch; without the keywords prove_batch is the seeded call, byte for byte; a FORMAT row raises as from_bytes would"""
    import bulletproofs_amd as bp
    gens = bp.BulletproofGens(64, 1)
    try:
        pc, n, nb = gens.pedersen(), 64, 5
        key = hashlib.sha256(b"api wallet").digest()
        vals = [[0], [1], [2**64 - 1], [2**63], [12345]]
        bls = [[tw.det_scalar(b"api", i).to_bytes(32, "little")] for i in range(nb)]
        msgs = [None, bytes(16), b"\xff" * 16, b"memo: rent, May.", None]
        coms = [gens.ctx.pedersen_commit_batch(v[0].to_bytes(8, "little"), 8, b[0])[0] for v, b in zip(vals, bls)]
        seeds = bp.RangeProof.rewind_seeds(gens, key, coms)
        mk = lambda: [bp.Transcript(b"api rewind %d" % (i % 2)) for i in range(nb)]
        out = bp.RangeProof.prove_batch(gens, pc, mk(), vals, bls, n, rng32=seeds, rewind=True, messages=msgs)
        assert [c[0] for _, c in out] == coms
        proofs = [p for p, _ in out]
        assert bp.RangeProof.verify_batch(gens, pc, mk(), proofs, [[c] for c in coms], n) == [None] * nb
        want = [(v[0], b[0], m or bytes(16)) for v, b, m in zip(vals, bls, msgs)]
        assert bp.RangeProof.rewind_batch(gens, pc, mk(), proofs, coms, n, seeds) == want
        assert bp.RangeProof.rewind_batch(gens, pc, bp.TranscriptBatch.from_states(gens, mk()), proofs, coms, n, seeds) == want
        assert proofs[2].rewind_single(gens, pc, mk()[2], coms[2], n, seeds[64:96]) == want[2]
        assert proofs[2].rewind_single(gens, pc, mk()[2], coms[2], n, seeds[32:64]) is None
        other = bp.RangeProof.rewind_seeds(gens, hashlib.sha256(b"another wallet").digest(), coms)
        mixed = seeds[:64] + other[64:128] + seeds[128:]
        assert bp.RangeProof.rewind_batch(gens, pc, mk(), proofs, coms, n, mixed) == want[:2] + [None, None] + want[4:]
        one = bp.Transcript(b"api rewind shared")
        shared = bp.RangeProof.prove_batch(gens, pc, one, vals, bls, n, rng32=seeds, rewind=True)
        assert bp.RangeProof.rewind_batch(gens, pc, one, [p for p, _ in shared], coms, n, seeds) == [(v[0], b[0], bytes(16)) for v, b in zip(vals, bls)]
        # without the keywords: today's call
        plain = bp.RangeProof.prove_batch(gens, pc, mk(), vals, bls, n, rng32=seeds)
        raw, rc = gens.ctx.rangeproof_prove_batch_ts(n, 1, [v[0] for v in vals], b"".join(b[0] for b in bls), b"".join(t.state for t in mk()), seeds)
        assert b"".join(p.to_bytes() for p, _ in plain) == raw and b"".join(c[0] for _, c in plain) == rc
        # ... whose proofs do not rewind -- but for the value 0, where e = 0 and the seeded proof IS the rewindable one without a message
        assert bp.RangeProof.rewind_batch(gens, pc, mk(), [p for p, _ in plain], coms, n, seeds) == [(0, bls[0][0], bytes(16))] + [None] * (nb - 1)
        bad = proofs[1].to_bytes()
        bad = bad[:192] + tw.L.to_bytes(32, "little") + bad[224:]
        with pytest.raises(bp.FormatError):
            bp.RangeProof.from_bytes(bad)
        with pytest.raises(bp.FormatError):
            bp.RangeProof.rewind_batch(gens, pc, mk(), [proofs[0], bad] + proofs[2:], coms, n, seeds)
        with pytest.raises(bp.FormatError):
            bp.RangeProof.rewind_batch(gens, pc, mk(), [p.to_bytes()[:-64] for p in proofs], coms, n, seeds)
        with pytest.raises(ValueError):
            bp.RangeProof.prove_batch(gens, pc, mk(), [v + v for v in vals], [b + b for b in bls], n, rng32=seeds, rewind=True)
        with pytest.raises(ValueError):
            bp.RangeProof.prove_batch(gens, pc, mk(), vals, bls, n, rewind=True)
    finally:
        gens.ctx.close()


def test_cpp_mirror_proves_verifies_and_rewinds(tmp_path):
    """include/bulletproofs.hpp: RangeProof::prove_batch_rewindable / rewind_batch / rewind_single / rewind_seeds"""
    exe, csrc = str(tmp_path / "range_proof_rewind_test"), os.path.join(ROOT, "bulletproofs_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "range_proof_rewind_test.cpp"),
                           "-L", csrc, "-lbpgpu", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout
