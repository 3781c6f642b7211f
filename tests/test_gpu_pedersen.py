"""Batches of Pedersen commitments and openings on the GPU (bpgpu_pedersen_commit_batch / _open_batch and their _dev forms,
BulletproofGens.commit_batch / verify_openings, bulletproofs.hpp).
CONTRACT (include/bpgpu.h): row i of the commit call equals bpgpu_msm_batch with the two terms (value_i, B), (blinding_i, B_blinding) --
what BulletproofGens.commit returns -- whatever fixed_window_bits and prover_constant_time are."""
import ctypes as C
import os
import subprocess

import pytest

import pedersen_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, NO_GENS = -1, -3
NBATCHES = [1, 63, 64, 65, 257]
SEED24 = bytes([24]) * 32
TS = 208


@pytest.fixture(scope="module")
def contexts():
    """(fixed_window_bits or None, prover_constant_time) -> a context with gens_create(8, 1), made once per module"""
    import bulletproofs_amd as bp
    made = {}

    def get(W=None, ct=0):
        if (W, ct) not in made:
            ctx = bp.Context(0, fixed_window_bits=W) if W else bp.Context(0)
            if ct:
                ctx.set_option("prover_constant_time", 1)
            ctx.gens_create(8, 1)
            made[(W, ct)] = ctx
        return made[(W, ct)]
    yield get
    for ctx in made.values():
        ctx.close()


@pytest.fixture(scope="module")
def bases(oracle):
    _, _, B, Bb = oracle.Gens(8, 1).export()
    return B, Bb


@pytest.fixture(scope="module")
def expected(oracle, bases):
    """the oracle's commitment to a row, computed once per row and shared by the tests of this module"""
    memo = {}

    def get(v, r):
        if (v, r) not in memo:
            memo[(v, r)] = pc.expect(oracle, bases[0], bases[1], v, r)
        return memo[(v, r)]
    return get


def _pack(values, value_bytes):
    return b"".join(v.to_bytes(value_bytes, "little") for v in values)


def _rows(nb):
    rows = pc.rows()
    return [rows[i % len(rows)] for i in range(nb)]


def _split(b):
    return [b[32 * i:32 * i + 32] for i in range(len(b) // 32)]


@pytest.mark.parametrize("value_bytes", [8, 32])
@pytest.mark.parametrize("nb", NBATCHES)
def test_rows_equal_the_two_term_msm_and_the_oracle(contexts, bases, expected, nb, value_bytes):
    ctx = contexts()
    rows = _rows(nb)
    vals, bls = [v for v, _ in rows], b"".join(pc.le32(r) for _, r in rows)
    got, st = ctx.pedersen_commit_batch(_pack(vals, value_bytes), value_bytes, bls)
    assert st == bytes(nb)
    assert _split(got) == [expected(v, r) for v, r in rows]
    ref, rst = ctx.msm_batch([2] * nb, b"".join(pc.le32(v) + pc.le32(r) for v, r in rows), (bases[0] + bases[1]) * nb)
    assert rst == bytes(nb) and got == ref
    assert got[:32] == bytes(32)                                   # (0, 0)


def test_every_row_of_the_matrix_and_the_scalar_only_values(contexts, expected):
    """the whole (value, blinding) matrix in one call, as u64 and as scalars; then 2^64, 2^252, l - 1 as values"""
    ctx = contexts()
    rows = pc.rows()
    bls = b"".join(pc.le32(r) for _, r in rows)
    want = b"".join(expected(v, r) for v, r in rows)
    for vb in (8, 32):
        got, st = ctx.pedersen_commit_batch(_pack([v for v, _ in rows], vb), vb, bls)
        assert st == bytes(len(rows)) and got == want
    rs = pc.blindings()
    rows2 = [(v, rs[(i + 2) % len(rs)]) for i, v in enumerate(pc.SCALAR_ONLY_VALUES)]
    got, st = ctx.pedersen_commit_batch(_pack([v for v, _ in rows2], 32), 32, b"".join(pc.le32(r) for _, r in rows2))
    assert st == bytes(3) and _split(got) == [expected(v, r) for v, r in rows2]


@pytest.mark.parametrize("W,ct", [(5, 0), (8, 0), (11, 0), (None, 1), (8, 1)])
def test_bytes_do_not_depend_on_the_window_or_on_the_constant_time_option(contexts, expected, W, ct):
    ctx = contexts(W, ct)
    assert ctx.get_option("prover_constant_time") == ct and (W is None or ctx.get_option("fixed_window_bits") == W)
    rows = _rows(257)
    bls = b"".join(pc.le32(r) for _, r in rows)
    want = b"".join(expected(v, r) for v, r in rows)
    for vb in (8, 32):
        got, st = ctx.pedersen_commit_batch(_pack([v for v, _ in rows], vb), vb, bls)
        assert st == bytes(257) and got == want
    got, st, bl = ctx.pedersen_commit_batch(_pack(range(8), 8), 8, rng_seed32=SEED24, want_blindings=True)
    assert _split(got) == [expected(j, int.from_bytes(b, "little")) for j, b in enumerate(_split(bl))]


@pytest.mark.parametrize("W,ct", [(None, 0), (8, 1)])
def test_status_bytes_and_the_rows_beside_a_rejected_row(contexts, expected, W, ct):
    ctx = contexts(W, ct)
    rs = pc.blindings()
    vals = [5] * 63 + [pc.L_ORDER, 6, 2**256 - 1, 7] + [8] * 63
    bls = [rs[i % len(rs)] for i in range(len(vals))]
    bls[1], bls[128] = pc.L_ORDER, pc.L_ORDER
    got, st = ctx.pedersen_commit_batch(_pack(vals, 32), 32, b"".join(pc.le32(r) for r in bls))
    for i, (v, r) in enumerate(zip(vals, bls)):
        if v >= pc.L_ORDER or r >= pc.L_ORDER:
            assert st[i] == pc.BAD_SCALAR and got[32 * i:32 * i + 32] == bytes(32), i
        else:
            assert st[i] == pc.OK and got[32 * i:32 * i + 32] == expected(v, r), i
    assert list(st).count(pc.BAD_SCALAR) == 4
    # u64 values beside a non-canonical blinding; the commitment to (0, 0) is 32 zero bytes with status OK
    got, st = ctx.pedersen_commit_batch(_pack([3, 0, 5], 8), 8, pc.le32(1) + pc.le32(pc.L_ORDER) + pc.le32(2))
    assert st == bytes([pc.OK, pc.BAD_SCALAR, pc.OK]) and _split(got) == [expected(3, 1), bytes(32), expected(5, 2)]
    got, st = ctx.pedersen_commit_batch(_pack([0], 8), 8, bytes(32))
    assert st == bytes(1) and got == bytes(32)


def test_seeded_batch_is_the_references_golden_vector(contexts, golden, expected):
    """BulletproofGens.commit_batch(range(8), rng_seed32 = [24] * 32) == the vc[j] and r_j of tests/range_proof.rs:103-113"""
    from bulletproofs_amd import BulletproofGens
    from chacha_rng import chacha20_block, golden_blindings
    gens = BulletproofGens(8, 1)
    coms, bls = gens.commit_batch(range(8), rng_seed32=SEED24)
    assert b"".join(coms) == golden["vc_bytes"] and bls == golden_blindings()
    part, blp = gens.commit_batch(range(3, 8), rng_seed32=SEED24, first_draw=3)
    assert part == coms[3:] and blp == bls[3:]
    gens.ctx.close()
    # the 32-bit counter boundary, on the variable-time and on the constant-time form
    first = 2**32 - 2
    want_bl = [int.from_bytes(chacha20_block(SEED24, first + i), "little") % pc.L_ORDER for i in range(4)]
    for ctx in (contexts(), contexts(8, 1)):
        got, st, bl = ctx.pedersen_commit_batch(_pack([9, 8, 7, 6], 8), 8, rng_seed32=SEED24, first_draw=first, want_blindings=True)
        assert st == bytes(4) and [int.from_bytes(b, "little") for b in _split(bl)] == want_bl
        assert _split(got) == [expected(v, r) for v, r in zip([9, 8, 7, 6], want_bl)]


def test_library_drawn_seed_gives_fresh_blindings_that_open(contexts):
    ctx = contexts()
    vals = _pack(range(100, 170), 8)
    a = ctx.pedersen_commit_batch(vals, 8)
    b = ctx.pedersen_commit_batch(vals, 8)
    assert len(a) == 3 and a[1] == b[1] == bytes(70)
    assert a[2] != b[2] and a[0] != b[0] and len(set(_split(a[2]))) == 70
    assert all(int.from_bytes(x, "little") < pc.L_ORDER for x in _split(a[2]))
    assert ctx.pedersen_open_batch(a[0], vals, 8, a[2]) == bytes(70)
    assert ctx.pedersen_open_batch(b[0], vals, 8, b[2]) == bytes(70)
    assert ctx.pedersen_open_batch(a[0], vals, 8, b[2]) == bytes([pc.VERIFICATION_ERROR]) * 70
    assert ctx.get_option("staging_residue") == 0


@pytest.mark.parametrize("W", [None, 8])
def test_open_verdicts_on_batches_that_mix_all_outcomes(contexts, expected, W):
    ctx = contexts(W)
    rows = pc.rows()
    vals, bls = [v for v, _ in rows], [r for _, r in rows]
    coms = [expected(v, r) for v, r in rows]
    n = len(rows)
    for vb in (8, 32):
        assert ctx.pedersen_open_batch(b"".join(coms), _pack(vals, vb), vb, b"".join(map(pc.le32, bls))) == bytes(n)
    bad = bytes([pc.VERIFICATION_ERROR]) * n
    assert ctx.pedersen_open_batch(b"".join(pc.flip_bit(c, (37 * i) % 256) for i, c in enumerate(coms)), _pack(vals, 8), 8, b"".join(map(pc.le32, bls))) == bad
    assert ctx.pedersen_open_batch(b"".join(coms), _pack([v ^ (1 << ((11 * i) % 64)) for i, v in enumerate(vals)], 8), 8, b"".join(map(pc.le32, bls))) == bad
    flipped = [r ^ (1 << ((13 * i) % 252)) for i, r in enumerate(bls)]
    flipped = [f if f < pc.L_ORDER else r & (r - 1) for f, r in zip(flipped, bls)]
    assert ctx.pedersen_open_batch(b"".join(coms), _pack(vals, 8), 8, b"".join(map(pc.le32, flipped))) == bad
    # the four outcomes in one batch, repeated over more than one wavefront
    unit_c = [coms[5], coms[6], b"\xff" * 32, (1).to_bytes(32, "little"), coms[9], coms[10], bytes(32)]
    unit_v = [vals[5], vals[6] + 1, vals[7], vals[8], pc.L_ORDER, vals[10], 0]
    unit_r = [bls[5], bls[6], bls[7], bls[8], bls[9], pc.L_ORDER, 0]
    unit_want = [pc.OPENS, pc.VERIFICATION_ERROR, pc.VERIFICATION_ERROR, pc.VERIFICATION_ERROR, pc.FORMAT_ERROR, pc.FORMAT_ERROR, pc.OPENS]
    reps = 19                                                              # 133 rows
    got = ctx.pedersen_open_batch(b"".join(unit_c) * reps, _pack(unit_v, 32) * reps, 32, b"".join(map(pc.le32, unit_r)) * reps)
    assert got == bytes(unit_want) * reps


def _to_dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(torch.device("cuda:0"))


@pytest.mark.parametrize("W,ct", [(None, 0), (8, 1)])
def test_device_pointer_forms_on_a_side_stream_give_the_host_forms_bytes(contexts, W, ct):
    import torch
    ctx = contexts(W, ct)
    nb = 130
    rows = _rows(nb)
    v8, v32 = _pack([v for v, _ in rows], 8), _pack([v for v, _ in rows], 32)
    bls = b"".join(pc.le32(r) for _, r in rows)
    want = ctx.pedersen_commit_batch(v8, 8, bls)
    want_seeded = ctx.pedersen_commit_batch(v32, 32, rng_seed32=SEED24, first_draw=5, want_blindings=True)
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream(device=dev)
    d_v8, d_v32, d_bl, d_seed = _to_dev(v8), _to_dev(v32), _to_dev(bls), _to_dev(SEED24)
    full = lambda n: torch.full((n,), 255, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d_c, d_st, d_bo = full(32 * nb), full(nb), full(32 * nb)
        ctx.pedersen_commit_batch_dev(nb, d_v8.data_ptr(), 8, d_bl.data_ptr(), None, 0, d_c.data_ptr(), d_bo.data_ptr(), d_st.data_ptr(), side.cuda_stream)
        d_c2, d_st2, d_bo2 = full(32 * nb), full(nb), full(32 * nb)
        ctx.pedersen_commit_batch_dev(nb, d_v32.data_ptr(), 32, None, d_seed.data_ptr(), 5, d_c2.data_ptr(), d_bo2.data_ptr(), d_st2.data_ptr(), side.cuda_stream)
        d_c3, d_st3, d_bo3 = full(32 * nb), full(nb), full(32 * nb)
        ctx.pedersen_commit_batch_dev(nb, d_v8.data_ptr(), 8, None, None, 0, d_c3.data_ptr(), d_bo3.data_ptr(), d_st3.data_ptr(), side.cuda_stream)
        d_vd, d_vd2, d_vd3 = full(nb), full(nb), full(nb)
        ctx.pedersen_open_batch_dev(nb, d_c.data_ptr(), d_v8.data_ptr(), 8, d_bl.data_ptr(), d_vd.data_ptr(), side.cuda_stream)
        ctx.pedersen_open_batch_dev(nb, d_c3.data_ptr(), d_v32.data_ptr(), 32, d_bo3.data_ptr(), d_vd2.data_ptr(), side.cuda_stream)
        ctx.pedersen_open_batch_dev(nb, d_c2.data_ptr(), d_v8.data_ptr(), 8, d_bo3.data_ptr(), d_vd3.data_ptr(), side.cuda_stream)
    side.synchronize()
    assert ctx.get_option("staging_residue") == 0
    host = lambda t: bytes(t.cpu().numpy())
    assert (host(d_c), host(d_st)) == want and host(d_bo) == bls
    assert (host(d_c2), host(d_st2), host(d_bo2)) == want_seeded
    assert host(d_st3) == bytes(nb) and host(d_c3) != host(d_c) and len(set(_split(host(d_bo3)))) == nb
    assert host(d_vd) == bytes(nb) and host(d_vd2) == bytes(nb) and host(d_vd3) == bytes([pc.VERIFICATION_ERROR]) * nb
    assert ctx.pedersen_open_batch(host(d_c3), v8, 8, host(d_bo3)) == bytes(nb)


def test_commitments_made_on_the_device_feed_the_device_prover(contexts):
    """values and device-drawn blindings stay on the device: bpgpu_pedersen_commit_batch_dev, then bpgpu_rangeproof_prove_batch_ts_dev
    on the same buffers; the proofs verify against the commit call's commitments, which are the prover's own V_j"""
    import torch
    from bulletproofs_amd._lib import transcript_new
    ctx = contexts()
    n, m, nb = 8, 1, 3
    vals = [0, 200, 255]
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream(device=dev)
    state = transcript_new(b"pedersen chaining")
    d_v = torch.tensor(vals, dtype=torch.int64, device=dev)
    d_seed, d_ts, d_rng = _to_dev(SEED24), _to_dev(state), _to_dev(bytes(range(32)) * nb)
    pl = 32 * (9 + 2 * 3)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d_c = torch.zeros(32 * nb, dtype=torch.uint8, device=dev)
        d_bl = torch.zeros(32 * nb, dtype=torch.uint8, device=dev)
        d_st = torch.full((nb,), 255, dtype=torch.uint8, device=dev)
        ctx.pedersen_commit_batch_dev(nb, d_v.data_ptr(), 8, None, d_seed.data_ptr(), 0, d_c.data_ptr(), d_bl.data_ptr(), d_st.data_ptr(), side.cuda_stream)
        d_p = torch.zeros(pl * nb, dtype=torch.uint8, device=dev)
        d_c2 = torch.zeros(32 * nb, dtype=torch.uint8, device=dev)
        ctx.rangeproof_prove_batch_ts_dev(n, m, nb, d_v.data_ptr(), d_bl.data_ptr(), d_ts.data_ptr(), 0, d_rng.data_ptr(), d_p.data_ptr(), d_c2.data_ptr(),
                                          None, side.cuda_stream)
    side.synchronize()
    coms, proofs = bytes(d_c.cpu().numpy()), bytes(d_p.cpu().numpy())
    assert bytes(d_st.cpu().numpy()) == bytes(nb) and coms == bytes(d_c2.cpu().numpy())
    assert bytes(ctx.rangeproof_verify_batch_ts(n, m, proofs, pl, coms, state)) == bytes(nb)


def test_error_returns(contexts):
    import bulletproofs_amd as bp
    ctx = contexts()
    L = bp.lib()
    nb = 3
    v8, v32, bl = _pack([1, 2, 3], 8), _pack([1, 2, 3], 32), pc.le32(4) * nb
    out, blo, st = C.create_string_buffer(32 * nb), C.create_string_buffer(32 * nb), C.create_string_buffer(nb)

    def commit(h=ctx.h, nb_=nb, v=v8, vb=8, bl_=bl, seed=None, first=0, out_=out, blo_=blo, st_=st):
        return L.bpgpu_pedersen_commit_batch(h, nb_, v, vb, bl_, seed, first, out_, blo_, st_)

    def open_(h=ctx.h, nb_=nb, c=out, v=v8, vb=8, bl_=bl, vd=st):
        return L.bpgpu_pedersen_open_batch(h, nb_, c, v, vb, bl_, vd)

    assert commit() == 0 and open_() == 0 and st.raw == bytes(nb)
    assert commit(nb_=0) == 0 and commit(nb_=0, v=None, bl_=None, out_=None, st_=None) == 0 and open_(nb_=0, c=None, v=None, bl_=None, vd=None) == 0
    for vb in (0, 4, 16, 31, 33, 64):
        assert commit(vb=vb) == INVALID_ARG and open_(vb=vb) == INVALID_ARG
    assert b"value_bytes" in L.bpgpu_last_error(ctx.h)
    assert commit(seed=SEED24) == INVALID_ARG and commit(first=1) == INVALID_ARG           # blindings together with a seed / a draw index
    assert commit(bl_=None, seed=SEED24, blo_=None) == 0                                  # the caller's seed: blindings_out optional
    assert commit(blo_=None) == 0                                                         # the caller's blindings: optional too
    assert commit(bl_=None, seed=None, blo_=None) == INVALID_ARG                          # the library's seed: required
    assert b"blindings_out" in L.bpgpu_last_error(ctx.h)
    assert commit(bl_=None, seed=None) == 0
    for kw in (dict(v=None), dict(out_=None), dict(st_=None)):
        assert commit(**kw) == INVALID_ARG, kw
    for kw in (dict(c=None), dict(v=None), dict(bl_=None), dict(vd=None)):
        assert open_(**kw) == INVALID_ARG, kw
    assert commit(h=None) == INVALID_ARG and open_(h=None) == INVALID_ARG
    assert commit(v=v32, vb=32) == 0
    assert ctx.get_option("staging_residue") == 0
    # a context without generators
    bare = bp.Context(0)
    assert commit(h=bare.h) == NO_GENS and open_(h=bare.h) == NO_GENS
    assert L.bpgpu_pedersen_commit_batch_dev(bare.h, nb, 256, 8, 256, None, 0, 256, None, 256, None) == NO_GENS
    assert L.bpgpu_pedersen_open_batch_dev(bare.h, nb, 256, 256, 8, 256, 256, None) == NO_GENS
    assert commit(h=bare.h, nb_=0) == 0
    bare.close()
    # the device forms check what they can without reading device memory
    D = L.bpgpu_pedersen_commit_batch_dev
    assert D(ctx.h, 0, None, 8, None, None, 0, None, None, None, None) == 0
    assert D(ctx.h, nb, 256, 7, 256, None, 0, 256, None, 256, None) == INVALID_ARG
    assert D(ctx.h, nb, 256, 8, 256, 256, 0, 256, None, 256, None) == INVALID_ARG         # blindings and a seed
    assert D(ctx.h, nb, 256, 8, None, None, 0, 256, None, 256, None) == INVALID_ARG       # the library's seed without blindings_out
    assert D(ctx.h, nb, 258, 8, 256, None, 0, 256, None, 256, None) == INVALID_ARG        # misaligned
    assert D(ctx.h, nb, None, 8, 256, None, 0, 256, None, 256, None) == INVALID_ARG
    O = L.bpgpu_pedersen_open_batch_dev
    assert O(ctx.h, 0, None, None, 8, None, None, None) == 0
    assert O(ctx.h, nb, 256, 256, 9, 256, 256, None) == INVALID_ARG and O(ctx.h, nb, 256, 256, 8, None, 256, None) == INVALID_ARG
    assert O(ctx.h, nb, 257, 256, 8, 256, 256, None) == INVALID_ARG
    assert commit() == 0


def test_python_api_matches_commit_row_by_row():
    from bulletproofs_amd import BulletproofGens
    from bulletproofs_amd.api import FormatError, VerificationError
    gens = BulletproofGens(8, 1, fixed_window_bits=8)
    rs = [pc.le32(r) for r in pc.blindings()]
    ints = [0, 1, 2**64 - 1, 2**63, 77, 0x8080808080808080, 5, 6]
    coms, bls = gens.commit_batch(ints, rs)
    assert bls == rs and coms == [gens.commit(v, r) for v, r in zip(ints, rs)]
    scalars = [pc.le32(v) for v in ints[:5] + pc.SCALAR_ONLY_VALUES]
    coms32, _ = gens.commit_batch(scalars, rs)
    assert coms32 == [gens.commit(v, r) for v, r in zip(scalars, rs)] and coms32[:5] == coms[:5]
    seeded, drawn = gens.commit_batch(ints, rng_seed32=SEED24, first_draw=2)
    assert seeded == [gens.commit(v, r) for v, r in zip(ints, drawn)]
    fresh, fresh_bl = gens.commit_batch(ints)
    assert fresh_bl != drawn and gens.verify_openings(fresh, ints, fresh_bl) == [None] * 8
    assert gens.commit_batch([]) == ([], []) and gens.verify_openings([], [], []) == []
    # ValueError for a non-canonical scalar, as commit raises; one kind of value per call
    with pytest.raises(ValueError):
        gens.commit(5, pc.le32(pc.L_ORDER))
    with pytest.raises(ValueError):
        gens.commit_batch([5, 6], [rs[0], pc.le32(pc.L_ORDER)])
    with pytest.raises(ValueError):
        gens.commit_batch([pc.le32(1), pc.le32(pc.L_ORDER)], rs[:2])
    with pytest.raises(ValueError):
        gens.commit_batch([2**64], rs[:1])
    with pytest.raises(ValueError):
        gens.commit_batch([1], rs[:1], rng_seed32=SEED24)
    with pytest.raises(TypeError):
        gens.commit_batch([1, pc.le32(2)], rs[:2])
    # the kinds of ProofError
    bad_c = list(coms)
    bad_c[1], bad_c[2] = pc.flip_bit(coms[1], 3), b"\xff" * 32
    bad_r = list(rs)
    bad_r[4] = pc.le32(pc.L_ORDER)
    res = gens.verify_openings(bad_c, ints, bad_r)
    assert res == [None, VerificationError(), VerificationError(), None, FormatError(), None, None, None]
    assert gens.verify_openings(coms32, scalars, rs) == [None] * 8
    gens.ctx.close()


def test_cpp_mirror_has_the_two_batch_calls(tmp_path):
    """include/bulletproofs.hpp: BulletproofGens::commit_batch / verify_openings"""
    exe, csrc = str(tmp_path / "pedersen_test"), os.path.join(ROOT, "bulletproofs_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "pedersen_test.cpp"),
                           "-L", csrc, "-lbpgpu", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout
