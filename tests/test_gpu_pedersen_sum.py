"""Signed sums of Pedersen commitments and the balance check on the GPU (bpgpu_pedersen_sum_batch / _balance_batch and their _dev
forms, BulletproofGens.sum_commitments / verify_balance, bulletproofs.hpp).
CONTRACTS (include/bpgpu.h): (a) row r of the sum call equals bpgpu_msm_batch on (+-1, C_i) ..., (value, B), (blinding, B_blinding);
(b) a row without terms equals row r of bpgpu_pedersen_commit_batch; (c) a balance row with exactly one added term has the verdict of
bpgpu_pedersen_open_batch -- whatever fixed_window_bits and prover_constant_time are."""
import ctypes as C
import os
import subprocess

import pytest

import pedersen_cases as pc
import pedersen_sum_cases as sc
import point_corpus as corpus

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, NO_GENS = -1, -3


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
def batch(oracle, bases):
    """the pattern and the long row in ONE batch, and the oracle's rows for it, computed once: (offsets, points, values, blindings) and
    expected(sign mode, with scalars) -> encodings"""
    lengths = sc.ROWS + [sc.LONG_ROW, 2]
    off = sc.offsets(lengths)
    vals, bls = sc.scalars(len(lengths))
    pts = sc.points(off[-1], shift=5)
    memo = {}

    def expected(mode, with_scalars):
        if (mode, with_scalars) not in memo:
            memo[(mode, with_scalars)] = sc.expect_rows(oracle, bases[0], bases[1], off, pts, sc.signs(mode, off[-1]), vals if with_scalars else None,
                                                        bls if with_scalars else None)
        return memo[(mode, with_scalars)]
    return (off, pts, vals, bls), expected


def _split(b):
    return [b[32 * i:32 * i + 32] for i in range(len(b) // 32)]


def _bl(bls):
    return b"".join(pc.le32(b) for b in bls)


def test_the_whole_pattern_equals_the_oracle(contexts, batch):
    """every row length of the pattern and the row that takes a reduce pass, every sign mode; u64 values, scalar values, no scalars"""
    ctx = contexts()
    (off, pts, vals, bls), expected = batch
    nb, flat = len(off) - 1, b"".join(pts)
    for mode in sc.SIGN_MODES:
        sg = sc.signs(mode, off[-1])
        got, st = ctx.pedersen_sum_batch(off, flat, sg)
        assert st == bytes(nb) and _split(got) == expected(mode, False), mode
        for vb in (8, 32):
            got, st = ctx.pedersen_sum_batch(off, flat, sg, sc.pack(vals, vb), vb, _bl(bls))
            assert st == bytes(nb) and _split(got) == expected(mode, True), (mode, vb)
    # one scalar of the two: the other is zero
    got, st = ctx.pedersen_sum_batch(off, flat, None, sc.pack(vals, 8), 8, None)
    got0, st0 = ctx.pedersen_sum_batch(off, flat, None, sc.pack(vals, 8), 8, bytes(32 * nb))
    assert st == st0 == bytes(nb) and got == got0
    got, st = ctx.pedersen_sum_batch(off, flat, None, None, 8, _bl(bls))
    got0, st0 = ctx.pedersen_sum_batch(off, flat, None, bytes(8 * nb), 8, _bl(bls))
    assert st == st0 == bytes(nb) and got == got0
    assert ctx.get_option("staging_residue") == 0


def test_contract_a_the_msm_route_gives_the_same_bytes(contexts, batch, bases):
    ctx = contexts()
    (off, pts, vals, bls), _ = batch
    sg = sc.signs("alternating", off[-1])
    got, st = ctx.pedersen_sum_batch(off, b"".join(pts), sg, sc.pack(vals, 8), 8, _bl(bls))
    n_terms, scalars, points = sc.msm_route(off, pts, sg, vals, bls, bases[0], bases[1])
    ref, rst = ctx.msm_batch(n_terms, scalars, points)
    assert rst == st == bytes(len(off) - 1) and got == ref


def test_contract_b_a_row_without_terms_is_the_commitment(contexts, batch):
    ctx = contexts()
    (off, pts, vals, bls), _ = batch
    nb = len(off) - 1
    got, st = ctx.pedersen_sum_batch(off, b"".join(pts), None, sc.pack(vals, 8), 8, _bl(bls))
    com, cst = ctx.pedersen_commit_batch(sc.pack(vals, 8), 8, _bl(bls))
    empty = [r for r in range(nb) if off[r] == off[r + 1]]
    assert len(empty) >= 3 and st == cst == bytes(nb)
    assert [_split(got)[r] for r in empty] == [_split(com)[r] for r in empty]
    # a call of empty rows only: every row
    got, st = ctx.pedersen_sum_batch([0] * (nb + 1), b"", None, sc.pack(vals, 32), 32, _bl(bls))
    assert (got, st) == (com, cst)
    assert ctx.pedersen_sum_batch([0] * 4, b"") == (bytes(96), bytes(3))
    assert ctx.pedersen_balance_batch([0] * 4, b"") == bytes(3)


def test_contract_c_one_added_term_has_the_open_calls_verdict(contexts, oracle, bases):
    ctx = contexts()
    rows = pc.rows()
    vals, bls = [v for v, _ in rows], [r for _, r in rows]
    coms = [pc.expect(oracle, bases[0], bases[1], v, r) for v, r in rows]
    n = len(rows)
    off = list(range(n + 1))

    def both(c, v, vb, b):
        a = ctx.pedersen_open_batch(b"".join(c), sc.pack(v, vb), vb, _bl(b))
        mine = ctx.pedersen_balance_batch(off, b"".join(c), None, sc.pack(v, vb), vb, _bl(b))
        assert mine == a
        return mine
    assert both(coms, vals, 8, bls) == bytes(n) and both(coms, vals, 32, bls) == bytes(n)
    assert both([pc.flip_bit(c, (37 * i) % 256) for i, c in enumerate(coms)], vals, 8, bls) == bytes([sc.VERIFICATION_ERROR]) * n
    assert both(coms, [v ^ (1 << ((11 * i) % 64)) for i, v in enumerate(vals)], 8, bls) == bytes([sc.VERIFICATION_ERROR]) * n
    mc, mv, mb = list(coms), list(vals), list(bls)
    mc[2], mc[3] = b"\xff" * 32, (1).to_bytes(32, "little")
    mv[4], mb[5] = pc.L_ORDER, pc.L_ORDER
    mc[6], mv[6] = corpus.REJECT_ENC[1], 2**256 - 1
    got = both(mc, mv, 32, mb)
    assert got[:7] == bytes([0, 0, 1, 1, 2, 2, 2]) and got[7:] == bytes(n - 7)


@pytest.mark.parametrize("W,ct", [(7, 0), (13, 0), (None, 1), (7, 1)])
def test_bytes_do_not_depend_on_the_window_or_on_the_constant_time_option(contexts, batch, W, ct):
    ctx = contexts(W, ct)
    assert ctx.get_option("prover_constant_time") == ct and (W is None or ctx.get_option("fixed_window_bits") == W)
    (off, pts, vals, bls), expected = batch
    nb = len(off) - 1
    sg = sc.signs("alternating", off[-1])
    for vb in (8, 32):
        got, st = ctx.pedersen_sum_batch(off, b"".join(pts), sg, sc.pack(vals, vb), vb, _bl(bls))
        assert st == bytes(nb) and _split(got) == expected("alternating", True)
    got, st = ctx.pedersen_sum_batch(off, b"".join(pts), sg)
    assert st == bytes(nb) and _split(got) == expected("alternating", False)


@pytest.mark.parametrize("nb", [1, 63, 64, 65, 257])
def test_row_counts_at_the_finish_launchs_lane_boundaries(contexts, oracle, bases, nb):
    """three-term rows (+, -, +) with a u64 value and a blinding: the sum against the oracle row by row, and its own balance"""
    ctx = contexts()
    off = [3 * r for r in range(nb + 1)]
    pts = sc.points(3 * nb, shift=nb)
    sg = b"\0\1\0" * nb
    vals, bls = sc.scalars(nb)
    got, st = ctx.pedersen_sum_batch(off, b"".join(pts), sg, sc.pack(vals, 8), 8, _bl(bls))
    assert st == bytes(nb) and _split(got) == sc.expect_rows(oracle, bases[0], bases[1], off, pts, sg, vals, bls)
    # the sum moved to the other side: terms - (terms + O) + O == 0, so the row (C_1, -C_2, C_3, -sum) balances against minus the opening
    off4 = [4 * r for r in range(nb + 1)]
    pts4 = [e for r in range(nb) for e in pts[3 * r:3 * r + 3] + [_split(got)[r]]]
    neg = lambda x: (pc.L_ORDER - x) % pc.L_ORDER
    vd = ctx.pedersen_balance_batch(off4, b"".join(pts4), b"\0\1\0\1" * nb, sc.pack([neg(v) for v in vals], 32), 32, _bl([neg(b) for b in bls]))
    assert vd == bytes(nb)
    wrong = ctx.pedersen_balance_batch(off4, b"".join(pts4), b"\0\1\0\1" * nb, sc.pack([neg(v + 1) for v in vals], 32), 32, _bl([neg(b) for b in bls]))
    assert wrong == bytes([sc.VERIFICATION_ERROR]) * nb


def test_each_rejection_class_alone_in_a_row(contexts, oracle, bases):
    ctx = contexts()
    lengths, pts, flags = sc.reject_rows()
    off = sc.offsets(lengths)
    sg = sc.signs("alternating", off[-1])
    got, st = ctx.pedersen_sum_batch(off, b"".join(pts), sg)
    vd = ctx.pedersen_balance_batch(off, b"".join(pts), sg)
    got = _split(got)
    for r, rejected in enumerate(flags):
        if rejected:
            assert (st[r], got[r], vd[r]) == (sc.BAD_POINT, bytes(32), sc.VERIFICATION_ERROR), corpus.REJECT[r // 2][0]
        else:
            s, e = sc.expect_row(oracle, bases[0], bases[1], pts[off[r]:off[r + 1]], sg[off[r]:off[r + 1]])
            assert s == 0 and (st[r], got[r]) == (sc.OK, e), r
    acc = corpus.ACCEPT_ENC
    off = sc.offsets([1] * len(acc) + [2] * len(acc))
    got, st = ctx.pedersen_sum_batch(off, b"".join(acc + [e for e in acc for _ in range(2)]), bytes(len(acc)) + b"\0\1" * len(acc))
    assert st == bytes(2 * len(acc)) and _split(got) == acc + [bytes(32)] * len(acc)


@pytest.mark.parametrize("ct", [0, 1])
def test_rejected_scalars_take_precedence_over_a_rejected_point(contexts, oracle, bases, ct):
    ctx = contexts(None, ct)
    p = sc.pool()
    bad_point = corpus.REJECT_ENC[0]
    off = sc.offsets([2] * 6)
    pts = [p[0], p[1], p[2], p[3], p[4], bad_point, p[5], p[6], bad_point, p[7], p[8], p[9]]
    for bad in pc.REJECTED_SCALARS:
        vals = [5, bad, bad, 6, 7, 8]
        bls = [1, 2, 3, bad, bad, 4]          # rows 1, 3: the scalar alone; rows 2, 4: the scalar and a bad point; rows 0, 5: fine
        got, st = ctx.pedersen_sum_batch(off, b"".join(pts), None, sc.pack(vals, 32), 32, _bl(bls))
        vd = ctx.pedersen_balance_batch(off, b"".join(pts), None, sc.pack(vals, 32), 32, _bl(bls))
        assert st == bytes([sc.OK] + [sc.BAD_SCALAR] * 4 + [sc.OK])
        assert vd == bytes([sc.VERIFICATION_ERROR] + [sc.FORMAT_ERROR] * 4 + [sc.VERIFICATION_ERROR])
        got = _split(got)
        assert got[1:5] == [bytes(32)] * 4
        for r in (0, 5):
            assert got[r] == sc.expect_row(oracle, bases[0], bases[1], pts[off[r]:off[r + 1]], None, vals[r], bls[r])[1]
    got, st = ctx.pedersen_sum_batch([0, 1, 2], b"".join(p[:2]), None, sc.pack([3, 4], 8), 8, _bl([pc.L_ORDER, 1]))
    assert st == bytes([sc.BAD_SCALAR, sc.OK]) and got[:32] == bytes(32)
    assert ctx.get_option("staging_residue") == 0


def test_balance_accepts_sums_of_commitments_and_rejects_one_flipped_bit(contexts, oracle, bases):
    ctx = contexts()
    lengths = [1, 2, 3, 0, 64, 65, 7, 200]
    off, pts, vals, bls = sc.balanced_rows(oracle, bases[0], bases[1], lengths)
    nb, flat = len(lengths), b"".join(pts)
    for vb in (8, 32):
        assert ctx.pedersen_balance_batch(off, flat, None, sc.pack(vals, vb), vb, _bl(bls)) == bytes(nb)
    bad = bytes(sc.VERIFICATION_ERROR if n else sc.BALANCED for n in lengths)
    flipped = list(pts)
    for r, n in enumerate(lengths):
        if n:
            t = off[r] + (5 * r) % n
            flipped[t] = pc.flip_bit(pts[t], (37 * r + 9) % 255)
    assert ctx.pedersen_balance_batch(off, b"".join(flipped), None, sc.pack(vals, 8), 8, _bl(bls)) == bad
    every = bytes([sc.VERIFICATION_ERROR]) * nb
    assert ctx.pedersen_balance_batch(off, flat, None, sc.pack([v ^ (1 << ((11 * r + 3) % 64)) for r, v in enumerate(vals)], 8), 8, _bl(bls)) == every
    bl2 = [b ^ (1 << ((13 * r) % 252)) for r, b in enumerate(bls)]
    bl2 = [f if f < pc.L_ORDER else (b & (b - 1) if b else 1) for f, b in zip(bl2, bls)]
    assert ctx.pedersen_balance_batch(off, flat, None, sc.pack(vals, 8), 8, _bl(bl2)) == every


def test_pinned_on_the_references_golden_commitments(contexts, golden):
    """the vc[j] = j B + r_j B_blinding of the reference's test: their sum opens to (28, sum r_j); vc[7] - vc[3] - vc[4] opens to
    (0, r_7 - r_3 - r_4) and not to value 1"""
    from chacha_rng import golden_blindings
    ctx = contexts()
    vc = _split(golden["vc_bytes"])
    r = [int.from_bytes(b, "little") for b in golden_blindings()]
    L = pc.L_ORDER
    off, pts, sg = [0, 8, 11, 14], vc + [vc[7], vc[3], vc[4]] * 2, bytes(8) + b"\0\1\1" * 2
    vals, bls = [28, 0, 1], [sum(r) % L, (r[7] - r[3] - r[4]) % L, (r[7] - r[3] - r[4]) % L]
    assert ctx.pedersen_balance_batch(off, b"".join(pts), sg, sc.pack(vals, 8), 8, _bl(bls)) == bytes([0, 0, sc.VERIFICATION_ERROR])
    got, st = ctx.pedersen_sum_batch(off[:3], b"".join(pts[:11]), sg[:11])
    com, cst = ctx.pedersen_commit_batch(sc.pack([28, 0], 8), 8, _bl(bls[:2]))
    assert st == cst == bytes(2) and got == com


def _to_dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(torch.device("cuda:0"))


@pytest.mark.parametrize("W,ct", [(None, 0), (7, 1)])
def test_device_pointer_forms_on_a_side_stream_give_the_host_forms_bytes(contexts, batch, W, ct):
    import torch
    ctx = contexts(W, ct)
    (off, pts, vals, bls), _ = batch
    nb, flat, sg = len(off) - 1, b"".join(pts), sc.signs("alternating", off[-1])
    v8, v32, bl = sc.pack(vals, 8), sc.pack(vals, 32), _bl(bls)
    want_plain = ctx.pedersen_sum_batch(off, flat, None)
    want = ctx.pedersen_sum_batch(off, flat, sg, v8, 8, bl)
    want_vd = ctx.pedersen_balance_batch(off, flat, sg, v32, 32, bl)        # (a call with scalars clears the staging on its way out)
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream(device=dev)
    d_pts, d_sg, d_v8, d_v32, d_bl = _to_dev(flat), _to_dev(bytes(3) + bytes(x | 0xfe for x in sg)), _to_dev(v8), _to_dev(v32), _to_dev(bl)
    d_sg = d_sg[3:]                      # the sign bytes at an odd address, every bit but bit 0 set: the _dev forms use bit 0
    full = lambda n: torch.full((n,), 255, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d_o, d_st, d_o2, d_st2, d_vd, d_vd2 = full(32 * nb), full(nb), full(32 * nb), full(nb), full(nb), full(nb)
        ctx.pedersen_sum_batch_dev(off, d_pts.data_ptr(), d_sg.data_ptr(), d_v8.data_ptr(), 8, d_bl.data_ptr(), d_o.data_ptr(), d_st.data_ptr(), side.cuda_stream)
        ctx.pedersen_sum_batch_dev(off, d_pts.data_ptr(), None, None, 8, None, d_o2.data_ptr(), d_st2.data_ptr(), side.cuda_stream)
        ctx.pedersen_balance_batch_dev(off, d_pts.data_ptr(), d_sg.data_ptr(), d_v32.data_ptr(), 32, d_bl.data_ptr(), d_vd.data_ptr(), side.cuda_stream)
        # the first call's sums, one per row, against nothing: row r balances exactly when its sum is the identity
        ctx.pedersen_balance_batch_dev(list(range(nb + 1)), d_o.data_ptr(), None, None, 8, None, d_vd2.data_ptr(), side.cuda_stream)
    side.synchronize()
    assert ctx.get_option("staging_residue") == 0
    host = lambda t: bytes(t.cpu().numpy())
    assert (host(d_o), host(d_st)) == want and (host(d_o2), host(d_st2)) == want_plain and host(d_vd) == want_vd
    assert host(d_vd2) == bytes(0 if e == bytes(32) else 1 for e in _split(want[0]))


def test_commitments_made_on_the_device_feed_the_device_balance_check(contexts):
    """bpgpu_pedersen_commit_batch_dev makes 3 x 70 commitments with device-drawn blindings; bpgpu_pedersen_sum_batch_dev adds them in rows
    of three; the device's own scalar sums open them in bpgpu_pedersen_balance_batch_dev: nothing visits the host but the verdicts"""
    import torch
    ctx = contexts()
    nb = 70
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream(device=dev)
    d_v = torch.arange(1, 3 * nb + 1, dtype=torch.int64, device=dev)
    d_seed = _to_dev(bytes([24]) * 32)
    off = [3 * r for r in range(nb + 1)]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d_c = torch.zeros(32 * 3 * nb, dtype=torch.uint8, device=dev)
        d_bl = torch.zeros(32 * 3 * nb, dtype=torch.uint8, device=dev)
        d_st = torch.full((3 * nb,), 255, dtype=torch.uint8, device=dev)
        ctx.pedersen_commit_batch_dev(3 * nb, d_v.data_ptr(), 8, None, d_seed.data_ptr(), 0, d_c.data_ptr(), d_bl.data_ptr(), d_st.data_ptr(), side.cuda_stream)
        d_vsum = d_v.view(nb, 3).sum(dim=1).contiguous()
        # the rows' sums on the device, then: inputs = the three commitments, output = their sum -> balances against (0, 0), no scalars
        d_sum = torch.zeros(32 * nb, dtype=torch.uint8, device=dev)
        d_sst = torch.full((nb,), 255, dtype=torch.uint8, device=dev)
        ctx.pedersen_sum_batch_dev(off, d_c.data_ptr(), None, None, 8, None, d_sum.data_ptr(), d_sst.data_ptr(), side.cuda_stream)
        d_rows = torch.cat([d_c.view(nb, 96), d_sum.view(nb, 32)], dim=1).contiguous()
        d_sg = torch.tensor([0, 0, 0, 1] * nb, dtype=torch.uint8, device=dev)
        d_vd = torch.full((nb,), 255, dtype=torch.uint8, device=dev)
        ctx.pedersen_balance_batch_dev([4 * r for r in range(nb + 1)], d_rows.data_ptr(), d_sg.data_ptr(), None, 8, None, d_vd.data_ptr(), side.cuda_stream)
        # and with the value on the device: sum - (sum v) B is a commitment to (0, sum r): it does not balance against value 0 without
        # the blinding, which stays a secret of the device buffers here -- the verdict is VerificationError for every row
        d_vd2 = torch.full((nb,), 255, dtype=torch.uint8, device=dev)
        ctx.pedersen_balance_batch_dev(off, d_c.data_ptr(), None, d_vsum.data_ptr(), 8, None, d_vd2.data_ptr(), side.cuda_stream)
    side.synchronize()
    host = lambda t: bytes(t.cpu().numpy())
    assert host(d_st) == bytes(3 * nb) and host(d_sst) == bytes(nb)
    assert host(d_vd) == bytes(nb) and host(d_vd2) == bytes([sc.VERIFICATION_ERROR]) * nb
    # the host agrees: the device-made commitments and blindings open row by row to (sum v, sum r)
    bl = [int.from_bytes(b, "little") for b in _split(host(d_bl))]
    rsum = [sum(bl[3 * r:3 * r + 3]) % pc.L_ORDER for r in range(nb)]
    vsum = [sum(range(3 * r + 1, 3 * r + 4)) for r in range(nb)]
    assert ctx.pedersen_balance_batch(off, host(d_c), None, sc.pack(vsum, 8), 8, _bl(rsum)) == bytes(nb)


def test_a_context_without_generators_serves_the_scalar_free_forms(oracle, bases):
    import bulletproofs_amd as bp
    bare = bp.Context(0)
    lengths = [0, 3, 70, 1]
    off = sc.offsets(lengths)
    pts = sc.points(off[-1], shift=9)
    sg = sc.signs("alternating", off[-1])
    got, st = bare.pedersen_sum_batch(off, b"".join(pts), sg)
    assert st == bytes(4) and _split(got) == sc.expect_rows(oracle, bases[0], bases[1], off, pts, sg)
    assert bare.pedersen_balance_batch([0, 2, 3], b"".join([pts[0], pts[0], pts[1]]), b"\0\1\0") == bytes([0, 1])
    L = bp.lib()
    o4 = (C.c_uint32 * 5)(*off)
    out, stb = C.create_string_buffer(128), C.create_string_buffer(4)
    flat = b"".join(pts)
    assert L.bpgpu_pedersen_sum_batch(bare.h, 4, o4, flat, None, bytes(32), 8, None, out, stb) == NO_GENS
    assert L.bpgpu_pedersen_sum_batch(bare.h, 4, o4, flat, None, None, 8, bytes(128), out, stb) == NO_GENS
    assert L.bpgpu_pedersen_balance_batch(bare.h, 4, o4, flat, None, bytes(32), 8, None, stb) == NO_GENS
    assert L.bpgpu_pedersen_sum_batch_dev(bare.h, 4, o4, 256, None, 256, 8, None, 256, 256, None) == NO_GENS
    assert L.bpgpu_pedersen_balance_batch_dev(bare.h, 4, o4, 256, None, None, 8, 256, 256, None) == NO_GENS
    assert L.bpgpu_pedersen_sum_batch(bare.h, 0, None, None, None, None, 8, None, None, None) == 0
    bare.close()


def test_error_returns(contexts):
    import bulletproofs_amd as bp
    ctx = contexts()
    L = bp.lib()
    nb = 3
    off = (C.c_uint32 * 4)(0, 2, 2, 5)
    pts = b"".join(sc.pool()[:5])
    sg, v8, bl = bytes([0, 1, 0, 0, 1]), sc.pack([1, 2, 3], 8), pc.le32(4) * nb
    out, st = C.create_string_buffer(32 * nb), C.create_string_buffer(nb)

    def S(h=ctx.h, nb_=nb, off_=off, p=pts, s=sg, v=v8, vb=8, b=bl, out_=out, st_=st):
        return L.bpgpu_pedersen_sum_batch(h, nb_, off_, p, s, v, vb, b, out_, st_)

    def B(h=ctx.h, nb_=nb, off_=off, p=pts, s=sg, v=v8, vb=8, b=bl, vd=st):
        return L.bpgpu_pedersen_balance_batch(h, nb_, off_, p, s, v, vb, b, vd)

    assert S() == 0 and st.raw == bytes(nb) and B() == 0
    assert S(nb_=0) == 0 and B(nb_=0) == 0 and S(nb_=0, off_=None, p=None, s=None, v=None, b=None, out_=None, st_=None) == 0
    for vb in (0, 4, 16, 31, 33, 64):
        assert S(vb=vb) == INVALID_ARG and B(vb=vb) == INVALID_ARG
        assert S(vb=vb, v=None) == 0                                               # value_bytes counts only when values are given
    assert b"value_bytes" in (S(vb=7), L.bpgpu_last_error(ctx.h))[1]
    for bad_off in ((1, 2, 2, 5), (0, 2, 1, 5), (0, 3, 2, 5)):
        o = (C.c_uint32 * 4)(*bad_off)
        assert S(off_=o) == INVALID_ARG and B(off_=o) == INVALID_ARG
    assert b"row_offsets" in L.bpgpu_last_error(ctx.h)
    for bad_sg in (bytes([0, 1, 2, 0, 1]), bytes([0, 0, 0, 0, 255])):
        assert S(s=bad_sg) == INVALID_ARG and B(s=bad_sg) == INVALID_ARG
    assert b"sign" in L.bpgpu_last_error(ctx.h)
    for kw in (dict(off_=None), dict(p=None), dict(out_=None), dict(st_=None)):
        assert S(**kw) == INVALID_ARG, kw
    for kw in (dict(off_=None), dict(p=None), dict(vd=None)):
        assert B(**kw) == INVALID_ARG, kw
    assert S(h=None) == INVALID_ARG and B(h=None) == INVALID_ARG
    assert S(s=None) == 0 and S(v=None) == 0 and S(b=None) == 0 and S(v=None, b=None) == 0 and B(v=None, b=None) == 0
    assert S(v=sc.pack([1, 2, 3], 32), vb=32) == 0
    assert ctx.get_option("staging_residue") == 0
    # the device forms check what they can without reading device memory
    D, V = L.bpgpu_pedersen_sum_batch_dev, L.bpgpu_pedersen_balance_batch_dev
    assert D(ctx.h, 0, None, None, None, None, 8, None, None, None, None) == 0 and V(ctx.h, 0, None, None, None, None, 8, None, None, None) == 0
    assert D(ctx.h, nb, off, 256, 257, 256, 7, 256, 256, 256, None) == INVALID_ARG and V(ctx.h, nb, off, 256, 257, 256, 9, 256, 256, None) == INVALID_ARG
    assert D(ctx.h, nb, (C.c_uint32 * 4)(0, 2, 1, 5), 256, None, None, 8, None, 256, 256, None) == INVALID_ARG
    assert D(ctx.h, nb, off, 258, None, None, 8, None, 256, 256, None) == INVALID_ARG          # misaligned points
    assert D(ctx.h, nb, off, 256, None, 258, 8, None, 256, 256, None) == INVALID_ARG           # ... values
    assert D(ctx.h, nb, off, 256, None, None, 8, None, 258, 256, None) == INVALID_ARG          # ... out
    assert D(ctx.h, nb, off, None, None, None, 8, None, 256, 256, None) == INVALID_ARG         # terms without points
    assert D(ctx.h, nb, off, 256, None, None, 8, None, None, 256, None) == INVALID_ARG and D(ctx.h, nb, off, 256, None, None, 8, None, 256, None, None) == INVALID_ARG
    assert V(ctx.h, nb, off, 256, None, None, 8, None, None, None) == INVALID_ARG and V(ctx.h, nb, None, 256, None, None, 8, None, 256, None) == INVALID_ARG
    assert S() == 0


def test_python_api():
    from bulletproofs_amd import BulletproofGens
    from bulletproofs_amd.api import FormatError, VerificationError
    gens = BulletproofGens(8, 1, fixed_window_bits=8)
    rs = [pc.le32(r) for r in pc.blindings()]
    ints = [0, 1, 2**64 - 1, 2**63, 77, 0x8080808080808080, 5, 6]
    coms, _ = gens.commit_batch(ints, rs)
    L = pc.L_ORDER
    rsum = lambda idx: pc.le32(sum(int.from_bytes(rs[i], "little") for i in idx) % L)
    # inputs {4, 6} and {1, 7} against outputs {} and {0}: (77 + 5, r4 + r6), (1 + 6 - 0, r1 + r7 - r0)
    inputs, outputs = [[coms[4], coms[6]], [coms[1], coms[7]], []], [[], [coms[0]], []]
    r1 = pc.le32((int.from_bytes(rs[1], "little") + int.from_bytes(rs[7], "little") - int.from_bytes(rs[0], "little")) % L)
    zero = bytes(32)
    assert gens.verify_balance(inputs, outputs, [82, 7, 0], [rsum([4, 6]), r1, zero]) == [None, None, None]
    assert gens.verify_balance(inputs, outputs, [pc.le32(82), pc.le32(7), zero], [rsum([4, 6]), r1, zero]) == [None, None, None]
    assert gens.verify_balance(inputs, outputs, [82, 8, 0], [rsum([4, 6]), r1, pc.le32(L)]) == [None, VerificationError(), FormatError()]
    assert gens.verify_balance([[coms[3]], [b"\xff" * 32]], [[coms[3]], []]) == [None, VerificationError()]
    sums = gens.sum_commitments(inputs, outputs)
    assert sums == [gens.commit(82, rsum([4, 6])), gens.commit(7, r1), zero]
    assert gens.sum_commitments([[coms[5]], []], None, [3, 9], [rs[2], rs[3]]) == [gens.sum_commitments([[coms[5], gens.commit(3, rs[2])]])[0], gens.commit(9, rs[3])]
    assert gens.sum_commitments([[coms[2], b"\xff" * 32], [coms[2]]]) == [None, coms[2]]
    assert gens.sum_commitments([]) == [] and gens.verify_balance([], []) == []
    with pytest.raises(ValueError):
        gens.sum_commitments([[coms[1]]], None, [5], [pc.le32(L)])
    with pytest.raises(ValueError):
        gens.sum_commitments([[coms[1]]], None, [2**64])
    with pytest.raises(ValueError):
        gens.sum_commitments([[coms[1]]], [[], []])
    with pytest.raises(ValueError):
        gens.verify_balance([[coms[1][:31]]], [[]])
    with pytest.raises(TypeError):
        gens.verify_balance([[coms[1]], []], [[], []], [1, pc.le32(2)])
    gens.ctx.close()


def test_cpp_mirror_has_the_two_calls(tmp_path):
    """include/bulletproofs.hpp: BulletproofGens::sum_commitments / verify_balance"""
    exe, csrc = str(tmp_path / "pedersen_sum_test"), os.path.join(ROOT, "bulletproofs_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "pedersen_sum_test.cpp"),
                           "-L", csrc, "-lbpgpu", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout
