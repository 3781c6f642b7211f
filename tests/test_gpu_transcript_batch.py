"""Batches of Merlin transcripts built and bound on the GPU (bpgpu_transcript_batch / _dev, bulletproofs_amd.TranscriptBatch).
CONTRACT (include/bpgpu.h): for every row, the output state and every challenge are byte for byte what the three host helpers
(bpgpu_transcript_new / _append_message / _challenge_bytes) produce when applied to that row's start state op by op.  The states made
on the device go into the `_ts_dev` entry points with no further step."""
import ctypes as C
import hashlib

import pytest

import rlc_ts_cases as cases

pytestmark = pytest.mark.gpu

TS = 208
INVALID_ARG = -1
L_ORDER = 2**252 + 27742317777372353535851937790883648493
NBATCHES = [1, 63, 64, 65, 257]


@pytest.fixture(scope="module")
def bare():
    """a context that never loads generators"""
    import bulletproofs_amd as bp
    c = bp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx8():
    import bulletproofs_amd as bp
    c = bp.Context(0)
    c.gens_create(8, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gens8(oracle):
    return oracle.Gens(8, 1)


def _msg(tag, n):
    return hashlib.shake_256(b"tsb-%d" % tag).digest(n)


_positions = {}


def _at(pos):
    """a bound state standing at STROBE position pos, found by search over the length of a session id (host helpers)"""
    from bulletproofs_amd import _lib
    if not _positions:
        for length in range(400):
            st = _lib.transcript_append_message(_lib.transcript_new(b"payment-protocol v3"), b"session", _msg(length, length))
            _positions.setdefault(st[200], st)
        assert sorted(_positions) == list(range(166))
    return _positions[pos]


def _host_loop(starts, script):
    """the reference: the three host helpers, row by row, op by op -> (states, [per challenge op: per row])"""
    from bulletproofs_amd import _lib
    states, outs = [], [[] for s in script if s[0].startswith("challenge")]
    for r, st in enumerate(starts):
        k = 0
        for step in script:
            if step[0] == "append":
                st = _lib.transcript_append_message(st, step[1], step[2] if isinstance(step[2], bytes) else step[2][r])
            elif step[0] == "append_u64":
                st = _lib.transcript_append_message(st, step[1], (step[2] if isinstance(step[2], int) else step[2][r]).to_bytes(8, "little"))
            elif step[0] == "challenge":
                st, o = _lib.transcript_challenge_bytes(st, step[1], step[2])
                outs[k].append(o)
                k += 1
            else:
                st, o = _lib.transcript_challenge_bytes(st, step[1], 64)
                outs[k].append((int.from_bytes(o, "little") % L_ORDER).to_bytes(32, "little"))
                k += 1
        states.append(st)
    return states, outs


def _to_dev(b):
    import torch
    return torch.frombuffer(bytearray(b) + bytearray(8), dtype=torch.uint8).to("cuda:0")[:len(b)]


def _dev_ops(script, nb):
    """the script with its rows in device memory -> (raw ops for Context.transcript_batch_dev, tensors to keep, [(out tensor, n)])"""
    import torch
    from bulletproofs_amd import _lib
    raw, keep, outs = [], [], []
    for step in script:
        kind, label = step[0], step[1]
        if kind == "append" and isinstance(step[2], bytes):
            t = _to_dev(step[2])
            raw.append((_lib.TS_APPEND, label, t.data_ptr(), 0, len(step[2]), None))
            keep.append(t)
        elif kind == "append":
            ln = max(len(m) for m in step[2])
            t = _to_dev(b"".join(m + bytes(ln - len(m)) for m in step[2]))
            lens = torch.tensor([len(m) for m in step[2]], dtype=torch.int32, device="cuda:0")
            ragged = any(len(m) != ln for m in step[2])
            raw.append((_lib.TS_APPEND, label, t.data_ptr(), ln, ln, lens.data_ptr() if ragged else None))
            keep += [t, lens]
        elif kind == "append_u64":
            xs = [step[2]] if isinstance(step[2], int) else step[2]
            t = torch.tensor([x - (1 << 64) if x >> 63 else x for x in xs], dtype=torch.int64, device="cuda:0")
            raw.append((_lib.TS_APPEND_U64, label, t.data_ptr(), 0 if isinstance(step[2], int) else 8, 8, None))
            keep.append(t)
        else:
            n = step[2] if kind == "challenge" else 32
            t = torch.full((n * nb + 1,), 0x5a, dtype=torch.uint8, device="cuda:0")      # one guard byte behind the last row
            raw.append((_lib.TS_CHALLENGE if kind == "challenge" else _lib.TS_CHALLENGE_SCALAR, label, t.data_ptr(), max(n, 1), n, None))
            outs.append((t, n))
    return raw, keep, outs


def _dev_form(ctx, starts, script, label=None, shared=False):
    import torch
    nb = len(starts)
    side = torch.cuda.Stream(device="cuda:0")
    raw, keep, outs = _dev_ops(script, nb)
    d_in = None if label is not None else _to_dev(starts[0] if shared else b"".join(starts))
    d_out = torch.full((TS * nb + 1,), 0x5a, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.transcript_batch_dev(nb, raw, d_out.data_ptr(), label=label, d_states_in=None if d_in is None else d_in.data_ptr(),
                             stride_in=0 if (shared or label is not None) else TS, stream=side.cuda_stream)
    side.synchronize()
    got = bytes(d_out.cpu().numpy())
    assert got[TS * nb:] == b"\x5a"
    res = []
    for t, n in outs:
        b = bytes(t.cpu().numpy())
        assert b[n * nb:] == b"\x5a"
        res.append([b[n * r:n * r + n] for r in range(nb)])
    return [got[TS * r:TS * r + TS] for r in range(nb)], res


def _host_form(ctx, starts, script, label=None, shared=False):
    nb = len(starts)
    st, outs = ctx.transcript_batch(nb, script, label=label, states=None if label is not None else (starts[0] if shared else b"".join(starts)))
    return [st[TS * r:TS * r + TS] for r in range(nb)], outs


def _parity(ctx, starts, script, **kw):
    want = _host_loop(starts, script)
    assert _host_form(ctx, starts, script, **kw) == want
    assert _dev_form(ctx, starts, script, **kw) == want


def _rich_script(nb):
    return [("append", b"context", [_msg(r, (37 * r) % 90) for r in range(nb)]), ("append", b"shared", _msg(9, 40)),
            ("append_u64", b"n", [(r * 0x9e3779b97f4a7c15) % 2**64 for r in range(nb)]), ("challenge", b"binding", 16), ("challenge_scalar", b"x"),
            ("append", _msg(1, 165), [_msg(r, 3) for r in range(nb)]), ("append_u64", b"m", 2**63 + 5), ("challenge", _msg(2, 167), 167),
            ("append", b"", b""), ("challenge", b"nothing", 0)]


@pytest.mark.parametrize("nb", NBATCHES)
def test_host_and_device_forms_equal_the_loop_of_host_helpers(bare, nb):
    """rows at positions 7 r mod 166 (every position of the rate at 257 rows), ragged and shared appends, u64s, challenges of 0, 16 and
    167 bytes, a scalar, labels of 0, 165 and 167 bytes; then the README binding from Transcript::new and from one shared state"""
    from bulletproofs_amd import _lib
    _parity(bare, [_at((7 * r) % 166) for r in range(nb)], _rich_script(nb))
    sessions = [("append", b"session", [_msg(r, 32) for r in range(nb)])]
    fresh = _lib.transcript_new(b"payment-protocol v3")
    _parity(bare, [fresh] * nb, sessions, label=b"payment-protocol v3")
    _parity(bare, [_at(150)] * nb, sessions + [("challenge", b"c", 32)], shared=True)
    _host_form(bare, [_at(150)] * nb, sessions, shared=True)
    assert bare.get_option("staging_residue") == 0          # the host form's staging is cleared on its way out


def test_one_row_of_a_wavefront_wraps_the_rate_inside_an_append(bare):
    starts = [_at(10)] * 64
    starts[17] = _at(150)
    script = [("append", b"V", [_msg(r, 32) for r in range(64)])]
    ends = [st[200] for st in _host_loop(starts, script)[0]]
    assert ends[17] < 150 and all(e > 10 for r, e in enumerate(ends) if r != 17)      # row 17 alone went round the rate
    _parity(bare, starts, script)


def test_a_wavefront_whose_rows_start_at_64_different_positions(bare):
    starts = [_at((5 * r) % 166) for r in range(64)]
    assert len({s[200] for s in starts}) == 64
    _parity(bare, starts, [("append", b"blob", [_msg(r, 400) for r in range(64)]), ("challenge", b"c", 200), ("challenge_scalar", b"s")])


def test_lens_make_rows_wrap_zero_one_and_two_times_in_one_op(bare):
    lens = [(10, 200, 400, 0)[r % 4] for r in range(64)]
    _parity(bare, [_at(20)] * 64, [("append", b"ragged", [_msg(r, n) for r, n in enumerate(lens)]), ("challenge", b"c", 8)])
    # message lengths around the rate and a long one, as lens of one op, from a position where the framing bytes straddle the rate
    lens = [0, 1000, 1, 3, 4, 5, 163, 164, 165, 166, 167, 168, 331, 332, 333, 1000, 0]
    _parity(bare, [_at(165)] * len(lens), [("append", b"m", [_msg(r, n) for r, n in enumerate(lens)])])


def test_rows_take_per_row_prefixes_of_one_shared_message(bare):
    """BPGPU_TS_APPEND with stride 0 AND lens, both forms: row 0 takes nothing of the one message, later rows more, some all of it"""
    import torch
    from bulletproofs_amd import _lib
    nb, msg = 66, _msg(77, 300)
    starts = [_at((23 * r) % 166) for r in range(nb)]
    lens = [0, 300, 1, 166] + [(37 * r) % 301 for r in range(4, nb)]
    want = b"".join(_host_loop(starts, [("append", b"shared", [msg[:n] for n in lens])])[0])
    bare.transcript_batch(nb, [("append", b"earlier", [_msg(r, 300) for r in range(nb)])], states=b"".join(starts))     # what a stale staging block would hold
    h_msg, h_lens = C.create_string_buffer(msg, len(msg)), (C.c_uint32 * nb)(*lens)
    arr, keep = bare._ts_ops([(_lib.TS_APPEND, b"shared", C.addressof(h_msg), 0, len(msg), C.addressof(h_lens))])
    out = C.create_string_buffer(TS * nb)
    assert bare._L.bpgpu_transcript_batch(bare.h, nb, None, 0, b"".join(starts), TS, arr, 1, out) == 0
    assert out.raw == want
    d_msg, d_lens, d_st = _to_dev(msg), torch.tensor(lens, dtype=torch.int32, device="cuda:0"), _to_dev(b"".join(starts))
    d_out = torch.zeros(TS * nb, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    bare.transcript_batch_dev(nb, [(_lib.TS_APPEND, b"shared", d_msg.data_ptr(), 0, len(msg), d_lens.data_ptr())], d_out.data_ptr(), d_states_in=d_st.data_ptr(),
                              stride_in=TS)
    bare.synchronize()
    assert bytes(d_out.cpu().numpy()) == want


def test_a_call_that_fails_after_staging_clears_the_staging(bare):
    """the host form meets a lens[r] > len in its SECOND op, when the first op's rows are staged already: INVALID_ARG, outputs untouched,
    nothing left in the staging buffers"""
    from bulletproofs_amd import _lib
    nb = 5
    starts = b"".join(_at(p) for p in range(nb))
    secret = C.create_string_buffer(b"\xa5" * (64 * nb), 64 * nb)
    small, lens_bad = C.create_string_buffer(b"\x5a" * (8 * nb), 8 * nb), (C.c_uint32 * nb)(1, 2, 9, 0, 8)
    arr, keep = bare._ts_ops([(_lib.TS_APPEND, b"secret", C.addressof(secret), 64, 64, None), (_lib.TS_APPEND, b"m", C.addressof(small), 8, 8, C.addressof(lens_bad))])
    out = C.create_string_buffer(b"\x77" * (TS * nb), TS * nb)
    assert bare._L.bpgpu_transcript_batch(bare.h, nb, None, 0, starts, TS, arr, 2, out) == INVALID_ARG
    assert out.raw == b"\x77" * (TS * nb)
    assert bare.get_option("staging_residue") == 0


def test_states_out_may_be_states_in_and_scripts_chain_on_one_stream(bare):
    import torch
    nb = 130
    starts = [_at((11 * r) % 166) for r in range(nb)]
    s1 = [("append", b"session", [_msg(r, 40 + r % 7) for r in range(nb)]), ("challenge", b"binding", 16)]
    s2 = [("append", b"context", [_msg(1000 + r, (13 * r + 5) % 166) for r in range(nb)]), ("challenge_scalar", b"x")]
    want_mid, want_o1 = _host_loop(starts, s1)
    want, want_o2 = _host_loop(want_mid, s2)
    side = torch.cuda.Stream(device="cuda:0")
    d_st = _to_dev(b"".join(starts))
    d_end = torch.full((TS * nb,), 0x5a, dtype=torch.uint8, device="cuda:0")
    raw1, keep1, outs1 = _dev_ops(s1, nb)
    raw2, keep2, outs2 = _dev_ops(s2, nb)
    torch.cuda.synchronize()
    bare.transcript_batch_dev(nb, raw1, d_st.data_ptr(), d_states_in=d_st.data_ptr(), stride_in=TS, stream=side.cuda_stream)      # in place
    bare.transcript_batch_dev(nb, raw2, d_end.data_ptr(), d_states_in=d_st.data_ptr(), stride_in=TS, stream=side.cuda_stream)    # no synchronisation between
    side.synchronize()
    assert bytes(d_st.cpu().numpy()) == b"".join(want_mid) and bytes(d_end.cpu().numpy()) == b"".join(want)
    assert bytes(outs1[0][0].cpu().numpy())[:16 * nb] == b"".join(want_o1[0]) and bytes(outs2[0][0].cpu().numpy())[:32 * nb] == b"".join(want_o2[0])
    # the host form in place of its own input
    from bulletproofs_amd import _lib
    buf, abc = C.create_string_buffer(b"".join(starts), TS * nb), C.create_string_buffer(b"abc", 3)
    arr, keep = bare._ts_ops([(_lib.TS_APPEND, b"shared", C.addressof(abc), 0, 3, None)])
    assert bare._L.bpgpu_transcript_batch(bare.h, nb, None, 0, buf, TS, arr, 1, buf) == 0
    assert buf.raw == b"".join(_host_loop(starts, [("append", b"shared", b"abc")])[0])


def _bind_script(nb, tag):
    """rlc_ts_cases.bound_state's history behind Transcript::new: session id, an earlier challenge, a context whose length moves the position"""
    js = [i + 1000 * len(tag) for i in range(nb)]
    return [("append", b"session", [hashlib.shake_256(b"sess%d" % j).digest(40 + j % 7) for j in js]), ("challenge", b"binding", 16),
            ("append", b"amount-commitment-context", [hashlib.shake_256(b"ctx%d" % j).digest((13 * j + 5) % 166) for j in js])]


def test_states_bound_on_the_device_verify_range_proofs_in_the_same_stream(ctx8, oracle, gens8):
    """new + append session + challenge binding + append context on the device, then bpgpu_rangeproof_verify_batch_ts_dev on those states, all
    in one stream: verdicts and transcripts_out equal the run on host-made states and oracle.verify_ts"""
    import torch
    n, m, nb, tag = 8, 1, 7, b"tsb"
    g = cases.proofs_on_states(oracle, gens8, n, m, nb, "differing", tag)
    proofs = bytearray(b"".join(g["proofs"]))
    proofs[2 * g["pl"] + 130] ^= 1                              # one wrong t_x
    proofs, coms, rng = bytes(proofs), b"".join(g["coms"]), cases.rand64(b"tsb-rng", nb)
    want_v, want_ts = ctx8.rangeproof_verify_batch_ts(n, m, proofs, g["pl"], coms, b"".join(g["states"]), rng, want_transcripts=True)
    side = torch.cuda.Stream(device="cuda:0")
    raw, keep, outs = _dev_ops(_bind_script(nb, tag), nb)
    d_st = torch.full((TS * nb,), 0x5a, dtype=torch.uint8, device="cuda:0")
    d_p, d_c, d_r = _to_dev(proofs), _to_dev(coms), _to_dev(rng)
    d_v = torch.full((nb,), 0x5a, dtype=torch.uint8, device="cuda:0")
    d_o = torch.full((TS * nb,), 0x5a, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx8.transcript_batch_dev(nb, raw, d_st.data_ptr(), label=b"payment-protocol v3", stream=side.cuda_stream)
    ctx8._chk(ctx8._L.bpgpu_rangeproof_verify_batch_ts_dev(ctx8.h, n, m, nb, d_p.data_ptr(), g["pl"], d_c.data_ptr(), None, d_st.data_ptr(), d_r.data_ptr(),
                                                          d_v.data_ptr(), None, d_o.data_ptr(), side.cuda_stream))
    side.synchronize()
    assert bytes(d_st.cpu().numpy()) == b"".join(g["states"])
    got_v, got_ts = bytes(d_v.cpu().numpy()), bytes(d_o.cpu().numpy())
    assert got_v == bytes(want_v) and got_ts == want_ts
    for i in range(nb):
        rc, _, est = oracle.verify_ts(gens8, proofs[g["pl"] * i:g["pl"] * (i + 1)], coms[32 * i:32 * i + 32], n, g["states"][i], rng[64 * i:64 * i + 64])
        assert got_v[i] == rc == (1 if i == 2 else 0) and got_ts[TS * i:TS * i + TS] == est, i


def test_states_bound_on_the_device_prove_range_proofs_in_the_same_stream(ctx8, oracle, gens8):
    import torch
    n, m, nb, tag = 8, 1, 5, b"tsbp"
    states = [cases.bound_state(oracle, i + 1000 * len(tag)) for i in range(nb)]
    vals = [(37 * i + 3) % 256 for i in range(nb)]
    bl = b"".join(hashlib.shake_256(b"tsbp-b%d" % i).digest(31) + b"\x00" for i in range(nb))
    seeds = hashlib.shake_256(b"tsbp-seeds").digest(32 * nb)
    want = ctx8.rangeproof_prove_batch_ts(n, m, vals, bl, b"".join(states), seeds, want_transcripts=True)
    pl = len(want[0]) // nb
    side = torch.cuda.Stream(device="cuda:0")
    raw, keep, outs = _dev_ops(_bind_script(nb, tag), nb)
    d_st = torch.full((TS * nb,), 0x5a, dtype=torch.uint8, device="cuda:0")
    d_vals = torch.tensor(vals, dtype=torch.int64, device="cuda:0")
    d_b, d_s = _to_dev(bl), _to_dev(seeds)
    d_p = torch.full((pl * nb,), 0x5a, dtype=torch.uint8, device="cuda:0")
    d_c = torch.full((32 * nb,), 0x5a, dtype=torch.uint8, device="cuda:0")
    d_o = torch.full((TS * nb,), 0x5a, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx8.transcript_batch_dev(nb, raw, d_st.data_ptr(), label=b"payment-protocol v3", stream=side.cuda_stream)
    ctx8.rangeproof_prove_batch_ts_dev(n, m, nb, d_vals.data_ptr(), d_b.data_ptr(), d_st.data_ptr(), TS, d_s.data_ptr(), d_p.data_ptr(), d_c.data_ptr(),
                                       d_o.data_ptr(), side.cuda_stream)
    side.synchronize()
    assert bytes(d_st.cpu().numpy()) == b"".join(states)
    got = (bytes(d_p.cpu().numpy()), bytes(d_c.cpu().numpy()), bytes(d_o.cpu().numpy()))
    assert got == want
    for i in range(nb):
        rc, _, est = oracle.verify_ts(gens8, got[0][pl * i:pl * (i + 1)], got[1][32 * i:32 * i + 32], n, states[i], bytes(64))
        assert rc == 0 and est == got[2][TS * i:TS * i + TS], i


def test_transcript_batch_in_the_python_api(oracle, gens8):
    """TranscriptBatch in place of the equivalent list of Transcript: RangeProof.verify_batch / verify_batch_combined / prove_batch and
    LinearProof.create_batch / verify_batch / verify_batch_combined give the list's results and leave the batch at the list's states"""
    import bulletproofs_amd as bp
    from bulletproofs_amd import api
    n, m, nb = 8, 1, 6
    gens = api.BulletproofGens(8, 1)
    ctx8 = gens.ctx
    g = cases.proofs_on_states(oracle, gens8, n, m, nb, "differing", b"tsba")
    script = _bind_script(nb, b"tsba")

    def batch():
        b = bp.TranscriptBatch(ctx8, b"payment-protocol v3", nb)
        b.append_message(b"session", script[0][2])
        assert b.challenge_bytes(b"binding", 16) == _host_loop([bp._lib.transcript_new(b"payment-protocol v3")] * nb, script[:2])[1][0]
        b.append_message(b"amount-commitment-context", script[2][2])
        return b

    def lst():
        out = []
        for st in g["states"]:
            t = api.Transcript(b"unused")
            t.state, t.fresh_label = st, None
            out.append(t)
        return out
    b = batch()
    assert len(b) == nb and b.states() == b"".join(g["states"]) and b[3].state == g["states"][3] and b[-1].state == g["states"][-1]
    proofs = [bytearray(p) for p in g["proofs"]]
    proofs[4][130] ^= 1
    proofs = [bytes(p) for p in proofs]
    coms = [[c] for c in g["coms"]]
    kinds = lambda res: [type(x) for x in res]
    want = [type(None)] * nb
    want[4] = api.VerificationError
    for fn in (api.RangeProof.verify_batch, api.RangeProof.verify_batch_combined):
        b, l = batch(), lst()
        assert kinds(fn(gens, None, b, proofs, coms, n)) == kinds(fn(gens, None, l, proofs, coms, n)) == want
        assert b.states() == b"".join(t.state for t in l) == b"".join(g["states"])                    # neither is advanced
    items = lambda ts: [(ts[i], proofs[i], coms[i], n) for i in range(nb)]
    assert kinds(api.RangeProof.verify_mixed_combined(gens, None, items(batch()), bound_transcripts=True)) == want
    vals, bl, seeds = [[i + 1] for i in range(nb)], [[bytes([i + 1]) + bytes(31)] for i in range(nb)], hashlib.shake_256(b"api-seeds").digest(32 * nb)
    b, l = batch(), lst()
    made_b, made_l = api.RangeProof.prove_batch(gens, None, b, vals, bl, n, seeds), api.RangeProof.prove_batch(gens, None, l, vals, bl, n, seeds)
    assert [(p.to_bytes(), c) for p, c in made_b] == [(p.to_bytes(), c) for p, c in made_l]
    assert b.states() == b"".join(t.state for t in l) != b"".join(g["states"])                         # both advanced, alike
    # a flush that the library refuses keeps the recorded appends
    c3 = b.clone()
    c3.append_message(b"too long", bytes(bp._lib.TS_MAX_LEN + 1))
    with pytest.raises(bp.BpgpuError):
        c3.states()
    assert len(c3._pending) == 1 and c3._states == b._states
    with pytest.raises(AssertionError):
        ctx8.transcript_batch(nb, [("append_u64", b"n", [7])], states=b.states())          # a list holds one value per row
    c2 = b.clone()
    c2.append_u64(b"more", 7)
    assert c2.states() != b.states() and len(c2.states()) == TS * nb
    # LinearProof: n = 4 statements on the same sessions
    ln = 4
    Gall, _, Bp, Bb = ctx8.gens_export()
    G, F, B = [Gall[32 * i:32 * i + 32] for i in range(ln)], Bp, Bb
    le = lambda x: x.to_bytes(32, "little")
    Cs, rs, avs, bvs = [], [], [], []
    for i in range(nb):
        a = [int.from_bytes(_msg(5000 + 10 * i + j, 31), "little") for j in range(ln)]
        bv = [int.from_bytes(_msg(6000 + 10 * i + j, 31), "little") for j in range(ln)]
        r = int.from_bytes(_msg(7000 + i, 31), "little")
        c = sum(x * y for x, y in zip(a, bv)) % L_ORDER
        rc, Cc = oracle.msm(b"".join(le(x) for x in a) + le(r) + le(c), b"".join(G) + B + F)
        assert rc == 0
        Cs.append(Cc), rs.append(le(r)), avs.append([le(x) for x in a]), bvs.append([le(x) for x in bv])
    b, l = batch(), lst()
    lp_b = api.LinearProof.create_batch(ctx8, b, Cs, rs, avs, bvs, G, F, B, rng_seed32=seeds)
    lp_l = api.LinearProof.create_batch(ctx8, l, Cs, rs, avs, bvs, G, F, B, rng_seed32=seeds)
    assert [p.to_bytes() for p in lp_b] == [p.to_bytes() for p in lp_l] and b.states() == b"".join(t.state for t in l)
    bad = list(lp_l)
    bad[1] = lp_l[2]
    for fn in (api.LinearProof.verify_batch, api.LinearProof.verify_batch_combined):
        b, l = batch(), lst()
        rb, rl = fn(ctx8, b, bad, Cs, G, F, B, bvs), fn(ctx8, l, bad, Cs, G, F, B, bvs)
        assert kinds(rb) == kinds(rl) and kinds(rl)[1] is api.VerificationError and kinds(rl).count(type(None)) == nb - 1
        assert b.states() == b"".join(t.state for t in l) != b"".join(g["states"])                     # left advanced to the same states
    # from_transcript / from_states
    t = lst()[2]
    ft = bp.TranscriptBatch.from_transcript(ctx8, t, 3)
    ft.append_message(b"k", [b"a", b"bb", b""])
    assert ft.states() == b"".join(_host_loop([t.state] * 3, [("append", b"k", [b"a", b"bb", b""])])[0]) and t.state == g["states"][2]
    fs = bp.TranscriptBatch.from_states(ctx8, lst())
    assert fs.challenge_scalars(b"x") == _host_loop(list(g["states"]), [("challenge_scalar", b"x")])[1][0]
    ctx8.close()


def test_invalid_arguments_caps_and_the_empty_batch(bare):
    import torch
    from bulletproofs_amd import _lib
    L = bare._L
    nb = 3
    st = C.create_string_buffer(b"".join(_at(p) for p in (0, 1, 2)), TS * nb)
    out = C.create_string_buffer(TS * nb)
    big = C.create_string_buffer(max(_lib.TS_MAX_LEN + 1, nb * (_lib.TS_MAX_CHALLENGE + 1)))
    lens_ok = (C.c_uint32 * nb)(0, 5, 2)
    lens_bad = (C.c_uint32 * nb)(0, 6, 2)
    d_st = _to_dev(st.raw)
    d_out = torch.zeros(TS * nb, dtype=torch.uint8, device="cuda:0")
    d_big = torch.zeros(len(big), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()

    def host(ops, nbatch=nb, label=None, states=st, stride=TS, states_out=out):
        arr, keep = bare._ts_ops(ops)
        return L.bpgpu_transcript_batch(bare.h, nbatch, label, len(label) if label is not None else 0, states, stride, arr, len(ops), states_out)

    def dev(ops, nbatch=nb, label=None, states=d_st.data_ptr(), stride=TS, states_out=d_out.data_ptr()):
        arr, keep = bare._ts_ops([(k, lb, None if d is None else d_big.data_ptr(), s, n, ls) for k, lb, d, s, n, ls in ops])
        rc = L.bpgpu_transcript_batch_dev(bare.h, nbatch, label, len(label) if label is not None else 0, states, stride, arr, len(ops), states_out, None)
        bare.synchronize()
        return rc
    p = C.addressof(big)
    A, U, Ch, Sc = _lib.TS_APPEND, _lib.TS_APPEND_U64, _lib.TS_CHALLENGE, _lib.TS_CHALLENGE_SCALAR
    for call in (host, dev):
        # the caps: at the cap, and one above
        assert call([(A, b"l", p, 0, 1, None)] * _lib.TS_MAX_OPS) == 0
        assert call([(A, b"l", p, 0, 1, None)] * (_lib.TS_MAX_OPS + 1)) == INVALID_ARG
        assert call([(A, b"x" * _lib.TS_MAX_LABEL, p, 0, 1, None)]) == 0
        assert call([(A, b"x" * (_lib.TS_MAX_LABEL + 1), p, 0, 1, None)]) == INVALID_ARG
        assert call([(A, b"l", p, 0, _lib.TS_MAX_LEN, None)]) == 0
        assert call([(A, b"l", p, 0, _lib.TS_MAX_LEN + 1, None)]) == INVALID_ARG
        assert call([(Ch, b"l", p, _lib.TS_MAX_CHALLENGE, _lib.TS_MAX_CHALLENGE, None)]) == 0
        assert call([(Ch, b"l", p, _lib.TS_MAX_CHALLENGE + 1, _lib.TS_MAX_CHALLENGE + 1, None)]) == INVALID_ARG
        assert call([], label=b"x" * _lib.TS_MAX_LABEL, states=None, stride=0) == 0
        assert call([], label=b"x" * (_lib.TS_MAX_LABEL + 1), states=None, stride=0) == INVALID_ARG
        # both or neither of new_label and states_in; a stride other than 0 or 208
        assert call([], label=b"both") == INVALID_ARG
        assert call([], states=None) == INVALID_ARG
        assert call([], stride=104) == INVALID_ARG and call([], stride=416) == INVALID_ARG
        # outputs need a stride; kinds; lens goes with appends only; missing data / states_out
        assert call([(Ch, b"l", p, 0, 8, None)]) == INVALID_ARG and call([(Sc, b"l", p, 0, 0, None)]) == INVALID_ARG
        assert call([(Ch, b"l", p, 7, 8, None)]) == INVALID_ARG and call([(Sc, b"l", p, 31, 0, None)]) == INVALID_ARG
        assert call([(0, b"l", p, 0, 1, None)]) == INVALID_ARG and call([(5, b"l", p, 0, 1, None)]) == INVALID_ARG
        assert call([(U, b"l", p, 4, 8, None)]) == INVALID_ARG
        assert call([(A, b"l", None, 0, 1, None)]) == INVALID_ARG
        assert call([], states_out=None) == INVALID_ARG
        # the empty batch
        assert call([(A, b"l", p, 0, 1, None)], nbatch=0) == 0 and call([], nbatch=0, states_out=None) == 0
    assert L.bpgpu_transcript_batch(None, nb, None, 0, st, TS, None, 0, out) == INVALID_ARG
    assert L.bpgpu_transcript_batch_dev(None, nb, None, 0, d_st.data_ptr(), TS, None, 0, d_out.data_ptr(), None) == INVALID_ARG
    # the host form reads lens and the states
    assert host([(A, b"l", p, 8, 5, C.addressof(lens_ok))]) == 0
    assert host([(A, b"l", p, 8, 5, C.addressof(lens_bad))]) == INVALID_ARG
    assert host([(Ch, b"l", p, 8, 8, C.addressof(lens_ok))]) == INVALID_ARG
    for off, val in ((200, 166), (201, 167)):
        bad = bytearray(st.raw)
        bad[TS * 2 + off] = val
        assert host([], states=C.create_string_buffer(bytes(bad), TS * nb)) == INVALID_ARG
        assert host([], states=C.create_string_buffer(bytes(bad[2 * TS:]), TS), stride=0) == INVALID_ARG
        # the device form starts such a row at position 0
        d_bad = _to_dev(bytes(bad))
        torch.cuda.synchronize()
        assert dev([(A, b"l", p, 0, 4, None)], states=d_bad.data_ptr()) == 0
        reset = bytearray(bad[2 * TS:3 * TS])
        reset[200] = reset[201] = 0
        assert bytes(d_out.cpu().numpy())[2 * TS:] == _host_loop([bytes(reset)], [("append", b"l", bytes(d_big[:4].cpu().numpy()))])[0][0]
    # the device form: misaligned states, one shared state overwritten by its own rows
    assert dev([], states=d_st.data_ptr() + 2) == INVALID_ARG and dev([], states_out=d_out.data_ptr() + 1) == INVALID_ARG
    assert dev([], stride=0, states_out=d_st.data_ptr()) == INVALID_ARG
    assert b"stride" in L.bpgpu_last_error(bare.h) or b"states_out" in L.bpgpu_last_error(bare.h)


def test_cpp_mirror_has_a_transcript_batch(tmp_path):
    """include/bulletproofs.hpp: TranscriptBatch and the TranscriptBatch& twins of LinearProof's std::vector<Transcript>& overloads"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, csrc = str(tmp_path / "transcript_batch_test"), os.path.join(root, "bulletproofs_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "transcript_batch_test.cpp"),
                           "-L", csrc, "-lbpgpu", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout
