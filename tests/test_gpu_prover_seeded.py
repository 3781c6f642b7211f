"""bpgpu_rangeproof_prove_batch_ts: range proofs on the callers' own transcripts, every random scalar drawn on the device from one
32-byte seed per proof.  The contract is byte identity with the existing entry point: for every proof the outputs equal
bpgpu_rangeproof_prove_batch(nbatch = 1, shared_transcript = its state, rng = the seed's ChaCha20 keystream), and what the prover
leaves in a transcript is what bpgpu_rangeproof_verify_batch_ts leaves there."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS = 208
INVALID_ARG, NO_GENS = -1, -3


def _block_sizes():
    src = open(os.path.join(ROOT, "bulletproofs_amd", "csrc", "kernels.h")).read()
    return [int(re.search(r"#define %s (\d+)" % name, src).group(1)) for name in ("BP_BLOCK", "RP_BLOCK")]


def _keystream(seed, nblocks):
    """blocks 0..nblocks-1 of ChaCha20 under `seed` (block counter = index, stream id 0), all counters at once; the first block is checked
    against the oracle's restatement of rand_chacha (oracle/py/chacha_rng.py, pinned by the reference's golden blindings)"""
    from chacha_rng import chacha20_block
    st = np.zeros((16, nblocks), dtype=np.uint32)
    st[0:4] = np.frombuffer(b"expand 32-byte k", dtype="<u4")[:, None]
    st[4:12] = np.frombuffer(seed, dtype="<u4")[:, None]
    st[12] = np.arange(nblocks, dtype=np.uint32)
    x = st.copy()
    rot = lambda v, r: (v << np.uint32(r)) | (v >> np.uint32(32 - r))

    def qr(a, b, c, d):
        x[a] += x[b]; x[d] = rot(x[d] ^ x[a], 16)
        x[c] += x[d]; x[b] = rot(x[b] ^ x[c], 12)
        x[a] += x[b]; x[d] = rot(x[d] ^ x[a], 8)
        x[c] += x[d]; x[b] = rot(x[b] ^ x[c], 7)
    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    out = (x + st).T.astype("<u4").tobytes()
    assert out[:64] == chacha20_block(seed, 0)
    return out


def _ndraws(n, m):
    return m * (2 * n + 2) + 2 * m


def _inputs(n, m, nb, tag):
    vals = [int.from_bytes(hashlib.shake_256(b"%s-v%d" % (tag, i)).digest(8), "little") % (1 << n) for i in range(nb * m)]
    bl = b"".join(hashlib.shake_256(b"%s-b%d" % (tag, i)).digest(31) + b"\x00" for i in range(nb * m))
    seeds = [hashlib.shake_256(b"%s-s%d" % (tag, i)).digest(32) for i in range(nb)]
    return vals, bl, seeds


@pytest.fixture(scope="module")
def contexts():
    """one context per generator shape, shared by the tests of this module (fixed_window_bits = 12: small tables)"""
    import bulletproofs_amd as bp
    made = {}

    def get(n, m):
        if (n, m) not in made:
            ctx = bp.Context(0, fixed_window_bits=12)
            ctx.gens_create(n, m)
            made[(n, m)] = ctx
        return made[(n, m)]
    yield get
    for ctx in made.values():
        ctx.close()


def _bound(session):
    from bulletproofs_amd._lib import transcript_append_message, transcript_new
    return transcript_append_message(transcript_new(b"payment-protocol v3"), b"session", session)


def _sep_wraps(state, n, m):
    """does rangeproof_domain_sep(n, m) cross the 166-byte rate boundary from this state?"""
    from bulletproofs_amd._lib import transcript_append_message
    pos = state[200]
    for label, msg in ((b"dom-sep", b"rangeproof v1"), (b"n", n.to_bytes(8, "little")), (b"m", m.to_bytes(8, "little"))):
        state = transcript_append_message(state, label, msg)
        if state[200] < pos:
            return True
        pos = state[200]
    return False


def _session_states(n, m):
    """five session bindings at five STROBE positions, two of them (found by search) making the separator wrap the rate"""
    plain, wrapping = [], []
    for length in range(1, 300):
        st = _bound(bytes((length + i) & 0xff for i in range(length)))
        (wrapping if _sep_wraps(st, n, m) else plain).append(st)
    assert len(plain) >= 3 and len(wrapping) >= 2
    states = [plain[0], wrapping[0], plain[7], wrapping[len(wrapping) // 2], plain[-1]]
    assert len(set(states)) == 5
    return states


def _shared_cases():
    big = max(_block_sizes()) + 1
    return [(8, 1, big, 0), (64, 1, 65, 0), (32, 4, 5, 0), (64, 16, 2, 0), (8, 2, 3, 1)]


@pytest.mark.parametrize("n,m,nb,ct", _shared_cases())
def test_shared_transcript_is_byte_identical_to_the_expanded_keystream(contexts, n, m, nb, ct):
    """distinct seeds, one bound transcript: proofs, commitments and transcripts_out == the existing entry point's on the draw buffer that
    ChaChaRng::from_seed(seed) would fill; the same with prover_constant_time = 1"""
    ctx = contexts(n, m)
    vals, bl, seeds = _inputs(n, m, nb, b"shared-%d-%d" % (n, m))
    start = _bound(b"one session for all")
    rng = b"".join(_keystream(s, _ndraws(n, m)) for s in seeds)
    ctx.set_option("prover_constant_time", ct)
    try:
        want = ctx.rangeproof_prove_batch(n, m, vals, bl, transcript=start, rng=rng, want_transcripts=True)
        got = ctx.rangeproof_prove_batch_ts(n, m, vals, bl, start, b"".join(seeds), want_transcripts=True)
        assert ctx.get_option("staging_residue") == 0
    finally:
        ctx.set_option("prover_constant_time", 0)
    assert got[1] == want[1] and got[0] == want[0] and got[2] == want[2]
    pl = len(got[0]) // nb
    assert len(set(got[0][pl * i:pl * (i + 1)] for i in range(nb))) == nb


@pytest.mark.parametrize("n,m", [(64, 1), (16, 2)])
def test_one_transcript_per_proof_matches_single_calls_and_the_verifier(contexts, n, m):
    ctx = contexts(n, m)
    nb = 5
    vals, bl, seeds = _inputs(n, m, nb, b"per-proof-%d-%d" % (n, m))
    states = _session_states(n, m)
    proofs, coms, ts = ctx.rangeproof_prove_batch_ts(n, m, vals, bl, b"".join(states), b"".join(seeds), want_transcripts=True)
    pl = len(proofs) // nb
    for p in range(nb):
        one = ctx.rangeproof_prove_batch(n, m, vals[m * p:m * (p + 1)], bl[32 * m * p:32 * m * (p + 1)], transcript=states[p],
                                         rng=_keystream(seeds[p], _ndraws(n, m)), want_transcripts=True)
        assert one == (proofs[pl * p:pl * (p + 1)], coms[32 * m * p:32 * m * (p + 1)], ts[TS * p:TS * (p + 1)]), p
    verdict, vts = ctx.rangeproof_verify_batch_ts(n, m, proofs, pl, coms, b"".join(states), want_transcripts=True)
    assert bytes(verdict) == bytes(nb) and vts == ts
    swapped = list(states)
    swapped[1], swapped[3] = swapped[3], swapped[1]
    verdict, _ = ctx.rangeproof_verify_batch_ts(n, m, proofs, pl, coms, b"".join(swapped), want_transcripts=True)
    assert [v != 0 for v in bytes(verdict)] == [False, True, False, True, False]


def test_library_seeds_give_fresh_proofs_that_verify(contexts):
    n, m, nb = 64, 1, 4
    ctx = contexts(n, m)
    vals, bl, _ = _inputs(n, m, nb, b"lib-seeds")
    start = _bound(b"library seeds")
    a = ctx.rangeproof_prove_batch_ts(n, m, vals, bl, start)
    b = ctx.rangeproof_prove_batch_ts(n, m, vals, bl, start)
    assert ctx.get_option("staging_residue") == 0
    pl = len(a[0]) // nb
    assert a[1] == b[1]
    assert all(a[0][pl * i:pl * (i + 1)] != b[0][pl * i:pl * (i + 1)] for i in range(nb))
    assert len(set(a[0][pl * i:pl * (i + 1)] for i in range(nb))) == nb
    for out in (a, b):
        assert bytes(ctx.rangeproof_verify_batch_ts(n, m, out[0], pl, out[1], start)) == bytes(nb)


def test_equal_rows_give_equal_proofs(contexts):
    n, m = 16, 2
    ctx = contexts(n, m)
    vals, bl, seeds = _inputs(n, m, 3, b"determinism")
    vals[2 * m:3 * m], seeds[2] = vals[0:m], seeds[0]
    bl = bl[:64 * m] + bl[:32 * m]
    st = _session_states(n, m)
    proofs, coms, ts = ctx.rangeproof_prove_batch_ts(n, m, vals, bl, st[1] + st[0] + st[1], b"".join(seeds), want_transcripts=True)
    pl = len(proofs) // 3
    assert proofs[:pl] == proofs[2 * pl:] != proofs[pl:2 * pl]
    assert coms[:32 * m] == coms[64 * m:] and ts[:TS] == ts[2 * TS:]


@pytest.mark.parametrize("n,m,nb", [(64, 1, 65), (8, 2, 3)])
def test_device_pointer_form_on_a_side_stream_gives_the_host_forms_bytes(contexts, n, m, nb):
    import torch
    ctx = contexts(n, m)
    vals, bl, seeds = _inputs(n, m, nb, b"dev-%d-%d" % (n, m))
    states = _session_states(n, m)
    states = b"".join(states[i % 5] for i in range(nb))
    want = ctx.rangeproof_prove_batch_ts(n, m, vals, bl, states, b"".join(seeds), want_transcripts=True)
    want_shared = ctx.rangeproof_prove_batch_ts(n, m, vals, bl, states[:TS], b"".join(seeds))
    dev = torch.device("cuda:0")
    to_dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    pl = len(want[0]) // nb
    side = torch.cuda.Stream(device=dev)
    d_v = torch.tensor([v - (1 << 64) if v >> 63 else v for v in vals], dtype=torch.int64, device=dev)
    d_b, d_t, d_s = to_dev(bl), to_dev(states), to_dev(b"".join(seeds))
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d_p = torch.full((pl * nb,), 255, dtype=torch.uint8, device=dev)
        d_c = torch.full((32 * m * nb,), 255, dtype=torch.uint8, device=dev)
        d_o = torch.full((TS * nb,), 255, dtype=torch.uint8, device=dev)
        ctx.rangeproof_prove_batch_ts_dev(n, m, nb, d_v.data_ptr(), d_b.data_ptr(), d_t.data_ptr(), TS, d_s.data_ptr(), d_p.data_ptr(), d_c.data_ptr(),
                                          d_o.data_ptr(), side.cuda_stream)
        d_p2 = torch.full((pl * nb,), 255, dtype=torch.uint8, device=dev)
        d_c2 = torch.full((32 * m * nb,), 255, dtype=torch.uint8, device=dev)
        ctx.rangeproof_prove_batch_ts_dev(n, m, nb, d_v.data_ptr(), d_b.data_ptr(), d_t.data_ptr(), 0, d_s.data_ptr(), d_p2.data_ptr(), d_c2.data_ptr(),
                                          None, side.cuda_stream)
        d_p3 = torch.full((pl * nb,), 255, dtype=torch.uint8, device=dev)
        d_c3 = torch.full((32 * m * nb,), 255, dtype=torch.uint8, device=dev)
        ctx.rangeproof_prove_batch_ts_dev(n, m, nb, d_v.data_ptr(), d_b.data_ptr(), d_t.data_ptr(), TS, None, d_p3.data_ptr(), d_c3.data_ptr(), None,
                                          side.cuda_stream)
    side.synchronize()
    assert ctx.get_option("staging_residue") == 0          # (before the verifier below stages its public inputs)
    assert (bytes(d_p.cpu().numpy()), bytes(d_c.cpu().numpy()), bytes(d_o.cpu().numpy())) == want
    assert (bytes(d_p2.cpu().numpy()), bytes(d_c2.cpu().numpy())) == want_shared
    # library-drawn seeds through the device form: the same commitments, other proofs, and they verify on their own states
    p3 = bytes(d_p3.cpu().numpy())
    assert bytes(d_c3.cpu().numpy()) == want[1] and all(p3[pl * i:pl * (i + 1)] != want[0][pl * i:pl * (i + 1)] for i in range(nb))
    assert bytes(ctx.rangeproof_verify_batch_ts(n, m, p3, pl, want[1], states)) == bytes(nb)


def test_errors_are_reported_and_nothing_is_left_in_staging(contexts):
    import bulletproofs_amd as bp
    n, m, nb = 8, 2, 3
    ctx = contexts(n, m)
    L = bp.lib()
    vals, bl, seeds = _inputs(n, m, nb, b"errors")
    va = (C.c_uint64 * (nb * m))(*vals)
    states = b"".join(_session_states(n, m)[:nb])
    seeds = b"".join(seeds)
    pr, cm, to = C.create_string_buffer(32 * 17 * nb), C.create_string_buffer(32 * m * nb), C.create_string_buffer(TS * nb)

    def call(n_=n, m_=m, nb_=nb, va_=va, bl_=bl, ts_=states, stride=TS, seeds_=seeds, pr_=pr, cm_=cm):
        rc = L.bpgpu_rangeproof_prove_batch_ts(ctx.h, n_, m_, nb_, va_, bl_, ts_, stride, seeds_, pr_, cm_, to)
        assert ctx.get_option("staging_residue") == 0
        return rc

    assert call() == 0 and pr.raw != bytes(len(pr.raw))
    assert call(nb_=0) == 0 and call(nb_=0, ts_=None, va_=None) == 0
    assert L.bpgpu_rangeproof_prove_batch_ts(None, n, m, nb, va, bl, states, TS, seeds, pr, cm, to) == INVALID_ARG
    for kw in (dict(ts_=None), dict(stride=1), dict(stride=TS - 1), dict(stride=2 * TS), dict(va_=None), dict(bl_=None), dict(pr_=None), dict(cm_=None),
               dict(n_=12), dict(n_=0), dict(n_=128), dict(m_=0), dict(m_=3)):
        assert call(**kw) == INVALID_ARG, kw
    assert call(m_=4, nb_=1) == NO_GENS and call(n_=16, m_=1) == NO_GENS          # InvalidGeneratorsLength
    big = (C.c_uint64 * (nb * m))(*vals)
    big[nb * m - 1] = 1 << n
    assert call(va_=big) == INVALID_ARG                                          # a value that does not fit n bits
    for at, byte in ((200, 166), (200, 255), (201, 167)):                          # every state is checked, the last one too
        bad = bytearray(states)
        bad[TS * (nb - 1) + at] = byte
        assert call(ts_=bytes(bad)) == INVALID_ARG
        assert call(ts_=bytes(bad[TS * (nb - 1):]), stride=0) == INVALID_ARG
    # the device form checks what it can without reading device memory
    assert L.bpgpu_rangeproof_prove_batch_ts_dev(ctx.h, n, m, 0, None, None, None, 0, None, None, None, None, None) == 0
    assert L.bpgpu_rangeproof_prove_batch_ts_dev(ctx.h, n, m, nb, 256, 256, None, 0, None, 256, 256, None, None) == INVALID_ARG
    assert L.bpgpu_rangeproof_prove_batch_ts_dev(ctx.h, n, m, nb, 256, 256, 256, 7, None, 256, 256, None, None) == INVALID_ARG
    assert L.bpgpu_rangeproof_prove_batch_ts_dev(ctx.h, 12, m, nb, 256, 256, 256, 0, None, 256, 256, None, None) == INVALID_ARG
    assert L.bpgpu_rangeproof_prove_batch_ts_dev(ctx.h, n, m, nb, 256, 256, 258, 0, None, 256, 256, None, None) == INVALID_ARG   # misaligned
    assert ctx.get_option("staging_residue") == 0
    assert call() == 0


def test_python_api_proves_a_batch_on_a_list_of_transcripts():
    from bulletproofs_amd import api
    n, m, nb = 32, 1, 3
    gens = api.BulletproofGens(n, m, fixed_window_bits=12)
    pc = gens.pedersen()
    vals, bl, seeds = _inputs(n, m, nb, b"api")
    values = [vals[m * i:m * (i + 1)] for i in range(nb)]
    blindings = [[bl[32 * (m * i + j):32 * (m * i + j) + 32] for j in range(m)] for i in range(nb)]

    def sessions():
        out = []
        for i in range(nb):
            t = api.Transcript(b"payment-protocol v3")
            t.append_message(b"session", b"id-%d" % i * (1 + 9 * i))
            out.append(t)
        return out
    provers, verifiers = sessions(), sessions()
    res = api.RangeProof.prove_batch(gens, pc, provers, values, blindings, n, b"".join(seeds))
    assert len(res) == nb
    for i, (proof, coms) in enumerate(res):
        assert len(coms) == m
        proof.verify_single(gens, pc, verifiers[i], coms[0], n)
        assert verifiers[i].state == provers[i].state and provers[i].fresh_label is None
    # a proof does not verify on another session's transcript
    with pytest.raises(api.ProofError):
        res[0][0].verify_single(gens, pc, sessions()[1], res[0][1][0], n)
    # the keyword of the single-proof calls takes the same path: the same bytes as the batch's first row
    t = sessions()[0]
    one, coms = api.RangeProof.prove_multiple_with_rng(gens, pc, t, values[0], blindings[0], n, rng_seed32=seeds[0])
    assert one.to_bytes() == res[0][0].to_bytes() and coms == res[0][1] and t.state == provers[0].state
    # one bound transcript for all: not advanced, every proof verifies on a copy of it
    shared = sessions()[2]
    before = shared.state
    res = api.RangeProof.prove_batch(gens, pc, shared, values, blindings, n)
    assert shared.state == before
    for proof, coms in res:
        proof.verify_single(gens, pc, shared.clone(), coms[0], n)
    gens.ctx.close()
