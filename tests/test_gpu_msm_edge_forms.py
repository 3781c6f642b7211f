"""Edge scalars through every MSM form the options reach, bit-exact against the oracle.  A scalar drawn uniformly mod l has
bit 252 set with probability ~2^-127, so random-scalar tests never fill the top radix-16 digit or the top bucket window; these
MSMs do: l - 1, l - 2, 2^252 +- 1, (l +- 1) / 2, 2^64 / 2^128 / 2^192 boundaries, and 2^(c-1), 2^(c-1) - 1, 2^c - 1, l - 2^(c-1) for
the window widths c in play, with runs of equal scalars (one crowded bucket), a repeated point, P beside -P, the identity
encoding and a term set that sums to the identity.  Non-canonical scalars must give status 2 and an undecodable point status 1
in every form, without touching the other MSMs of the batch."""
import ctypes as C
import hashlib

import pytest

import bp_twin as T
import limb_corpus as LC

pytestmark = pytest.mark.gpu

L = T.L
ZERO = bytes(32)


def _pts(oracle, tag, n):
    out = C.create_string_buffer(32)
    r = []
    for i in range(n):
        oracle.lib().oracle_from_uniform_bytes(hashlib.shake_256(b"%s-%d" % (tag, i)).digest(64), out)
        r.append(out.raw)
    return r


def _neg(p):
    return T.compress(T.pt_neg(T.decompress(p)))


def _enc(xs):
    return b"".join(x.to_bytes(32, "little") for x in xs)


def _edge_msms(oracle):
    """[(scalars, points)] -- every MSM within the narrow form's limits (at most 16 MSMs, 768 terms in all)."""
    es = LC.msm_edge_scalars()
    pts = _pts(oracle, b"edge-forms", len(es))
    msms = [(es, pts)]
    msms.append((es, [pts[3]] * len(es)))                                               # one point repeated
    runs = [L - 1] * 6 + [2**252] * 5 + [2**16 - 1] * 5 + [1] * 4
    msms.append((runs, pts[:len(runs)]))                                                # runs of equal scalars: one bucket crowded
    pm = es[:12]
    msms.append((pm + pm, pts[:12] + [_neg(p) for p in pts[:12]]))                     # P beside -P, equal scalars: identity
    msms.append((es[:10] + [L - x for x in es[1:10]], pts[:10] + pts[1:10]))           # s P + (l - s) P for every P (but one)
    msms.append((es[:8] + [5, L - 1], pts[:8] + [ZERO, ZERO]))                          # the identity encoding among the points
    msms.append(([L - 1], [pts[0]]))
    msms.append(([2**252 + 1, 2**252 - 1], [pts[1], _neg(pts[1])]))
    return [(_enc(s), b"".join(p)) for s, p in msms]


def _run_batch(call, oracle, msms):
    nt = [len(s) // 32 for s, _ in msms]
    out, st = call(nt, b"".join(s for s, _ in msms), b"".join(p for _, p in msms))
    for k, (s, p) in enumerate(msms):
        assert st[k] == 0 and out[32 * k:32 * k + 32] == oracle.msm(s, p)[1], k
    # a non-canonical scalar in one MSM -> status 2 there; an undecodable point in another -> status 1; the rest unchanged
    for bad in LC.NONCANONICAL_SCALARS:
        s0 = bytearray(msms[0][0])
        s0[32 * 3:32 * 4] = bad.to_bytes(32, "little")
        p1 = bytearray(msms[1][1])
        p1[0] |= 1
        mod = [(bytes(s0), msms[0][1]), (msms[1][0], bytes(p1))] + msms[2:]
        out, st = call(nt, b"".join(s for s, _ in mod), b"".join(p for _, p in mod))
        assert st[0] == 2 and st[1] == 1, (hex(bad), st[:2])
        for k in range(2, len(msms)):
            assert st[k] == 0 and out[32 * k:32 * k + 32] == oracle.msm(*msms[k])[1], (hex(bad), k)


@pytest.mark.parametrize("narrow", [0, 1])
def test_edge_scalars_msm_batch_narrow_and_batch_forms(oracle, narrow):
    import bulletproofs_amd as bp
    c = bp.Context(0)
    c.set_option("msm_narrow", narrow)
    _run_batch(c.msm_batch, oracle, _edge_msms(oracle))
    c.close()


def test_edge_scalars_every_bucket_form(oracle):
    import bulletproofs_amd as bp
    msms = _edge_msms(oracle)
    c = bp.Context(0)
    c.set_option("msm_narrow", 0)
    c.set_option("bucket_min_terms", 1)
    for chain in (0, 1):
        for lanes in (64, 128, 256):
            for tail in (0, 1):
                c.set_option("bucket_chain", chain)
                c.set_option("bucket_lanes", lanes)
                c.set_option("bucket_fast_tail", tail)
                _run_batch(c.msm_batch, oracle, msms)
    c.close()


def test_edge_scalars_pool_msm_batch(oracle):
    import bulletproofs_amd as bp
    pool = bp.Pool((0,), 2)
    _run_batch(pool.msm_batch, oracle, _edge_msms(oracle))
    pool.close()


@pytest.mark.parametrize("W", [2, 5, 12, 17])   # 17: the first W above 16 that saves a window (fb_nwin)
def test_edge_scalars_msm_batch_shared_every_window_and_fork(oracle, W):
    import bulletproofs_amd as bp
    n, m = 8, 1
    ngen = 2 * n * m + 2
    g = oracle.Gens(n, m)
    G, H, B, Bb = g.export()
    gen_pts = Bb + B + G[:32 * n] + H[:32 * n]
    es = LC.msm_edge_scalars()
    up = _pts(oracle, b"shared-edge", 6)
    uq = [up[0], up[0], _neg(up[0]), ZERO, up[1], up[2]]
    nu = len(uq)
    batches = []
    for b in range(6):   # generator scalars and own scalars from the edge list, rotated per MSM
        gs = [es[(b * 5 + i) % len(es)] for i in range(ngen)]
        us = [es[(b * 7 + 3 * i) % len(es)] for i in range(nu)]
        batches.append((gs, us))
    batches.append(([L - 1] * ngen, [L - 1, 1, L - 1, 3, 2**252, 2**252]))
    for fork in (0, 1):
        c = bp.Context(0, fixed_window_bits=W)
        c.set_option("msm_fork", fork)
        c.gens_load(n, m, G, H, B, Bb)
        GS = b"".join(_enc(gs) for gs, _ in batches)
        US = b"".join(_enc(us) for _, us in batches)
        UP = b"".join(uq) * len(batches)
        out, st = c.msm_batch_shared(n, m, len(batches), nu, GS, US, UP)
        for k, (gs, us) in enumerate(batches):
            exp = oracle.msm(_enc(gs) + _enc(us), gen_pts + b"".join(uq))
            assert st[k] == 0 and out[32 * k:32 * k + 32] == exp[1], (W, fork, k)
        for bad in LC.NONCANONICAL_SCALARS:
            for where in ("gen", "own"):
                gs2, us2 = bytearray(GS), bytearray(US)
                if where == "gen":
                    gs2[32 * 4:32 * 5] = bad.to_bytes(32, "little")
                else:
                    us2[32 * 1:32 * 2] = bad.to_bytes(32, "little")
                up2 = bytearray(UP)
                up2[32 * nu + 32 * 5] |= 1                                          # MSM 1: an undecodable own point
                out2, st2 = c.msm_batch_shared(n, m, len(batches), nu, bytes(gs2), bytes(us2), bytes(up2))
                assert st2[0] == 2 and st2[1] == 1, (W, fork, where, hex(bad), st2[:2])
                assert st2[2:] == st[2:] and out2[64:] == out[64:], (W, fork, where, hex(bad))
        c.close()
