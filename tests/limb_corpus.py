"""Corner-case corpora and big-int references for the three limb arithmetics (fe25519.h's 10 x 25.5-bit field limbs,
horner_wave.h's 16 x 16-bit wavefront limbs, sc25519.h's 10 x 28-bit Montgomery limbs), shared by the host tests
(test_limb_bounds_on_cpu.py, through the CPU harness) and the device tests (test_gpu_limb_bounds.py, through
tests/gpu_prims).  Every corpus stays inside the input contract its primitive documents; the reference reads the limbs
at their weights with Python big ints.  Test-only."""
import ctypes as C
import random

import bp_twin as T
import point_corpus as PC

P, L = T.P, T.L

# ---- radices --------------------------------------------------------------------------------------------------------
FE_W = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]          # limb i of a field element sits at 2^ceil(25.5 i)
SC_W = [28 * i for i in range(10)]
HW_W = [16 * i for i in range(16)]


def val(limbs, w):
    return sum(x << s for x, s in zip(limbs, w))


def split(v, w):
    """v in the radix w, canonical limbs except the top one, which takes the rest."""
    out = []
    for i in range(len(w) - 1):
        out.append((v >> w[i]) & ((1 << (w[i + 1] - w[i])) - 1))
    out.append(v >> w[-1])
    return out


# ---- the bounds the sources state -----------------------------------------------------------------------------------
FE_REDUCED = [0x407ffff if i % 2 == 0 else 0x207ffff for i in range(10)]   # < 2^26 (25) + 2^19
FE_LAZY = [0xc200000 if i % 2 == 0 else 0x6100000 for i in range(10)]      # fe_check_lazy
FE_CARRY_IN = [0xffffff7f] * 10                                            # fe_carry: limbs < 2^32 - 2^7
FE_COLMAX = 10 * (2 * 0x6100000) * (19 * 0xc200000)                        # fe_mul's column sums at lazy inputs
SC28_MAX = 2**28 + 4
HW_SMALL = 2**16 + 38 * 2**10                                              # hw_norm's output bound
HW_MUL_IN = 2**21
HW_SUB_B = 2**18 - 8
HW_NORM_IN = 2**26 - 1
HW_TO_FE_IN = 2**17


def _values():
    """Field-sized values with long carry runs."""
    vs = [0, 1, 2, 19, 38, P - 2, P - 1, 2**255 - 1, 2**256 - 1, 2**255, 2**255 + 18]
    vs += [P + i for i in range(19)]
    for k in (16, 25, 26, 51, 64, 128, 127, 192, 230, 254):
        vs += [2**k - 1, 2**k, 2**k + 1]
    return vs


def limb_corpus(bound, w, seed, nrand=200, values=True):
    """Limb vectors with every limb <= bound[i]: maxima, alternating maxima, single maxima, all-0xffff-style carry runs,
    the values of _values() in radix w (where they fit), 2^k +- 1, and nrand seeded random vectors."""
    n = len(bound)
    cs = [list(bound), [0] * n]
    cs.append([bound[i] if i % 2 == 0 else 0 for i in range(n)])
    cs.append([bound[i] if i % 2 == 1 else 0 for i in range(n)])
    for i in range(n):
        cs.append([bound[j] if j == i else 0 for j in range(n)])
    for i in range(n):   # every limb full except one
        cs.append([bound[j] if j != i else 0 for j in range(n)])
    full = [(1 << (w[i + 1] - w[i])) - 1 if i + 1 < n else (1 << 16) - 1 for i in range(n)]
    cs.append([min(full[i], bound[i]) for i in range(n)])            # all limbs 2^26 - 1 / 2^25 - 1 / 0xffff / 2^28 - 1
    cs.append([min(full[i] + 1, bound[i]) for i in range(n)])
    if values:
        for v in _values():
            cs.append(split(v, w))
    rng = random.Random(seed)
    for _ in range(nrand):
        kind = rng.randrange(3)
        if kind == 0:
            cs.append([rng.randint(0, b) for b in bound])
        elif kind == 1:   # near the bound
            cs.append([max(0, b - rng.randrange(64)) for b in bound])
        else:
            cs.append([rng.randint(0, b) if rng.random() < 0.5 else b for b in bound])
    return [c for c in cs if all(0 <= x <= b for x, b in zip(c, bound))]


def pairs(corpus, seed):
    """(a, b) pairs: every vector against a rotated copy of the corpus and against itself."""
    rng = random.Random(seed)
    n = len(corpus)
    out = [(corpus[i], corpus[(i * 7 + 3) % n]) for i in range(n)]
    out += [(corpus[i], corpus[i]) for i in range(0, n, 5)]
    out += [(corpus[rng.randrange(n)], corpus[rng.randrange(n)]) for _ in range(n // 2)]
    return out


def sc28_corpus(seed, nrand=200):
    """sc28 lazy inputs: limbs <= 2^28 + 4 and value < 2^254, with values just below 2^254 and the low limbs pushed to 2^28 + 4."""
    cs = limb_corpus([SC28_MAX] * 9 + [3], SC_W, seed, nrand)
    for v in (L - 2, L - 1, L, L + 1, 2 * L, 3 * L, 2**252 - 1, 2**252, 2**253, 2**254 - 1, 2**254 - 2**28, 2**254 - 2**252 - 1):
        cs.append(split(v, SC_W))
    for top in range(4):
        for lo in (2**28, 2**28 + 1, SC28_MAX):
            cs.append([lo] * 9 + [top])
            cs.append([lo if i % 2 == 0 else 2**28 - 1 for i in range(9)] + [top])
    rng = random.Random(seed + 1)
    for _ in range(64):   # the same value with some low limbs borrowing from the next: limbs in [2^28, 2^28 + 4]
        c = split(rng.randrange(2**253, 2**254), SC_W)
        for i in range(9):
            if c[i] <= 4 or rng.random() < 0.5:
                if c[i] <= 4 and c[i + 1] > 0:
                    c[i] += 2**28
                    c[i + 1] -= 1
        cs.append(c)
    return [c for c in cs if all(0 <= x <= SC28_MAX for x in c) and val(c, SC_W) < 2**254]


# ---- ctypes plumbing -------------------------------------------------------------------------------------------------
def u32(rows):
    flat = [x for r in rows for x in r]
    return (C.c_uint32 * max(1, len(flat)))(*flat)


def u64(rows):
    flat = [x for r in rows for x in r]
    return (C.c_uint64 * max(1, len(flat)))(*flat)


def u16(rows):
    flat = [x for r in rows for x in r]
    return (C.c_uint16 * max(1, len(flat)))(*flat)


class Backend:
    """The raw-limb calls of one build: prefix 'h_' (CPU harness) or 'g_' (GPU module); the same signatures."""

    def __init__(self, lib, prefix):
        self.lib, self.p = lib, prefix

    def _f(self, name):
        return getattr(self.lib, self.p + name)

    def _call(self, name, *args):
        rc = self._f(name)(*args)
        assert rc == 0, (self.p + name, rc)

    def fe(self, op, A, B, width=10):
        n = len(A)
        out, ok = (C.c_uint32 * (10 * n))(), (C.c_uint8 * n)()
        self._call("fe_raw", op, n, u32(A), u32(B), out, ok)
        return [list(out[10 * i:10 * i + width]) for i in range(n)], list(ok)

    def fe_cols(self, cols):
        n = len(cols)
        out, ok = (C.c_uint32 * (10 * n))(), (C.c_uint8 * n)()
        self._call("fe_cols_raw", n, u64(cols), out, ok)
        return [list(out[10 * i:10 * i + 10]) for i in range(n)], list(ok)

    def limbs_to_fe(self, L16):
        n = len(L16)
        out, ok = (C.c_uint32 * (10 * n))(), (C.c_uint8 * n)()
        self._call("limbs_to_fe_raw", n, u32(L16), out, ok)
        return [list(out[10 * i:10 * i + 10]) for i in range(n)], list(ok)

    def sc(self, op, A, B):
        n = len(A)
        out, ok = (C.c_uint32 * (10 * n))(), (C.c_uint8 * n)()
        self._call("sc_raw", op, n, u32(A), u32(B), out, ok)
        return [list(out[10 * i:10 * i + 10]) for i in range(n)], list(ok)

    def sc_cols(self, cols):
        n = len(cols)
        out, ok = (C.c_uint32 * (10 * n))(), (C.c_uint8 * n)()
        self._call("sc_cols_raw", n, u64(cols), out, ok)
        return [list(out[10 * i:10 * i + 10]) for i in range(n)], list(ok)

    def ge(self, op, Pp, Q):
        n = len(Pp)
        out, ok = (C.c_uint32 * (40 * n))(), (C.c_uint8 * n)()
        self._call("ge_raw", op, n, u32(Pp), u32(Q), out, ok)
        return [list(out[40 * i:40 * i + 40]) for i in range(n)], list(ok)

    def hw(self, op, A, B, nsq=0):
        n = len(A)
        out, ok = (C.c_uint32 * (64 * n))(), (C.c_uint8 * n)()
        self._call("hw_raw", op, n, u32(A), u32(B), nsq, out, ok)
        return [list(out[64 * i:64 * i + 64]) for i in range(n)], list(ok)

    def drv(self, name, n, inp, width, *extra):
        out = (C.c_uint32 * (width * n))()
        self._call("drv_" + name, n, inp, *extra, out)
        return [list(out[width * i:width * i + width]) for i in range(n)]


# ---- op codes (limb_ops.h) -------------------------------------------------------------------------------------------
FE_CARRY, FE_ADD, FE_SUB, FE_SUB_RR, FE_MUL, FE_SQ, FE_TO_WORDS, FE_INVERT, FE_POW22523 = range(9)
SC_MONTMUL, SC_MONTSQ, SC_FROM_MONT, SC_FROM_SC28 = range(4)
GE_ADD_CACHED, GE_SUB_CACHED, GE_MADD, GE_MSUB, GE_DBL, GE_DBL_NO_T, GE_TO_CACHED, GE_FROM_NIELS, GE_FROM_NIELS_NEG = range(9)
HW_NORM, HW_SUB, HW_MUL, HW_SQN, HW_INVSQRT_RAW, HW_DBL, HW_ADD_CACHED, HW_TO_CACHED = range(8)

D2 = 2 * T.D % P
RINV = pow(2**280, -1, L)


def fev(l):
    return val(l, FE_W)


def fe4(l40):
    return [fev(l40[10 * i:10 * i + 10]) % P for i in range(4)]


def hw_rows(l64):
    return [val(l64[16 * r:16 * r + 16], HW_W) for r in range(4)]


def words_val(w):
    return sum(x << (32 * i) for i, x in enumerate(w))


def invsqrt_raw(t):
    """fe_invsqrt_raw / hw_invsqrt_raw: t^3 (t^7)^((p-5)/8)."""
    return pow(t, 3, P) * pow(pow(t, 7, P), (P - 5) // 8, P) % P


# ---- the point formulas, restated -----------------------------------------------------------------------------------
def ge_add_cached(p, q, neg):
    """ge25519.h ge_add_cached; q = (Y+X, Y-X, Z, 2dT)."""
    X, Y, Z, Tt = p
    ypx, ymx, qz, t2d = q
    qa, qb = (ypx, ymx) if neg else (ymx, ypx)             # fe_select(qa, q.YmX, q.YpX, neg) ...
    a, b = (Y - X) * qa, (Y + X) * qb                       # fe_mul(a, ymx, qa); fe_mul(b, ypx, qb)
    c, d = Tt * t2d, 2 * Z * qz                             # fe_mul(c, p.T, q.T2d); d = 2 Z1 Z2
    e, h = b - a, b + a
    f, g = (d + c, d - c) if neg else (d - c, d + c)       # fe_select(f, dmc, dpc, neg); fe_select(g, dpc, dmc, neg)
    return [f * e % P, h * g % P, f * g % P, h * e % P]


def ge_madd(p, q, neg):
    """ge25519.h ge_madd; q = Niels (y+x, y-x, -, 2dxy)."""
    X, Y, Z, Tt = p
    ypx, ymx, _, t2d = q
    qa, qb = (ypx, ymx) if neg else (ymx, ypx)
    a, b = (Y - X) * qa, (Y + X) * qb
    c, d = Tt * t2d, 2 * Z                                   # fe_add(d, p.Z, p.Z)
    e, h = b - a, b + a
    f, g = (d + c, d - c) if neg else (d - c, d + c)
    return [f * e % P, h * g % P, f * g % P, h * e % P]


def ge_dbl(p, with_t=True):
    """ge25519.h ge_dbl (dbl-2008-hwcd with H and F negated); the same formula as hw_dbl."""
    X, Y, Z = p[0], p[1], p[2]
    xx, yy, zz2, s = X * X, Y * Y, 2 * Z * Z, (X + Y) ** 2
    h, g = yy + xx, yy - xx
    e, f = s - h, zz2 - g
    return [f * e % P, h * g % P, f * g % P, (h * e % P) if with_t else 0]


def ge_to_cached(p):
    return [(p[1] + p[0]) % P, (p[1] - p[0]) % P, p[2] % P, p[3] * D2 % P]


def ge_from_niels(q, neg):
    """ge25519.h ge_from_niels: (2e : 2h : 4 : e h)."""
    ypx, ymx = q[0], q[1]
    qa, qb = (ypx, ymx) if neg else (ymx, ypx)
    e, h = qb - qa, qb + qa
    return [2 * e % P, 2 * h % P, 4, e * h % P]


def hw_add_cached(c, q):
    """horner_wave.h hw_add_cached: q in row order (Y-X, Y+X, Z, 2dT)."""
    X, Y, Z, Tt = c
    A, B, ZZ, Cc = (Y - X) * q[0], (Y + X) * q[1], Z * q[2], Tt * q[3]   # the four rows' product
    d = 2 * ZZ
    e, h, f, g = B - A, B + A, d - Cc, d + Cc
    return [e * f % P, h * g % P, g * f % P, e * h % P]             # hw_point_finish


def hw_to_cached(c, d2):
    X, Y, Z, Tt = c
    return [(Y - X) % P, (Y + X) % P, Z % P, Tt * d2 % P]


def hw_horner(colq, nwin, ndbl):
    """hw_horner / hw_horner8: colq[w] = the four rows' values of window w."""
    c = [0, 1, 1, 0]
    for w in range(nwin - 1, -1, -1):
        if w != nwin - 1:
            for _ in range(ndbl):
                c = ge_dbl(c)
        c = hw_add_cached(c, colq[w])
    return c


# ---- the checks: each calls one backend on its corpus, asserts the big-int reference and the stated output bound, and
# returns the raw outputs (the GPU test compares them with the CPU harness's, limb for limb) ----------------------------
def check_fe(B, nrand=200):
    outs = {}
    red = limb_corpus(FE_REDUCED, FE_W, 11, nrand)
    lazy = limb_corpus(FE_LAZY, FE_W, 12, nrand)
    carry_in = limb_corpus(FE_CARRY_IN, FE_W, 13, nrand)
    for op, corpus, ref in ((FE_ADD, red, lambda a, b: a + b), (FE_SUB_RR, red, lambda a, b: a - b),
                            (FE_SUB, lazy, lambda a, b: a - b), (FE_MUL, lazy, lambda a, b: a * b)):
        ab = pairs(corpus, op)
        A, Bv = [a for a, _ in ab], [b for _, b in ab]
        out, ok = B.fe(op, A, Bv)
        for a, b, o, f in zip(A, Bv, out, ok):
            assert fev(o) % P == ref(fev(a), fev(b)) % P, (op, a, b, o)
            assert f, ("bound", op, a, b, o)
        if op == FE_SUB_RR:   # the lazy value the source promises: every limb <= reduced + 2p's limb
            for o in out:
                assert all(x <= FE_REDUCED[i] + (0x7ffffda if i == 0 else (0x7fffffe if i % 2 == 0 else 0x3fffffe)) for i, x in enumerate(o))
        outs[op] = out
    for op, corpus, ref in ((FE_SQ, lazy, lambda a: a * a % P), (FE_CARRY, carry_in, lambda a: a % P),
                            (FE_TO_WORDS, carry_in, lambda a: a % P)):
        out, ok = B.fe(op, corpus, corpus)
        for a, o, f in zip(corpus, out, ok):
            got = words_val(o[:8]) if op == FE_TO_WORDS else fev(o) % P
            assert got == ref(fev(a)), (op, a, o)
            assert f, ("bound", op, a, o)
        outs[op] = out
    few = lazy[:40] + lazy[-24:]
    for op, ref in ((FE_INVERT, lambda a: pow(a, P - 2, P)), (FE_POW22523, lambda a: pow(a, (P - 5) // 8, P))):
        out, ok = B.fe(op, few, few)
        for a, o, f in zip(few, out, ok):
            assert fev(o) % P == ref(fev(a) % P) and f, (op, a, o)
        outs[op] = out
    # fe_reduce_columns: column sums up to what fe_mul forms from lazy inputs
    cols = limb_corpus([FE_COLMAX] * 10, FE_W, 14, nrand, values=False)
    out, ok = B.fe_cols(cols)
    for c, o, f in zip(cols, out, ok):
        assert fev(o) % P == val(c, FE_W) % P and f, (c, o)
    outs["cols"] = out
    return outs


def check_limbs_to_fe(B, nrand=300):
    corpus = limb_corpus([HW_TO_FE_IN] * 16, HW_W, 21, nrand)
    corpus.append([0xffff] * 15 + [0x1ffff])          # 2^257 - 1 = 75 (mod p): two carries out of limb 15
    corpus.append([0x1ffff] * 16)
    corpus.append([0x1ffff] * 15 + [0x10000])
    out, ok = B.limbs_to_fe(corpus)
    for l, o, f in zip(corpus, out, ok):
        assert fev(o) % P == val(l, HW_W) % P, (l, o)
        assert f, ("bound", l, o)
    return out


def check_sc(B, nrand=200):
    outs = {}
    corpus = sc28_corpus(31, nrand)
    ab = pairs(corpus, 32)
    A, Bv = [a for a, _ in ab], [b for _, b in ab]
    for op, args, ref in ((SC_MONTMUL, (A, Bv), lambda a, b: a * b * RINV % L), (SC_MONTSQ, (corpus, corpus), lambda a, b: a * a * RINV % L),
                          (SC_FROM_MONT, (corpus, corpus), lambda a, b: a * RINV % L), (SC_FROM_SC28, (corpus, corpus), lambda a, b: a % L)):
        out, ok = B.sc(op, *args)
        for a, b, o, f in zip(args[0], args[1], out, ok):
            va, vb = val(a, SC_W), val(b, SC_W)
            if op == SC_FROM_SC28:
                assert words_val(o[:8]) == ref(va, vb), (op, a, o)
            else:
                assert val(o, SC_W) % L == ref(va, vb) and val(o, SC_W) < 2**254, (op, a, b, o)
            assert f, ("bound", op, a, b, o)
        outs[op] = out
    # sc28_montreduce on the schoolbook columns of lazy pairs (what sc28_montmul / sc28_montsq hand it)
    cols = []
    for a, b in ab:
        t = [0] * 20
        for i in range(10):
            for j in range(10):
                t[i + j] += a[i] * b[j]
        cols.append(t)
    out, ok = B.sc_cols(cols)
    for t, o, f in zip(cols, out, ok):
        assert val(o, SC_W) % L == val(t, [28 * i for i in range(20)]) * RINV % L and val(o, SC_W) < 2**254 and f, (t, o)
    outs["cols"] = out
    return outs


def _fe_pool(seed):
    """Field elements with reduced limbs: at the bound, carry runs, values >= p, random."""
    return limb_corpus(FE_REDUCED, FE_W, seed, 60)


def check_ge(B):
    outs = {}
    pool = _fe_pool(41)
    n = len(pool)
    rng = random.Random(42)
    Pp, Q = [], []
    for i in range(n):   # coordinate i, i+1, ... of the pool; every 4th case all four at the limb bound
        if i % 4 == 0:
            Pp.append(FE_REDUCED * 4)
            Q.append(pool[i] + FE_REDUCED * 3)
        else:
            Pp.append(sum((pool[(i + k) % n] for k in range(4)), []))
            Q.append(sum((pool[rng.randrange(n)] for k in range(4)), []))
    for op in range(9):
        out, ok = B.ge(op, Pp, Q)
        for p, q, o, f in zip(Pp, Q, out, ok):
            pv, qv = [fev(p[10 * k:10 * k + 10]) for k in range(4)], [fev(q[10 * k:10 * k + 10]) for k in range(4)]
            exp = {GE_ADD_CACHED: lambda: ge_add_cached(pv, qv, False), GE_SUB_CACHED: lambda: ge_add_cached(pv, qv, True),
                   GE_MADD: lambda: ge_madd(pv, qv, False), GE_MSUB: lambda: ge_madd(pv, qv, True),
                   GE_DBL: lambda: ge_dbl(pv), GE_DBL_NO_T: lambda: ge_dbl(pv, False), GE_TO_CACHED: lambda: ge_to_cached(pv),
                   GE_FROM_NIELS: lambda: ge_from_niels(qv, False), GE_FROM_NIELS_NEG: lambda: ge_from_niels(qv, True)}[op]()
            assert fe4(o) == [x % P for x in exp], (op, p, q)
            assert f, ("bound", op, p, q, o)
        outs[op] = out
    return outs


def _hw_case(rows):
    return [x for r in rows for x in r]


def check_hw(B, nrand=60):
    """One wavefront per case: row r of a case is limb vector r of the corpus (four field elements at once)."""
    outs = {}

    def waves(bound, seed, n=nrand):
        c = limb_corpus([bound] * 16, HW_W, seed, n)
        return [_hw_case([c[(4 * i + r) % len(c)] for r in range(4)]) for i in range((len(c) + 3) // 4)] + \
               [_hw_case([c[(i + 5 * r) % len(c)] for r in range(4)]) for i in range(len(c))]

    def canon(seed, n):
        rng = random.Random(seed)
        vs = [0, 1, P - 1, P - 19, 2**255 - 20, 2**128, 2**240 - 1] + [rng.randrange(P) for _ in range(n)]
        return [split(v, HW_W) for v in vs]

    def check(op, A, Bv, ref, nsq=0):
        out, ok = B.hw(op, A, Bv, nsq)
        for a, b, o, f in zip(A, Bv, out, ok):
            assert [x % P for x in hw_rows(o)] == [x % P for x in ref(hw_rows(a), hw_rows(b))], (op, a, b, o)
            assert f and max(o) <= HW_SMALL, ("bound", op, a, b, o)
        outs[(op, nsq)] = out

    norm_in = waves(HW_NORM_IN, 51)
    check(HW_NORM, norm_in, norm_in, lambda a, b: a)
    mul_in = waves(HW_MUL_IN, 52)
    sub_b = waves(HW_SUB_B, 53)
    check(HW_SUB, mul_in, [sub_b[i % len(sub_b)] for i in range(len(mul_in))], lambda a, b: [x - y for x, y in zip(a, b)])
    mul_b = mul_in[1:] + mul_in[:1]
    check(HW_MUL, mul_in, mul_b, lambda a, b: [x * y for x, y in zip(a, b)])
    for nsq in (1, 3):
        check(HW_SQN, mul_in, mul_in, lambda a, b: [pow(x, 2**nsq, P) for x in a], nsq)
    small = waves(HW_SMALL, 54, 24)
    cv = canon(55, 60)
    cq = [_hw_case([cv[(i + r) % len(cv)] for r in range(4)]) for i in range(len(small))]
    check(HW_INVSQRT_RAW, small[:24] + cq[:24], small[:24] + cq[:24], lambda a, b: [invsqrt_raw(x % P) for x in a])
    check(HW_DBL, small, small, lambda a, b: ge_dbl(a))
    check(HW_ADD_CACHED, small, cq, lambda a, b: hw_add_cached(a, b))
    d2 = _hw_case([split(D2, HW_W)] * 4)
    check(HW_TO_CACHED, small, [d2] * len(small), lambda a, b: hw_to_cached(a, D2))
    return outs


# ---- horner_wave.h's drivers (host and device copies) ----------------------------------------------------------------
def driver_points(n, tag):
    import hashlib
    return [T.from_uniform_bytes(hashlib.shake_256(tag + b"%d" % i).digest(64)) for i in range(n)]


def fe_limbs(v):
    return split(v % P, FE_W)


def pt_limbs(p):
    return sum((fe_limbs(c) for c in p), [])


def affine(p):
    zi = pow(p[2], P - 2, P)
    return p[0] * zi % P, p[1] * zi % P


def check_drivers(B, decode_encodings):
    """The seven drivers' outputs against the big-int restatement (and, for decode, against RFC 9496); returns the outputs."""
    outs = {}
    rng = random.Random(61)
    ts = [0, 1, 2, P - 1, 2**255 - 20, 2**128] + [rng.randrange(P) for _ in range(26)]
    out = B.drv("invsqrt", len(ts), u32([[(t >> (32 * i)) & 0xffffffff for i in range(8)] for t in ts]), 10)
    for t, o in zip(ts, out):
        assert fev(o) % P == invsqrt_raw(t), t
    outs["invsqrt"] = out
    enc = decode_encodings
    out = B.drv("decode", len(enc), u32([[int.from_bytes(e[4 * i:4 * i + 4], "little") for i in range(8)] for e in enc]), 40)
    for e, o in zip(enc, out):
        d = T.decompress(e)
        v = fe4(o)
        if d is not None:
            assert v[2] == 1 and affine(v) == affine(d) and v[3] == v[0] * v[1] % P, e.hex()
        # rejected encodings as well: the driver gives no verdict and the narrow chain doubles its output 128 times, so the
        # coordinates must be the RFC's formulas carried to the end (what the lane decoder leaves behind)
        failed, full = PC.decode_full(e)
        assert (d is None) == bool(failed) and tuple(v) == full, (e.hex(), "".join(sorted(failed)))
    outs["decode"] = out
    pts = driver_points(6, b"drv")
    pts[1] = tuple(2 * c % P for c in pts[1])                   # Z != 1
    pin = u32([pt_limbs(p) for p in pts])
    for n in (1, 64, 128, 192):
        out = B.drv("point_shift", len(pts), pin, 40, n)
        for p, o in zip(pts, out):
            e = list(p)
            for _ in range(n):
                e = ge_dbl(e)
            assert fe4(o) == e, n
            assert affine(fe4(o)) == affine(T.pt_mul(2**n, p))
        outs[("shift", n)] = out
        out = B.drv("shift_table8", len(pts), pin, 320, n)
        for p, o in zip(pts, out):
            cur = list(p)
            for _ in range(n):
                cur = ge_dbl(cur)
            c1 = hw_to_cached(cur, D2)
            for e in range(8):
                if e:
                    cur = hw_add_cached(cur, c1)
                ce = hw_to_cached(cur, D2)
                ypx, ymx, z, t2d = fe4(o[40 * e:40 * e + 40])   # ge_cached: (Y+X, Y-X, Z, 2dT)
                assert [ymx, ypx, z, t2d] == ce, (n, e)
        outs[("table8", n)] = out
    for name, nwin, ndbl in (("horner", 64, 4), ("horner8", 32, 8)):
        cases = []
        for i in range(3):   # window sums: canonical field values, or 0xffff-heavy values just below p, or cached points
            if i == 0:
                q = [[rng.randrange(P) for _ in range(4)] for _ in range(nwin)]
            elif i == 1:
                q = [[P - 1 - rng.randrange(2**20) for _ in range(4)] for _ in range(nwin)]
            else:
                ps = driver_points(nwin, b"hq")
                q = [[(p[1] - p[0]) % P, (p[1] + p[0]) % P, p[2], p[3] * D2 % P] for p in ps]
            cases.append(q)
        col = u16([sum((split(v, HW_W) for v in w), []) for q in cases for w in q])
        out = B.drv(name, len(cases), col, 40)
        for q, o in zip(cases, out):
            assert fe4(o) == hw_horner(q, nwin, ndbl), name
        outs[name] = out
    return outs


# ---- edge scalars for the MSM forms (the CPU harness's lists gathered, plus the window edges of every width in play) ------
def msm_edge_scalars(widths=(2, 4, 5, 8, 12, 17)):
    s = [0, 1, 2, L - 1, L - 2, 2**252 - 1, 2**252, 2**252 + 1, (L - 1) // 2, (L + 1) // 2, 2**64, 2**128 - 1, 2**128, 2**192,
         (2**124 - 1) << 128, int("8" * 64, 16) % L, int("8" * 63, 16) % L, 7, 8]
    for c in widths:
        s += [2**(c - 1), 2**(c - 1) - 1, 2**c - 1, L - 2**(c - 1)]
    assert all(0 <= x < L for x in s)
    return s


NONCANONICAL_SCALARS = [L, L + 1, 2**253, 2**255, 2**256 - 1]
