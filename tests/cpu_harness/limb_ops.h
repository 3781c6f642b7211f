// Raw-limb wrappers around the field, scalar, point and wavefront primitives: limb arrays in, limb arrays out, so that a
// test can hand a primitive any input inside its documented contract (limbs at their maximum, long carry runs, values in
// [p, 2^256)) instead of only what a 32-byte encoding loads to.  Each wrapper returns whether its output met the bound the
// source states -- a flag, never an assert.  Shared by the CPU harness (harness.cpp, the host build of the headers) and the
// GPU test module (tests/gpu_prims/prims.hip, the device build), which run the identical call on the identical corpus.
// TEST-ONLY.
#ifndef BPGPU_TEST_LIMB_OPS_H
#define BPGPU_TEST_LIMB_OPS_H
#include "../../bulletproofs_amd/csrc/fe25519.h"
#include "../../bulletproofs_amd/csrc/ge25519.h"
#include "../../bulletproofs_amd/csrc/sc25519.h"
#include "../../bulletproofs_amd/csrc/horner_wave.h"

namespace lo {
using namespace bp;

// fe25519.h's limb discipline
BP_HD bool is_reduced(const fe &f) {
    bool ok = true;
    for (int i = 0; i < 10; i++) ok = ok && f.v[i] < ((i & 1) ? 0x2080000u : 0x4080000u);   // 2^25(26) + 2^19
    return ok;
}
BP_HD bool is_lazy(const fe &f) {
    bool ok = true;
    for (int i = 0; i < 10; i++) ok = ok && f.v[i] <= ((i & 1) ? 0x6100000u : 0xc200000u);
    return ok;
}
// 8 words < p = 2^255 - 19
BP_HD bool words_below_p(const uint32_t w[8]) {
    bool top = w[7] == 0x7fffffffu;
    for (int i = 1; i < 7; i++) top = top && w[i] == 0xffffffffu;
    return w[7] <= 0x7fffffffu && !(top && w[0] >= 0xffffffedu);
}
// sc25519.h's lazy 10 x 28-bit form (the value bound < 2^254 is checked by the caller)
BP_HD bool is_sc28_lazy(const sc28 &a) {
    bool ok = true;
    for (int i = 0; i < 10; i++) ok = ok && a.v[i] <= 0x10000004u;
    return ok;
}

BP_HD void ld(fe &f, const uint32_t *a) {
    for (int i = 0; i < 10; i++) f.v[i] = a[i];
}
BP_HD void st(uint32_t *o, const fe &f) {
    for (int i = 0; i < 10; i++) o[i] = f.v[i];
}

enum { FE_CARRY, FE_ADD, FE_SUB, FE_SUB_RR, FE_MUL, FE_SQ, FE_TO_WORDS, FE_INVERT, FE_POW22523, FE_NOPS };

// a, b, out: 10 limbs (FE_TO_WORDS: 8 words + 2 zeros)
BP_HD bool fe_raw(int op, const uint32_t *a, const uint32_t *b, uint32_t *out) {
    fe x, y, r;
    ld(x, a);
    ld(y, b);
    fe_0(r);
    bool ok = false;
    switch (op) {
    case FE_CARRY: r = x; fe_carry(r); ok = is_reduced(r); break;
    case FE_ADD: fe_add(r, x, y); ok = is_lazy(r); break;
    case FE_SUB: fe_sub(r, x, y); ok = is_reduced(r); break;
    case FE_SUB_RR: fe_sub_rr(r, x, y); ok = is_lazy(r); break;
    case FE_MUL: fe_mul(r, x, y); ok = is_reduced(r); break;
    case FE_SQ: fe_sq(r, x); ok = is_reduced(r); break;
    case FE_TO_WORDS: {
        uint32_t w[8];
        fe_to_words(w, x);
        for (int i = 0; i < 8; i++) r.v[i] = w[i];
        ok = words_below_p(w);
    } break;
    case FE_INVERT: fe_invert(r, x); ok = is_reduced(r); break;
    case FE_POW22523: fe_pow22523(r, x); ok = is_reduced(r); break;
    default: break;
    }
    st(out, r);
    return ok;
}
// ten 64-bit column sums -> reduced limbs
BP_HD bool fe_cols_raw(const uint64_t *c, uint32_t *out) {
    uint64_t t[10];
    for (int i = 0; i < 10; i++) t[i] = c[i];
    fe r;
    fe_reduce_columns(r, t);
    st(out, r);
    return is_reduced(r);
}
// 16 lazy radix-2^16 limbs -> field element
BP_HD bool limbs_to_fe_raw(const uint32_t *l16, uint32_t *out) {
    uint32_t l[16];
    for (int i = 0; i < 16; i++) l[i] = l16[i];
    fe r;
    hw_limbs_to_fe(r, l);
    st(out, r);
    return is_reduced(r);
}

enum { SC_MONTMUL, SC_MONTSQ, SC_FROM_MONT, SC_FROM_SC28, SC_NOPS };

// a, b, out: 10 limbs (SC_FROM_SC28: 8 canonical words + 2 zeros)
BP_HD bool sc_raw(int op, const uint32_t *a, const uint32_t *b, uint32_t *out) {
    sc28 x, y, r;
    for (int i = 0; i < 10; i++) {
        x.v[i] = a[i];
        y.v[i] = b[i];
        r.v[i] = 0;
    }
    bool ok = false;
    switch (op) {
    case SC_MONTMUL: sc28_montmul(r, x, y); ok = is_sc28_lazy(r); break;
    case SC_MONTSQ: sc28_montsq(r, x); ok = is_sc28_lazy(r); break;
    case SC_FROM_MONT: sc28_from_mont(r, x); ok = is_sc28_lazy(r); break;
    case SC_FROM_SC28: {
        sc s;
        sc_from_sc28(s, x);
        for (int i = 0; i < 8; i++) r.v[i] = s.v[i];
        ok = !sc_geq_l(s.v);
    } break;
    default: break;
    }
    for (int i = 0; i < 10; i++) out[i] = r.v[i];
    return ok;
}
// twenty 64-bit column sums -> lazy limbs
BP_HD bool sc_cols_raw(const uint64_t *c, uint32_t *out) {
    uint64_t t[20];
    for (int i = 0; i < 20; i++) t[i] = c[i];
    sc28 r;
    sc28_montreduce(r, t);
    for (int i = 0; i < 10; i++) out[i] = r.v[i];
    return is_sc28_lazy(r);
}

enum { GE_ADD_CACHED, GE_SUB_CACHED, GE_MADD, GE_MSUB, GE_DBL, GE_DBL_NO_T, GE_TO_CACHED, GE_FROM_NIELS, GE_FROM_NIELS_NEG, GE_NOPS };

// p: (X, Y, Z, T), q: cached (Y+X, Y-X, Z, 2dT) or Niels (y+x, y-x, -, 2dxy); out: (X, Y, Z, T) or cached -- 40 limbs each
BP_HD bool ge_raw(int op, const uint32_t *pa, const uint32_t *qa, uint32_t *out) {
    ge_ext p, r;
    ge_cached q;
    ld(p.X, pa); ld(p.Y, pa + 10); ld(p.Z, pa + 20); ld(p.T, pa + 30);
    ld(q.YpX, qa); ld(q.YmX, qa + 10); ld(q.Z, qa + 20); ld(q.T2d, qa + 30);
    ge_niels n;
    n.ypx = q.YpX; n.ymx = q.YmX; n.t2d = q.T2d;
    ge_identity(r);
    switch (op) {
    case GE_ADD_CACHED: ge_add_cached(r, p, q, false); break;
    case GE_SUB_CACHED: ge_add_cached(r, p, q, true); break;
    case GE_MADD: ge_madd(r, p, n, false); break;
    case GE_MSUB: ge_madd(r, p, n, true); break;
    case GE_DBL: ge_dbl(r, p, true); break;
    case GE_DBL_NO_T: fe_0(r.T); ge_dbl(r, p, false); break;
    case GE_TO_CACHED: {
        ge_cached c;
        ge_to_cached(c, p);
        r.X = c.YpX; r.Y = c.YmX; r.Z = c.Z; r.T = c.T2d;
    } break;
    case GE_FROM_NIELS: ge_from_niels(r, n, false); break;
    case GE_FROM_NIELS_NEG: ge_from_niels(r, n, true); break;
    default: break;
    }
    st(out, r.X); st(out + 10, r.Y); st(out + 20, r.Z); st(out + 30, r.T);
    return is_reduced(r.X) && is_reduced(r.Y) && is_reduced(r.Z) && is_reduced(r.T);
}

enum { HW_NORM, HW_SUB, HW_MUL, HW_SQN, HW_INVSQRT_RAW, HW_DBL, HW_ADD_CACHED, HW_TO_CACHED, HW_NOPS };

// one 64-lane wavefront: lane = 16 row + k holds limb k of row `row`'s field element (horner_wave.h's layout)
WV_FN wu32 hw_raw(const wv_ctx &cx, int op, const wu32 &a, const wu32 &b, int n) {
    const wu32 lane = wv_lane();
    const wu32 k = lane & 15u, row = lane >> 4;
    switch (op) {
    case HW_NORM: return hw_norm(a, k);
    case HW_SUB: return hw_sub(a, b, k);
    case HW_MUL: return hw_mul(cx, a, b, k);
    case HW_SQN: return hw_sqn(cx, a, n, k);
    case HW_INVSQRT_RAW: return hw_invsqrt_raw(cx, a, k);
    case HW_DBL: return hw_dbl(cx, a, row, k);
    case HW_ADD_CACHED: return hw_add_cached(cx, a, b, row, k);
    case HW_TO_CACHED: return hw_to_cached(cx, a, b, row, k);
    default: return a;
    }
}
// the bound of hw_norm's output, which every hw_* result passes through
#define LO_HW_SMALL (0x10000u + 38u * 0x400u)

}  // namespace lo
#endif
