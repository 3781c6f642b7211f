// Batches of Pedersen commitments and openings: PedersenGens::commit (src/generators.rs:38-42 of the reference),
//     V_i = v_i B + r_i B_blinding ,
// for many (v_i, r_i) at once, in ONE launch: lane = commitment.  A lane reads its value and its blinding (or draws the blinding:
// keystream block first_draw + i of ONE ChaChaRng seed for the batch -- one rng, one Scalar::random per commitment, the reference's own
// shape, tests/range_proof.rs:103-113), walks the window tables of the two bases that already sit in HBM (msm_fixed.h: no decoding,
// no doublings), compresses its point and stores the 32 bytes (commit) or compares them with a given commitment (open).
//
// The walk recodes in registers as fb_walk_thread does.  B_blinding takes all fb_nwin(W) windows.  A u64 value takes only the
// windows it can reach: the signed recoding adds half at every window it walks, so with nw windows the recoded value is
// v + half (2^(W nw) - 1) / (2^W - 1) < 2^64 + 2^(W nw) / 2 * (1 + 1 / (2^W - 1)), which stays below 2^(W nw) as soon as W nw >= 66
// (2^(W nw) (1 - 2^(W-1) / (2^W - 1)) >= 2^66 / 3 > 2^64 for W >= 2): ceil(66 / W) windows, 9 instead of 32 at W = 8.  The bias
// covers exactly the windows walked, so the digits sum to v again.
//
// Constant-time form (context option "prover_constant_time"): the W = 4 table of fb_accum_ct_thread; every (generator, window) pair
// reads all 8 entries, selects by masks and always adds; the number of B windows follows from the value's TYPE.  Same bytes.
#ifndef BPGPU_PEDERSEN_H
#define BPGPU_PEDERSEN_H
#include "msm_fixed.h"
#include "rp_prover.h"

namespace bp {

// where a batch's values and blindings come from
struct ped_in {
    const uint32_t *values;      // [row][value_words]
    uint32_t value_words;        // 2: u64 values, 8: 32-byte scalars
    const uint32_t *blindings;   // [row][8], or nullptr: drawn
    const uint8_t *seed32;       // the batch's seed when the blindings are drawn
    uint64_t first_draw;         // row i takes draw first_draw + i
};

// windows a u64 value reaches under the signed recoding (see above)
BP_HD uint32_t ped_u64_windows(fb_params prm) {
    const uint32_t nw = (66 + prm.W - 1) / prm.W;
    return nw < prm.nwin ? nw : prm.nwin;
}
BP_HD uint32_t ped_value_windows(fb_params prm, uint32_t value_words) { return value_words == 2 ? ped_u64_windows(prm) : prm.nwin; }

// A lane's parking space outside its registers (LDS in the kernel, locals on the host): the recoded scalar, word k at rw[k * rstride]
// (windows are cut from it by index -- the index is the same in every lane and depends on the window only -- instead of shifting a
// ten-register array through the walk), and the accumulated point between the walk and the two halves of the encoding.
struct ped_park {
    uint32_t *rw;
    uint32_t rstride;
    ge_ext *pt;
};

// rw = s + sum_{win < nw} half << (W win): the recoded scalar whose W-bit windows are digit + half
BP_HD void ped_bias_add(const ped_park &pk, const uint32_t s[8], uint32_t W, uint32_t nw) {
    uint32_t k[10];
#pragma unroll
    for (int i = 0; i < 10; i++) k[i] = 0;
    for (uint32_t win = 0; win < nw; win++) {   // public: depends on W and the value's type only
        const uint32_t bit = win * W + (W - 1), word = bit >> 5, m = 1u << (bit & 31);
#pragma unroll
        for (int i = 0; i < 10; i++) k[i] |= (word == (uint32_t)i) ? m : 0u;
    }
    uint32_t carry = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) {
        const uint64_t t = (uint64_t)(i < 8 ? s[i] : 0u) + k[i] + carry;
        pk.rw[i * pk.rstride] = (uint32_t)t;
        carry = (uint32_t)(t >> 32);
    }
}
// window `win` of the recoded scalar: bits [W win, W win + W); W (win + 1) <= 255 + W <= 275, so word index + 1 <= 9
BP_HD uint32_t ped_window(const ped_park &pk, uint32_t win, uint32_t W) {
    const uint32_t bit = win * W, idx = bit >> 5, sh = bit & 31;
    const uint64_t two = (uint64_t)pk.rw[idx * pk.rstride] | ((uint64_t)pk.rw[(idx < 9 ? idx + 1 : 9) * pk.rstride] << 32);
    return (uint32_t)(two >> sh) & ((1u << W) - 1u);
}

// one window of the variable-time walk: the first non-zero digit of a lane sets the accumulator (1 multiplication, not 7)
BP_HD void ped_step(ge_ext &acc, bool &started, const fb_line &line, uint32_t v, fb_params prm) {
    const int d = (int)v - (int)prm.half;
    if (d != 0) {
        ge_niels n;
#pragma unroll
        for (int i = 0; i < 10; i++) {
            n.ypx.v[i] = line.w[i];
            n.ymx.v[i] = line.w[10 + i];
            n.t2d.v[i] = line.w[20 + i];
        }
        if (!started) ge_from_niels(acc, n, d < 0);
        else ge_madd(acc, acc, n, d < 0);
        started = true;
    }
}
BP_HD const fb_entry *ped_entry(const fb_entry *base, uint32_t win, uint32_t v, fb_params prm) {
    const int d = (int)v - (int)prm.half;
    const uint32_t a = (uint32_t)(d < 0 ? -d : d);   // <= half: v is masked to W bits
    return base + (uint64_t)win * prm.half + (a ? a - 1 : 0);
}
// acc += s * P_gen over windows [0, nw) of generator row `gen`.  ONE line buffer: a window's line is requested when its turn comes and
// the other wavefronts of the SIMD cover the gather.  The second buffer of fb_walk_thread (the line of window w + 1 in flight while
// window w is added) does not fit here beside the first-digit branch: under the 168-register cap k_ped_commit<false> then parks 25
// registers in 104 B of scratch (tools/kernel_resources.py), and it measured 4 - 5 % slower at 64 and 4 096 rows, level at 262 144
// (profiles/pedersen_rate_line_buffers.json).  -DBP_PED_SECOND_LINE builds that form for comparison.
BP_HD void ped_walk(ge_ext &acc, bool &started, const ped_park &pk, const uint32_t s[8], uint32_t nw, uint32_t gen, fb_params prm, const fb_entry *table) {
    ped_bias_add(pk, s, prm.W, nw);
    const fb_entry *base = table + (uint64_t)gen * prm.nwin * prm.half;
    fb_line line;
#ifndef BP_PED_SECOND_LINE
    for (uint32_t win = 0; win < nw; win++) {
        const uint32_t v = ped_window(pk, win, prm.W);
        fb_load_line(line, ped_entry(base, win, v, prm));
        ped_step(acc, started, line, v, prm);
    }
#else
    uint32_t v = ped_window(pk, 0, prm.W);
    fb_load_line(line, ped_entry(base, 0, v, prm));
    for (uint32_t win = 0; win < nw; win++) {
        fb_line next = line;
        uint32_t vn = v;
        if (win + 1 < nw) {
            vn = ped_window(pk, win + 1, prm.W);
            fb_load_line(next, ped_entry(base, win + 1, vn, prm));
        }
        ped_step(acc, started, line, v, prm);
        line = next;
        v = vn;
    }
#endif
}
// the constant-time twin over the W = 4 table (prm.half == 8): fb_accum_ct_thread's window body
BP_HD void ped_walk_ct(ge_ext &acc, const ped_park &pk, const uint32_t s[8], uint32_t nw, uint32_t gen, fb_params prm, const fb_entry *table) {
    ped_bias_add(pk, s, BP_FB_CT_W, nw);
    for (uint32_t win = 0; win < nw; win++) {
        const uint32_t *sub = (const uint32_t *)(table + ((uint64_t)gen * prm.nwin + win) * 8);   // 8 entries of 32 words, same address in every lane
        const int d = (int)ped_window(pk, win, BP_FB_CT_W) - 8;
        const int sgn = d >> 31;                          // all ones for a negative digit
        const uint32_t a = (uint32_t)((d ^ sgn) - sgn);   // |d| in 0..8
        uint32_t sel[30];
#pragma unroll
        for (int i = 0; i < 30; i++) sel[i] = 0;
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            const uint32_t m = 0u - (uint32_t)(a == k + 1);
#pragma unroll
            for (int i = 0; i < 30; i++) sel[i] |= sub[32 * k + i] & m;
        }
        const uint32_t m0 = 0u - (uint32_t)(a == 0);      // digit 0: the neutral element (1, 1, 0)
        sel[0] |= 1u & m0;
        sel[10] |= 1u & m0;
        ge_niels n;
#pragma unroll
        for (int i = 0; i < 10; i++) {
            n.ypx.v[i] = sel[i];
            n.ymx.v[i] = sel[10 + i];
            n.t2d.v[i] = sel[20 + i];
        }
        ge_madd(acc, acc, n, sgn != 0);
    }
}

// row i's blinding: given, or draw first_draw + i of the batch's seed (reduced by construction); stored to blindings_out where asked for
BP_HD void ped_load_blinding(uint32_t i, const ped_in &in, uint32_t r[8], uint32_t *blindings_out) {
    if (in.blindings) {
#pragma unroll
        for (int q = 0; q < 8; q++) r[q] = in.blindings[8 * (uint64_t)i + q];
    } else {
        sc x;
        rpp_draw(x, in.seed32, in.first_draw + i);
#pragma unroll
        for (int q = 0; q < 8; q++) r[q] = x.v[q];
    }
    if (blindings_out) {
#pragma unroll
        for (int q = 0; q < 8; q++) blindings_out[8 * (uint64_t)i + q] = r[q];
    }
}
// row i's value: a u64, zero-extended, or 8 words
BP_HD void ped_load_value(uint32_t i, const ped_in &in, uint32_t v[8]) {
#pragma unroll
    for (int q = 0; q < 8; q++) v[q] = 0;
    if (in.value_words == 2) {
        v[0] = in.values[2 * (uint64_t)i];
        v[1] = in.values[2 * (uint64_t)i + 1];
    } else {
#pragma unroll
        for (int q = 0; q < 8; q++) v[q] = in.values[8 * (uint64_t)i + q];
    }
}

// The point of row i: term 0 is r_i on B_blinding, term 1 is v_i on B -- one loop body for both, each scalar read when its walk begins
// (the value does not occupy registers through the blinding's walk).  gen_ids: the shared path's id list, [0] = B_blinding, [1] = B.
// CT: table and prm are the W = 4 set.  pk: the lane's parking space.  Returns whether both scalars are canonical; a rejected row
// walks too (the masked digits stay inside the tables), so nothing branches on a secret.
template <bool CT>
BP_HD bool ped_point(ge_ext &acc, uint32_t i, const ped_in &in, const ped_park &pk, fb_params prm, const uint32_t *gen_ids, const fb_entry *table,
                     uint32_t *blindings_out) {
    ge_identity(acc);
    bool ok = true, started = false;
#pragma unroll 1
    for (uint32_t term = 0; term < 2; term++) {
        uint32_t s[8];
        if (term == 0) ped_load_blinding(i, in, s, blindings_out);
        else ped_load_value(i, in, s);
        ok = ok & sc_is_canonical(s);
        const uint32_t nw = term == 0 ? prm.nwin : ped_value_windows(prm, in.value_words);
        if (CT) ped_walk_ct(acc, pk, s, nw, gen_ids[term], prm, table);
        else ped_walk(acc, started, pk, s, nw, gen_ids[term], prm, table);
    }
    return ok;
}

// The finish in the same lane.  The point is parked and its coordinates are read again where they are used: only t = u1 u2^2 crosses
// the inversion's squaring chain (ristretto_compress_front / fe_invsqrt_i, as ristretto_compress_lp), and the back half below never
// holds more than two coordinates beside its own intermediates -- ristretto_compress's steps in an order that lets values die early.
// That keeps the lane within the walk's register budget; the bytes are ristretto_compress's (the CPU harness compares).
BP_HD void ped_reload(fe &r, const fe *src) {   // a fresh read each time: nothing is kept in registers between uses
    const volatile uint32_t *q = (const volatile uint32_t *)src->v;
#pragma unroll
    for (int i = 0; i < 10; i++) r.v[i] = q[i];
}
BP_HD void ped_encode(uint32_t w[8], const ge_ext &acc, const ped_park &pk) {
    const fe sqrt_m1 = BP_FE_SQRT_M1, invsqrt_a_minus_d = BP_FE_INVSQRT_A_MINUS_D;
    *pk.pt = acc;
    const ge_ext *p = pk.pt;
    fe I, i1, i2, zinv, den, t;
    {   // I = 1 / sqrt(u1 u2^2): fe_invsqrt_i with its input parked in the scalar's words (the walk is over) instead of carried through the chain
        fe tin, v3, v7, raw;
        ristretto_compress_front(tin, p);
#pragma unroll
        for (int q = 0; q < 10; q++) pk.rw[q * pk.rstride] = tin.v[q];
        fe_sq(v3, tin);
        fe_mul(v3, v3, tin);
        fe_sq(v7, v3);
        fe_mul(v7, v7, tin);
        fe_pow22523(raw, v7);
        {
            const volatile uint32_t *q0 = pk.rw;
#pragma unroll
            for (int q = 0; q < 10; q++) tin.v[q] = q0[q * pk.rstride];
        }
        fe_sq(v3, tin);
        fe_mul(v3, v3, tin);
        fe_mul(raw, raw, v3);
        fe_invsqrt_fix(I, raw, tin);
    }
    {   // i1 = I u1, i2 = I u2
        fe X, Y, Z, a, b, u;
        ped_reload(Y, &p->Y);
        ped_reload(Z, &p->Z);
        fe_add(a, Z, Y);
        fe_sub(b, Z, Y);
        fe_mul(u, a, b);
        fe_mul(i1, I, u);
        ped_reload(X, &p->X);
        fe_mul(u, X, Y);
        fe_mul(i2, I, u);
    }
    bool rotate;
    {
        fe T;
        ped_reload(T, &p->T);
        fe_mul(zinv, i1, i2);
        fe_mul(zinv, zinv, T);
        fe_mul(t, T, zinv);
        rotate = fe_isneg(t);
    }
    {
        fe dr;
        fe_mul(dr, i1, invsqrt_a_minus_d);
        fe_select(den, i2, dr, rotate);
    }
    bool neg;
    {   // the sign of x z_inv after the rotation
        fe X, Y, xr;
        ped_reload(X, &p->X);
        ped_reload(Y, &p->Y);
        fe_mul(xr, Y, sqrt_m1);
        fe_select(X, X, xr, rotate);
        fe_mul(t, X, zinv);
        neg = fe_isneg(t);
    }
    {
        fe X, Y, Z, yr;
        ped_reload(X, &p->X);
        ped_reload(Y, &p->Y);
        fe_mul(yr, X, sqrt_m1);
        fe_select(Y, Y, yr, rotate);
        fe_cneg(Y, neg);
        ped_reload(Z, &p->Z);
        fe_sub(t, Z, Y);
        fe_mul(t, t, den);
        fe_abs(t);
        fe_to_words(w, t);
    }
}

// lane = commitment: 8 words out (zeros for a rejected row) and the row's BPGPU_MSM_* status byte
template <bool CT>
BP_HD void ped_commit_lane(uint32_t i, ped_in in, ped_park pk, fb_params prm, const uint32_t *gen_ids, const fb_entry *table, uint32_t *out_words,
                           uint32_t *blindings_out, uint8_t *status) {
    ge_ext acc;
    const bool ok = ped_point<CT>(acc, i, in, pk, prm, gen_ids, table, blindings_out);
    uint32_t w[8];
    ped_encode(w, acc, pk);
#pragma unroll
    for (int q = 0; q < 8; q++) out_words[8 * (uint64_t)i + q] = ok ? w[q] : 0u;
    status[i] = ok ? (uint8_t)BP_STATUS_OK : (uint8_t)BP_STATUS_BAD_SCALAR;
}

// lane = opening: verdict 0 = (v, r) opens the commitment, 1 = it does not (an encoding that does not decode equals no output of
// compress, which is canonical), 2 = a scalar is not canonical.  Variable time: its inputs are public to the verifier.
BP_HD void ped_open_lane(uint32_t i, ped_in in, ped_park pk, const uint32_t *commitments, fb_params prm, const uint32_t *gen_ids, const fb_entry *table,
                         uint8_t *verdict) {
    ge_ext acc;
    const bool ok = ped_point<false>(acc, i, in, pk, prm, gen_ids, table, nullptr);
    uint32_t w[8];
    ped_encode(w, acc, pk);
    uint32_t diff = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) diff |= w[q] ^ commitments[8 * (uint64_t)i + q];
    verdict[i] = !ok ? 2 : (diff ? 1 : 0);
}

}  // namespace bp
#endif
