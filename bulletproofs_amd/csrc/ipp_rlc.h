// Batch combination of stand-alone InnerProductProof verifications (bpgpu_ipp_verify_rlc, include/bpgpu.h): the RLC of linear_rlc.h
// applied to ipp.h's final check, for bases shared by the batch.
//
//   R = sum_p rho_p * Check_p ,   Check_p = (a_p b_p) Q_p + sum_i (a_p s_{p,i} g_{p,i}) G_i + sum_i (b_p s_{p,i}^-1 h_{p,i}) H_i
//                                           - sum_j u_{p,j}^2 L_{p,j} - sum_j u_{p,j}^-2 R_{p,j} - P_p          (inner_product_proof.rs:308-325)
//     = sum_i (sum_p rho_p a_p s_{p,i} g_{p,i}) G_i + sum_i (sum_p rho_p b_p s_{p,i}^-1 h_{p,i}) H_i  +  sum_p sum_u (rho_p t_{p,u}) X_{p,u}
//
// G_0..G_{n-1}, H_0..H_{n-1} are shared by the whole batch (the caller's points or the context's generators), so their 2n coefficients
// add up in the scalar field; only the U = 2k + 2 points Q, L_j, R_j, P of every proof stay proof-specific.  Nothing here is as large as
// nbatch x n: k_ipp_vs_front (ipp_vs_front_thread, unchanged) leaves per proof its status, u_j^2, u_j^-2 and the Montgomery table
// (u_j, u_j^-1); then
//   rlc_rho_thread        : lane = proof          its weight rho_p
//   ipp_rlc_uniq_thread   : lane = proof          the U unique terms times rho_p into the combined list (scalar 0 and the identity
//                                                 encoding for a proof that stopped in the front end); parks rho a, rho b
//   ipp_rlc_weigh_begin / _step : lane = (block of B rows, proof), proof fastest   rho_p a_p s_{p,i} g_{p,i} (row i) or
//                                                 rho_p b_p s_{p,i}^-1 h_{p,i} (row n + i) for rlc.h's limb sums; s from the proof's table, in
//                                                 closed form for the block's first row and then along a Gray-code walk
//   rlc_reduce_thread     : lane = row            the accumulated coefficient mod l -- into the generator-table row, or with the base's
//                                                 encoding into the head of the combined list (explicit bases: ipp_rlc_reduce_thread)
// ONE multiscalar multiplication, and rlc_verdict_thread (lane = proof).
#ifndef BPGPU_IPP_RLC_H
#define BPGPU_IPP_RLC_H
#include "ipp.h"
#include "rlc_comb.h"

namespace bp {

#define IPP_RLC_WEIGHT_DOMAIN 0x69706377u   // "wcpi": the combination weights the caller did not bring
#define IPP_RLC_MAX_PROOFS (1u << 24)       // rlc_acc_to_sc's 2^24 sums per row
#define IPP_RLC_MAX_TERMS (1u << 24)        // proof-specific terms of the one MSM: 1 GiB of list

// Rows a weigh lane walks: IPP_RLC_BLOCK (n when n is smaller) from IPP_RLC_BLOCK_MIN_PAIRS (row, proof) pairs on, else 1.  A walk costs
// 4 products per row instead of k + 2 but leaves an eighth of the lanes: measured on one MI355X it is 3 ... 16 % of the call ahead from
// 2^21 pairs on and 1 ... 6 % behind up to 2^19
#define IPP_RLC_BLOCK 8u
#define IPP_RLC_BLOCK_MIN_PAIRS (1u << 20)

// nstride: nproofs rounded up to 64 (the lanes of the padding add nothing), so that the 64 lanes of a wavefront share their rows.
// B: rows per weigh lane, a power of two that divides n.
// row0: the combined row of G_0 (2 in generator-table mode, behind B_blinding and B; 0 with explicit bases).  u0: first slot of the
// unique terms in the combined list (2n with explicit bases: the bases come first; 0 in generator-table mode)
struct ipp_rlc_shape {
    uint32_t nproofs, nstride, n, k, U, proof_len, row0, u0, B;
};

// the shared key and rho body under this check's names and domain (the host harness drives them so)
using ipp_rlc_key = rlc_key;
BP_HD void ipp_rlc_rho_thread(uint32_t p, const uint8_t *weights64, const ipp_rlc_key &key, uint32_t *rho) {
    rlc_rho_thread(p, weights64, key, IPP_RLC_WEIGHT_DOMAIN, rho);
}

// r = x * ym with x a plain value (any 256-bit words) and ym in Montgomery form: the plain product, canonical
BP_HD void ipp_rlc_mul_plain(sc &r, const uint32_t x[8], const sc28 &ym) {
    sc28 t;
    sc28_from_words(t, x);
    sc28_montmul(t, t, ym);
    sc_from_sc28(r, t);
}

// lane = proof p: slots p U .. p U + U - 1 of the combined list behind u0 -- rho a b on Q_p, -rho u_j^2 on L_j, -rho u_j^-2 on R_j,
// -rho on P_p -- and rho a, rho b in Montgomery form to ab[p][2][10] for the weigh lanes.  A proof with a non-zero status gets
// scalar 0 and the all-zero encoding in every slot, and nothing of its staging is read.
BP_HD void ipp_rlc_uniq_thread(uint32_t p, const ipp_rlc_shape &sh, const uint32_t *status, const uint32_t *rho, const uint8_t *proofs,
                               const uint8_t *P, const uint8_t *Q, const uint32_t *u_sq, const uint32_t *u_inv_sq, uint32_t *ab,
                               uint32_t *comb_sc, uint32_t *comb_pt) {
    const uint32_t k = sh.k;
    const uint64_t slot0 = (uint64_t)sh.u0 + (uint64_t)p * sh.U;
    uint32_t *dsc = comb_sc + slot0 * 8, *dpt = comb_pt + slot0 * 8;
    if (status[p] != 0) {
        for (uint32_t t = 0; t < sh.U * 8; t++) dsc[t] = 0u, dpt[t] = 0u;
        return;
    }
    const uint8_t *pr = proofs + (uint64_t)p * sh.proof_len;
    sc r, x;
    sc28 rm, am, bm;
#pragma unroll
    for (int q = 0; q < 8; q++) r.v[q] = rho[8 * (uint64_t)p + q];
    sc_to_mont28(rm, r);
    uint32_t w[8];
    load_words8(w, pr + 64 * k);
    sc28_from_words(am, w);
    sc28_montmul(am, am, rm);                       // a rho (plain)
    sc28_to_mont(am, am);
    load_words8(w, pr + 64 * k + 32);
    ipp_rlc_mul_plain(x, w, am);                    // rho a b on Q
    store_words8(dsc, x);
    sc28_from_words(bm, w);
    sc28_montmul(bm, bm, rm);                       // b rho (plain)
    sc28_to_mont(bm, bm);
    uint32_t *abp = ab + (uint64_t)p * 20;
#pragma unroll
    for (int q = 0; q < 10; q++) abp[q] = am.v[q], abp[10 + q] = bm.v[q];
    load_words8(w, Q + (uint64_t)p * 32);
#pragma unroll
    for (int q = 0; q < 8; q++) dpt[q] = w[q];
    for (uint32_t j = 0; j < k; j++) {
        const uint32_t *us = u_sq + ((uint64_t)p * k + j) * 8, *ui = u_inv_sq + ((uint64_t)p * k + j) * 8;
#pragma unroll
        for (int q = 0; q < 8; q++) w[q] = us[q];
        ipp_rlc_mul_plain(x, w, rm);
        sc_neg(x, x);                               // -rho u_j^2 on L_j
        store_words8(dsc + (1 + j) * 8, x);
#pragma unroll
        for (int q = 0; q < 8; q++) w[q] = ui[q];
        ipp_rlc_mul_plain(x, w, rm);
        sc_neg(x, x);                               // -rho u_j^-2 on R_j
        store_words8(dsc + (1 + k + j) * 8, x);
        load_words8(w, pr + 64 * j);
#pragma unroll
        for (int q = 0; q < 8; q++) dpt[(1 + j) * 8 + q] = w[q];
        load_words8(w, pr + 64 * j + 32);
#pragma unroll
        for (int q = 0; q < 8; q++) dpt[(1 + k + j) * 8 + q] = w[q];
    }
    sc_neg(x, r);                                   // -rho on P
    store_words8(dsc + (1 + 2 * k) * 8, x);
    load_words8(w, P + (uint64_t)p * 32);
#pragma unroll
    for (int q = 0; q < 8; q++) dpt[(1 + 2 * k) * 8 + q] = w[q];
}

// One weigh lane: proof p and the B consecutive rows from r0 (all of G or all of H: B divides n), walked in Gray-code order.
// s: s_i (for H its inverse) of the row the lane stands on, ra: rho a (for H rho b), both in Montgomery form
struct ipp_rlc_lane {
    sc28 s, ra;
    const uint32_t *tb;   // the proof's table (u_j, u_j^-1)
    const uint8_t *f;     // the proof's factors of these rows: g_{p,i0..} or h_{p,i0..}
    uint32_t r0;
    bool h, active;       // active: the proof exists and reached the check
};

// lane tid = block * nstride + proof over the 2n / B blocks of rows (G_0.., H_0..).  s_{i0} of the block's first row in closed form
// as in ipp_vs_s_thread: for bit b of i, u or u^-1 at index k-1-b, swapped for H.
BP_HD void ipp_rlc_weigh_begin(uint32_t tid, const ipp_rlc_shape &sh, const uint32_t *status, const uint32_t *ab, const uint32_t *tab, const uint8_t *Gf,
                               const uint8_t *Hf, ipp_rlc_lane &ln) {
    const uint32_t blk = tid / sh.nstride, p = tid - blk * sh.nstride, n = sh.n, k = sh.k;
    ln.r0 = blk * sh.B;
    ln.h = ln.r0 >= n;
    ln.active = p < sh.nproofs && status[p] == 0;
    if (!ln.active) return;
    const uint32_t i0 = ln.h ? ln.r0 - n : ln.r0;
    ln.f = (ln.h ? Hf : Gf) + ((uint64_t)p * n + i0) * 32;
    ln.tb = tab + (uint64_t)p * 2 * k * 10;
    const uint32_t *f = ab + (uint64_t)p * 20 + (ln.h ? 10 : 0);
#pragma unroll
    for (int q = 0; q < 10; q++) ln.ra.v[q] = f[q];
    sc28_one_mont(ln.s);
    for (uint32_t bb = 0; bb < k; bb++) {
        f = ln.tb + (2 * (k - 1 - bb) + ((((i0 >> bb) & 1) != 0) == ln.h ? 1 : 0)) * 10;
        sc28 fm;
#pragma unroll
        for (int q = 0; q < 10; q++) fm.v[q] = f[q];
        sc28_montmul(ln.s, ln.s, fm);
    }
}

// step g of B: the lane moves to row r0 + gray(g) -- one bit b of the index flips, so s picks up the square of the table's entry
// for the bit's new value (u_j^2 or u_j^-2, j = k-1-b: two products instead of k; B = 1 never gets here) -- and returns true with the weighted coefficient
// `v` = rho a s_i g_{p,i} (H: rho b s_i^-1 h_{p,i}) for the caller's accumulation (false for a proof that stopped and for the
// padding).  `row` is set in every lane: it is the wavefront's row.  The plain factor times Montgomery forms stays a plain value.
BP_HD bool ipp_rlc_weigh_step(uint32_t g, const ipp_rlc_shape &sh, ipp_rlc_lane &ln, sc &v, uint32_t &row) {
    const uint32_t gi = g ^ (g >> 1);
    row = sh.row0 + ln.r0 + gi;
    sc_0(v);
    if (!ln.active) return false;
    sc28 fm;
    if (g) {
        const uint32_t bb = (uint32_t)__builtin_ctz(g);
        const uint32_t *f = ln.tb + (2 * (sh.k - 1 - bb) + ((((gi >> bb) & 1) != 0) == ln.h ? 1 : 0)) * 10;
#pragma unroll
        for (int q = 0; q < 10; q++) fm.v[q] = f[q];
        sc28_montmul(ln.s, ln.s, fm);
        sc28_montmul(ln.s, ln.s, fm);
    }
    uint32_t w[8];
    load_words8(w, ln.f + (uint64_t)gi * 32);
    sc28 x;
    sc28_from_words(x, w);
    sc28_montmul(x, x, ln.ra);
    sc28_montmul(x, x, ln.s);
    sc_from_sc28(v, x);
    return true;
}

// explicit bases, lane = row of (G_0.., H_0..): rlc_reduce_thread, and the base's encoding beside it, taken once from the caller's
// G, H (out_sc, out_pt are the head of the combined list)
BP_HD void ipp_rlc_reduce_thread(uint32_t row, uint32_t n, const uint64_t *acc, const uint8_t *G, const uint8_t *H, uint32_t *out_sc,
                                 uint32_t *out_pt) {
    rlc_reduce_thread(row, acc, out_sc);
    uint32_t w[8];
    load_words8(w, row < n ? G + 32 * (uint64_t)row : H + 32 * (uint64_t)(row - n));
#pragma unroll
    for (int q = 0; q < 8; q++) out_pt[(uint64_t)row * 8 + q] = w[q];
}

}  // namespace bp
#endif
