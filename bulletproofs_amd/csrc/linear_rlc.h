// Batch combination of LinearProof verifications (bpgpu_linear_verify_rlc, include/bpgpu.h): the RLC of rlc.h / r1cs_rlc.h applied to
// linear.h's final check.
//
//   R = sum_p rho_p * Check_p ,   Check_p = r_p B + (a_p b0_p) F + sum_i (a_p s_{p,i}) G_i - x*_p C_p - sum_j (x*_p x_{p,j}) L_{p,j}
//                                           - sum_j (x*_p / x_{p,j}) R_{p,j} - S_p                      (linear_proof.rs:214-236)
//     = (sum_p rho_p r_p) B + (sum_p rho_p a_p b0_p) F + sum_i (sum_p rho_p a_p s_{p,i}) G_i  +  sum_p sum_u (rho_p t_{p,u}) Q_{p,u}
//
// B, F and G_0..G_{n-1} are shared by the whole batch (the caller's points or the context's generators), so their n + 2 coefficients
// add up in the scalar field; only the U = 2k + 2 points C, L_j, R_j, S of every proof stay proof-specific.  k_lin_prepare fills the
// per-proof staging exactly as for the per-proof path; then
//   lin_rlc_rho_thread    : lane = proof           its weight rho_p
//   lin_rlc_weigh_thread  : lane = (term, proof), proof fastest   the U unique terms times rho_p into the combined list (scalar 0 and the
//                                                   identity encoding for a proof that stopped in the front end), and the n + 2 base
//                                                   coefficients times rho_p for the accumulators (rlc.h's limb sums), rows (B, F, G_0..)
//   lin_rlc_reduce_thread : lane = row             the accumulated coefficient mod l -- into the generator-table row, or with the base's
//                                                   encoding into the head of the combined list (explicit bases)
// ONE multiscalar multiplication, and lin_rlc_verdict_thread (lane = proof).
#ifndef BPGPU_LINEAR_RLC_H
#define BPGPU_LINEAR_RLC_H
#include "linear.h"
#include "rlc.h"
#include "chacha20.h"

namespace bp {

#define LIN_RLC_WEIGHT_DOMAIN 0x6e6c6377u   // "wcln": the combination weights the caller did not bring
#define LIN_RLC_MAX_PROOFS (1u << 24)       // rlc_acc_to_sc's 2^24 sums per row
#define LIN_RLC_MAX_TERMS (1u << 24)        // proof-specific terms of the one MSM: 1 GiB of list

// nstride: nproofs rounded up to 64 (the lanes of the padding add nothing), so that the 64 lanes of a wavefront share their term.
// fixed != 0: generator-table staging (the base coefficients in the proof's row of gen_sc, lists of U terms C, L.., R.., S); else the
// explicit-bases lists of n + 2k + 4 terms B, F, C, L.., R.., G.., S.  u0: first slot of the unique terms in the combined list
// (n + 2 with explicit bases: the bases come first; 0 in generator-table mode)
struct lin_rlc_shape {
    uint32_t nproofs, nstride, n, k, U, fixed, u0;
};
struct lin_rlc_key {
    uint32_t w[8];
};

// rho of proof p: from_bytes_mod_order_wide(weights64[p]), or of block p of ChaCha20(key, nonce = LIN_RLC_WEIGHT_DOMAIN)
BP_HD void lin_rlc_rho_thread(uint32_t p, const uint8_t *weights64, const lin_rlc_key &key, uint32_t *rho) {
    uint32_t w16[16];
    if (weights64) {
        const uint8_t *src = weights64 + 64 * (uint64_t)p;
        for (int i = 0; i < 16; i++)
            w16[i] = (uint32_t)src[4 * i] | ((uint32_t)src[4 * i + 1] << 8) | ((uint32_t)src[4 * i + 2] << 16) | ((uint32_t)src[4 * i + 3] << 24);
    } else {
        chacha20_block(key.w, (uint64_t)p, LIN_RLC_WEIGHT_DOMAIN, 0u, w16);
    }
    sc r;
    sc_from_wide(r, w16);
    store_words8(rho + 8 * (uint64_t)p, r);
}

// lane tid = term * nstride + proof over U + n + 2 terms.  Unique terms go to the combined list; a shared-base term sets its combined
// row `row` (also in the padding lanes: it is the wavefront's row) and returns true with its weighted coefficient `v` for the caller's
// accumulation (false for a proof that stopped and for the padding).
BP_HD bool lin_rlc_weigh_thread(uint32_t tid, const lin_rlc_shape &sh, const uint32_t *status, const uint32_t *rho, const uint32_t *gen_sc,
                                const uint32_t *list_sc, const uint32_t *list_pt, uint32_t *comb_sc, uint32_t *comb_pt, sc &v, uint32_t &row) {
    const uint32_t t = tid / sh.nstride, p = tid - t * sh.nstride;
    sc_0(v);
    row = t < sh.U ? 0u : t - sh.U;
    if (p >= sh.nproofs) return false;
    const uint32_t st = status[p];
    const uint32_t N = sh.fixed ? sh.U : sh.n + 2 * sh.k + 4;   // terms per proof in the staging lists
    sc x, r;
#pragma unroll
    for (int q = 0; q < 8; q++) r.v[q] = rho[8 * (uint64_t)p + q];
    if (t < sh.U) {
        // C, L_0.., R_0.. are consecutive in both layouts (from 0, or from 2 behind B and F); S closes the list
        const uint32_t idx = sh.fixed ? t : (t + 1 < sh.U ? 2 + t : N - 1);
        const uint64_t src = ((uint64_t)p * N + idx) * 8, dst = ((uint64_t)sh.u0 + (uint64_t)p * sh.U + t) * 8;
        if (st != 0) {
            sc_0(x);
#pragma unroll
            for (int q = 0; q < 8; q++) comb_pt[dst + q] = 0u;
        } else {
#pragma unroll
            for (int q = 0; q < 8; q++) {
                x.v[q] = list_sc[src + q];
                comb_pt[dst + q] = list_pt[src + q];
            }
            sc_mul(x, x, r);
        }
        store_words8(comb_sc + dst, x);
        return false;
    }
    if (st != 0) return false;
    const uint32_t g = row;   // 0: B, 1: F, 2 + i: G_i
    const uint32_t *src = sh.fixed ? gen_sc + ((uint64_t)p * (sh.n + 2) + g) * 8
                                   : list_sc + ((uint64_t)p * N + (g < 2 ? g : 1 + 2 * sh.k + g)) * 8;   // G_i is term 3 + 2k + i
#pragma unroll
    for (int q = 0; q < 8; q++) x.v[q] = src[q];
    sc_mul(v, x, r);
    return true;
}

// lane = row of (B, F, G_0..): the accumulated coefficient mod l to out_sc[row]; with explicit bases (out_pt != NULL) also the base's
// encoding, taken once from the caller's B, F, G, to out_pt[row] -- the head of the combined list
BP_HD void lin_rlc_reduce_thread(uint32_t row, const uint64_t *acc, const uint8_t *B, const uint8_t *F, const uint8_t *G, uint32_t *out_sc,
                                 uint32_t *out_pt) {
    uint64_t a[10];
#pragma unroll
    for (int i = 0; i < 10; i++) a[i] = acc[(uint64_t)row * 10 + i];
    sc s;
    rlc_acc_to_sc(s, a);
    store_words8(out_sc + (uint64_t)row * 8, s);
    if (out_pt) {
        uint32_t w[8];
        load_words8(w, row == 0 ? B : (row == 1 ? F : G + 32 * (uint64_t)(row - 2)));
#pragma unroll
        for (int q = 0; q < 8; q++) out_pt[(uint64_t)row * 8 + q] = w[q];
    }
}

// verdict of proof p: its front-end code, else 0 when R (enc = compress(R), msm_status[0] != 0: a point did not decode) is the identity
// and every point decoded, else undecided (the host then re-verifies proof by proof); lane 0 also writes the 33 batch bytes
BP_HD void lin_rlc_verdict_thread(uint32_t p, const uint32_t *status, const uint32_t *enc, const uint8_t *msm_status, uint8_t *verdict,
                                  uint8_t *batch_out) {
    uint32_t nz = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) nz |= enc[i];
    const bool decoded = msm_status[0] == 0, pass = decoded && nz == 0;
    verdict[p] = status[p] ? (uint8_t)status[p] : (pass ? (uint8_t)BP_VERDICT_OK : (uint8_t)BP_VERDICT_UNDECIDED);
    if (p == 0) {
        batch_out[0] = pass ? 0 : 1;
        for (int i = 0; i < 32; i++) batch_out[1 + i] = decoded ? (uint8_t)(enc[i >> 2] >> (8 * (i & 3))) : 0;
    }
}

}  // namespace bp
#endif
