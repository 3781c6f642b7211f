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
//   rlc_rho_thread        : lane = proof           its weight rho_p
//   lin_rlc_weigh_thread  : lane = (term, proof), proof fastest   the U unique terms times rho_p into the combined list (scalar 0 and the
//                                                   identity encoding for a proof that stopped in the front end), and the n + 2 base
//                                                   coefficients times rho_p for the accumulators (rlc.h's limb sums), rows (B, F, G_0..)
//   rlc_reduce_thread     : lane = row             the accumulated coefficient mod l -- into the generator-table row, or with the base's
//                                                   encoding into the head of the combined list (explicit bases: lin_rlc_reduce_thread)
// ONE multiscalar multiplication, and rlc_verdict_thread (lane = proof).
#ifndef BPGPU_LINEAR_RLC_H
#define BPGPU_LINEAR_RLC_H
#include "linear.h"
#include "rlc_comb.h"

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

// the shared key and rho body under this check's names and domain (the host harness drives them so)
using lin_rlc_key = rlc_key;
BP_HD void lin_rlc_rho_thread(uint32_t p, const uint8_t *weights64, const lin_rlc_key &key, uint32_t *rho) {
    rlc_rho_thread(p, weights64, key, LIN_RLC_WEIGHT_DOMAIN, rho);
}

// rlc_weigh_thread's index maps; either way base term g (0: B, 1: F, 2 + i: G_i) lands on row g.
// Generator-table staging: lists of U terms C, L.., R.., S; the n + 2 base coefficients in the proof's row of gen_sc
struct lin_rlc_table_map {
    uint32_t n, U;
    const uint32_t *gen_sc;
    BP_HD uint64_t uniq(uint32_t p, uint32_t t) const { return (uint64_t)p * U + t; }
    BP_HD const uint32_t *shared(uint32_t p, uint32_t g) const { return gen_sc + ((uint64_t)p * (n + 2) + g) * 8; }
    BP_HD uint32_t row(uint32_t g) const { return g; }
};
// Explicit bases: lists of N = n + 2k + 4 terms B, F, C, L.., R.., G.., S -- C, L_0.., R_0.. are consecutive from 2, S closes the
// list, G_i is term 3 + 2k + i
struct lin_rlc_bases_map {
    uint32_t k, U, N;
    const uint32_t *list_sc;
    BP_HD uint64_t uniq(uint32_t p, uint32_t t) const { return (uint64_t)p * N + (t + 1 < U ? 2 + t : N - 1); }
    BP_HD const uint32_t *shared(uint32_t p, uint32_t g) const { return list_sc + ((uint64_t)p * N + (g < 2 ? g : 1 + 2 * k + g)) * 8; }
    BP_HD uint32_t row(uint32_t g) const { return g; }
};

// lane tid = term * nstride + proof over U + n + 2 terms (rlc_weigh_thread) in the staging's layout
BP_HD bool lin_rlc_weigh_thread(uint32_t tid, const lin_rlc_shape &sh, const uint32_t *status, const uint32_t *rho, const uint32_t *gen_sc,
                                const uint32_t *list_sc, const uint32_t *list_pt, uint32_t *comb_sc, uint32_t *comb_pt, sc &v, uint32_t &row) {
    comb_sc += 8 * (uint64_t)sh.u0, comb_pt += 8 * (uint64_t)sh.u0;
    if (sh.fixed)
        return rlc_weigh_thread(tid, sh.nproofs, sh.nstride, sh.U, lin_rlc_table_map{sh.n, sh.U, gen_sc}, status, rho, list_sc, list_pt, comb_sc, comb_pt, v, row);
    return rlc_weigh_thread(tid, sh.nproofs, sh.nstride, sh.U, lin_rlc_bases_map{sh.k, sh.U, sh.n + 2 * sh.k + 4, list_sc}, status, rho, list_sc, list_pt,
                            comb_sc, comb_pt, v, row);
}

// lane = row of (B, F, G_0..): rlc_reduce_thread, and with explicit bases (out_pt != NULL: out_sc, out_pt are the head of the combined
// list) the base's encoding beside it, taken once from the caller's B, F, G
BP_HD void lin_rlc_reduce_thread(uint32_t row, const uint64_t *acc, const uint8_t *B, const uint8_t *F, const uint8_t *G, uint32_t *out_sc,
                                 uint32_t *out_pt) {
    rlc_reduce_thread(row, acc, out_sc);
    if (!out_pt) return;
    uint32_t w[8];
    load_words8(w, row == 0 ? B : (row == 1 ? F : G + 32 * (uint64_t)(row - 2)));
#pragma unroll
    for (int q = 0; q < 8; q++) out_pt[(uint64_t)row * 8 + q] = w[q];
}

}  // namespace bp
#endif
