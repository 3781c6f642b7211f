// Batch combination of R1CS proof verifications (bpgpu_r1cs_verify_rlc, include/bpgpu.h): the range-proof RLC of rlc.h applied to
// r1cs.h's mega-check, across one or many circuits.
//
//   R = sum_i rho_i * MegaCheck_i ,   MegaCheck_i = r1cs/verifier.rs:459-491 for proof i
//     = sum_g (sum_i rho_i s_{i,g}) P_g  +  sum_i sum_u (rho_i t_{i,u}) Q_{i,u}
//
// Proofs of different circuits share the generator rows once they are laid out on the batch's PN = max padded_n: B_blinding, B and
// G_i keep their row, H_i moves from 2 + pn + i to 2 + PN + i.  The k_r1cs_front / flatten / finish launches of one group (slice) fill
// the per-proof staging exactly as for the per-proof path; then, per slice:
//   r1_rlc_weigh_thread : lane = (term, proof), proof fastest   the U = 11 + m + 2k unique terms times rho_p into the combined list
//                                        (scalar 0 and the identity encoding for a proof that stopped before its MSM), and the
//                                        2 pn + 2 generator coefficients times rho_p for the accumulators (rlc.h's limb sums)
// and once per combination: the reduction of the accumulators (rlc_reduce_thread), ONE shared-generator MSM over PN, the sum of the
// combinations' points (r1_rlc_sum_thread) and the verdicts (rlc_verdict_thread).
#ifndef BPGPU_R1CS_RLC_H
#define BPGPU_R1CS_RLC_H
#include "r1cs.h"
#include "rlc_comb.h"

namespace bp {

#define R1_RLC_WEIGHT_DOMAIN 0x72316377u   // "wc1r": the combination weights the caller did not bring
#define R1_RLC_MAX_TERMS (1u << 24)        // unique terms per combination: 1 GiB of list; within bucket_fits and rlc_acc_to_sc's 2^24 sums
#define R1_RLC_SLICE 1024                  // proofs per front-end slice: bounds the per-proof staging

// one slice of one group: its proofs are [gp0, gp0 + nproofs) of the call, its unique terms [u0, u0 + nproofs U) of the combined list.
// nstride: nproofs rounded up to 64 (the lanes of the padding add nothing), so that the 64 lanes of a wavefront share their term;
// ngen: the generator terms per proof, 2 pn + 2 -- or 0 for a slice whose padded_n exceeds the generators (every proof stopped in
// launch 1; pn may then exceed PN, and no lane may form a row from it)
struct r1_rlc_slice {
    uint32_t nproofs, nstride, U, ngen, pn, PN;
    uint32_t gp0, u0;
};

// the shared key and rho body under this check's names and domain (the host harness drives them so)
using r1_rlc_key = rlc_key;
BP_HD void r1_rlc_rho_thread(uint32_t gp, const uint8_t *weights64, const r1_rlc_key &key, uint32_t *rho) {
    rlc_rho_thread(gp, weights64, key, R1_RLC_WEIGHT_DOMAIN, rho);
}

// generator row g (of 2 pn + 2) of a proof with padded_n pn -> row of the combined MSM over PN >= pn
BP_HD uint32_t r1_rlc_gen_row(uint32_t g, uint32_t pn, uint32_t PN) { return g < 2 + pn ? g : g + (PN - pn); }

// rlc_weigh_thread's index map: the U unique terms of a proof lie side by side in uniq_sc / uniq_pt, its 2 pn + 2 generator coefficients
// in gen_sc; generator term g lands on r1_rlc_gen_row
struct r1_rlc_map {
    uint32_t U, pn, PN;
    const uint32_t *gen_sc;
    BP_HD uint64_t uniq(uint32_t p, uint32_t t) const { return (uint64_t)p * U + t; }
    BP_HD const uint32_t *shared(uint32_t p, uint32_t g) const { return gen_sc + ((uint64_t)p * (2 * pn + 2) + g) * 8; }
    BP_HD uint32_t row(uint32_t g) const { return r1_rlc_gen_row(g, pn, PN); }
};

// lane tid = term * nstride + proof over U + ngen terms (rlc_weigh_thread); the lanes of term 0 also hand the proof's front-end code to
// its place in the call's gstatus (nproofs <= nstride, so tid < nproofs is term 0 of proof tid)
BP_HD bool r1_rlc_weigh_thread(uint32_t tid, const r1_rlc_slice &sl, const uint32_t *status, const uint32_t *rho, const uint32_t *gen_sc,
                               const uint32_t *uniq_sc, const uint32_t *uniq_pt, uint32_t *comb_sc, uint32_t *comb_pt, uint32_t *gstatus, sc &v,
                               uint32_t &row) {
    if (tid < sl.nproofs) gstatus[sl.gp0 + tid] = status[tid];
    const r1_rlc_map map{sl.U, sl.pn, sl.PN, gen_sc};
    return rlc_weigh_thread(tid, sl.nproofs, sl.nstride, sl.U, map, status, rho + 8 * (uint64_t)sl.gp0, uniq_sc, uniq_pt, comb_sc + 8 * (uint64_t)sl.u0,
                            comb_pt + 8 * (uint64_t)sl.u0, v, row);
}

// the combinations' points summed (ncomb >= 1): res[0..8) = compress(sum), rst[0] = 0 when every point decoded -- what a single MSM
// leaves, and what rlc_verdict_thread takes
BP_HD void r1_rlc_sum_thread(uint32_t ncomb, const uint32_t *parts, const uint8_t *part_status, uint32_t *res, uint8_t *rst) {
    if (ncomb == 1) {   // (the usual case: the one MSM's encoding as it is -- no decompression, 0.3 ms on one lane)
        for (int i = 0; i < 8; i++) res[i] = parts[i];
        rst[0] = part_status[0] != 0;
        return;
    }
    ge_ext acc, q;
    ge_identity(acc);
    uint8_t bad = 0;
    for (uint32_t j = 0; j < ncomb; j++) {
        if (part_status[j] != 0 || !ristretto_decompress(q, parts + 8 * (uint64_t)j)) {
            bad = 1;
            continue;
        }
        ge_add(acc, acc, q);
    }
    ristretto_compress(res, acc);
    rst[0] = bad;
}

}  // namespace bp
#endif
