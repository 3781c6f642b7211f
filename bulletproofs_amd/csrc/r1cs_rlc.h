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
// and once per combination: the reduction of the accumulators (rlc_acc_to_sc), ONE shared-generator MSM over PN, the sum of the
// combinations' points (r1_rlc_sum_thread) and the verdicts (r1_rlc_verdict_thread).
#ifndef BPGPU_R1CS_RLC_H
#define BPGPU_R1CS_RLC_H
#include "r1cs.h"
#include "rlc.h"

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
struct r1_rlc_key {
    uint32_t w[8];
};

// generator row g (of 2 pn + 2) of a proof with padded_n pn -> row of the combined MSM over PN >= pn
BP_HD uint32_t r1_rlc_gen_row(uint32_t g, uint32_t pn, uint32_t PN) { return g < 2 + pn ? g : g + (PN - pn); }

// rho of the call's proof gp: from_bytes_mod_order_wide(weights64[gp]), or of block gp of ChaCha20(key, nonce = R1_RLC_WEIGHT_DOMAIN)
BP_HD void r1_rlc_rho_thread(uint32_t gp, const uint8_t *weights64, const r1_rlc_key &key, uint32_t *rho) {
    uint32_t w16[16];
    if (weights64) {
        const uint8_t *src = weights64 + 64 * (uint64_t)gp;
        for (int i = 0; i < 16; i++)
            w16[i] = (uint32_t)src[4 * i] | ((uint32_t)src[4 * i + 1] << 8) | ((uint32_t)src[4 * i + 2] << 16) | ((uint32_t)src[4 * i + 3] << 24);
    } else {
        chacha20_block(key.w, (uint64_t)gp, R1_RLC_WEIGHT_DOMAIN, 0u, w16);
    }
    sc r;
    sc_from_wide(r, w16);
    store_words8(rho + 8 * (uint64_t)gp, r);
}

// lane tid = term * nstride + proof over U + ngen terms.  Unique terms go to the combined list; a generator term sets its combined row
// `row` (also in the padding lanes: it is the wavefront's row) and returns true with its weighted coefficient `v` for the caller's
// accumulation (false for a proof that stopped and for the padding).
BP_HD bool r1_rlc_weigh_thread(uint32_t tid, const r1_rlc_slice &sl, const uint32_t *status, const uint32_t *rho, const uint32_t *gen_sc,
                               const uint32_t *uniq_sc, const uint32_t *uniq_pt, uint32_t *comb_sc, uint32_t *comb_pt, uint32_t *gstatus, sc &v,
                               uint32_t &row) {
    const uint32_t t = tid / sl.nstride, p = tid - t * sl.nstride;
    sc_0(v);
    row = t < sl.U ? 0u : r1_rlc_gen_row(t - sl.U, sl.pn, sl.PN);
    if (p >= sl.nproofs) return false;
    const uint32_t st = status[p];
    if (t == 0) gstatus[sl.gp0 + p] = st;
    sc x, r;
#pragma unroll
    for (int q = 0; q < 8; q++) r.v[q] = rho[8 * ((uint64_t)sl.gp0 + p) + q];
    if (t < sl.U) {
        const uint64_t src = ((uint64_t)p * sl.U + t) * 8, dst = (uint64_t)sl.u0 * 8 + src;
        if (st != 0) {
            sc_0(x);
#pragma unroll
            for (int q = 0; q < 8; q++) comb_pt[dst + q] = 0u;
        } else {
#pragma unroll
            for (int q = 0; q < 8; q++) {
                x.v[q] = uniq_sc[src + q];
                comb_pt[dst + q] = uniq_pt[src + q];
            }
            sc_mul(x, x, r);
        }
        store_words8(comb_sc + dst, x);
        return false;
    }
    const uint32_t g = t - sl.U;
    if (st != 0) return false;
    const uint64_t src = ((uint64_t)p * (2 * sl.pn + 2) + g) * 8;
#pragma unroll
    for (int q = 0; q < 8; q++) x.v[q] = gen_sc[src + q];
    sc_mul(v, x, r);
    return true;
}

// the combinations' points summed (ncomb >= 1): res[0..8) = compress(sum), res[8] = 1 when every point decoded
BP_HD void r1_rlc_sum_thread(uint32_t ncomb, const uint32_t *parts, const uint8_t *part_status, uint32_t *res) {
    if (ncomb == 1) {   // (the usual case: the one MSM's encoding as it is -- no decompression, 0.3 ms on one lane)
        for (int i = 0; i < 8; i++) res[i] = parts[i];
        res[8] = part_status[0] == 0 ? 1u : 0u;
        return;
    }
    ge_ext acc, q;
    ge_identity(acc);
    uint32_t ok = 1;
    for (uint32_t j = 0; j < ncomb; j++) {
        if (part_status[j] != 0 || !ristretto_decompress(q, parts + 8 * (uint64_t)j)) {
            ok = 0;
            continue;
        }
        ge_add(acc, acc, q);
    }
    ristretto_compress(res, acc);
    res[8] = ok;
}

// verdict of the call's proof gp: its front-end code, else 0 when R is the identity and every point decoded, else undecided (the host
// then re-verifies proof by proof); lane 0 also writes the 33 batch bytes
BP_HD void r1_rlc_verdict_thread(uint32_t gp, const uint32_t *gstatus, const uint32_t *res, uint8_t *verdict, uint8_t *batch_out) {
    uint32_t nz = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) nz |= res[i];
    const bool pass = res[8] != 0 && nz == 0;
    verdict[gp] = gstatus[gp] ? (uint8_t)gstatus[gp] : (pass ? (uint8_t)BP_VERDICT_OK : (uint8_t)BP_VERDICT_UNDECIDED);
    if (gp == 0) {
        batch_out[0] = pass ? 0 : 1;
        for (int i = 0; i < 32; i++) batch_out[1 + i] = res[8] ? (uint8_t)(res[i >> 2] >> (8 * (i & 3))) : 0;
    }
}

}  // namespace bp
#endif
