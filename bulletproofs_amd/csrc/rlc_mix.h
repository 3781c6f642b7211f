// Batch combination of range proofs of MIXED shapes (bpgpu_rangeproof_verify_rlc_mixed, include/bpgpu.h): rlc.h's combination across
// groups of different (n, m), as r1cs_rlc.h does across circuits.
//
//   R = sum_i rho_i * MegaCheck_i ,   MegaCheck_i = the multiscalar multiplication of mod.rs:421-443 for proof i
//     = sum_g (sum_i rho_i s_{i,g}) P_g  +  sum_i sum_u (rho_i t_{i,u}) Q_{i,u}
//
// BulletproofGens::new(N, M) serves every n <= N, m <= M from the same points (generators.rs:157-259: party j's G_j[i], H_j[i] are the
// first n of its N), so the generator coefficients of proofs of different shapes add up on shared rows once they are laid out on the
// call's (N, M) = (max n, max m): B_blinding and B keep rows 0 and 1, G_j[i] moves from 2 + j n + i to 2 + j N + i, H_j[i] from
// 2 + n m + j n + i to 2 + N M + j N + i (rm_gen_row; the order of gen_ids_for(N, M)).
// Per group:
//   k_rlc_mix_front  launch 1 of the one-shape combination (transcript replay, per-proof scalars with the weight applied, point decode)
//                    with the U = 4 + 2k + m coefficients as plain canonical scalars (rp_expand_a_thread<true>)
//   k_rlc_mix_weigh  lane = (term, proof), proof fastest over nstride (a multiple of 64) proofs: the U unique terms into the group's slice
//                    of the call's combined list (scalar 0 and the identity encoding for a proof that stopped), the B_blinding / B
//                    coefficients (RPF_ROW0 / RPF_ROW1) and the 2 n m exponents, four G and four H indices per lane
//                    (rp_expand_b4_thread), into rlc.h's limb sums at their remapped rows
// and once per call: the reduction (rlc_reduce_thread), ONE shared-generator MSM over (N, M) and the verdicts (rlc_verdict_thread; a group
// rejected as a whole has its verdicts from the per-shape path and RLC_GSTATUS_DONE in gstatus).
#ifndef BPGPU_RLC_MIX_H
#define BPGPU_RLC_MIX_H
#include "rangeproof.h"
#include "rlc_comb.h"

namespace bp {

// domains of the randomness the caller did not bring, block = the proof's index WITHIN THE CALL (never within its group: two proofs of
// one call must not share a weight) of ChaCha20(key, nonce = domain)
#define RM_WEIGHT_DOMAIN 0x786d6377u   // "wcmx": the combination weights
#define RM_RNG_DOMAIN 0x786d6372u      // "rcmx": the batching challenge's rng bytes (mod.rs:396)
#define RM_MAX_TERMS (1u << 24)        // proofs, and unique terms, of one call: rlc_acc_to_sc's 2^24 sums; 1 GiB of combined list

// one group: its proofs are [gp0, gp0 + nproofs) of the call, its unique terms [u0, u0 + nproofs U) of the combined list
struct rm_group {
    uint32_t nproofs, nstride;   // nstride: nproofs rounded up to 64 -- the 64 lanes of a wavefront share their term, the padding adds nothing
    uint32_t n, m, N, M;
    uint32_t gp0, u0;
};
// terms of the weigh launch: U unique ones, one for rows 0 and 1, n m / 4 quads of exponents
BP_HD uint32_t rm_terms(const rp_shape &sh) { return sh.U + 1 + sh.nm / 4; }

// generator row g (of 2 n m + 2, the order of gen_ids_for(n, m)) of a proof of shape (n, m) -> row of the combined MSM over (N, M)
BP_HD uint32_t rm_gen_row(uint32_t g, uint32_t n, uint32_t m, uint32_t N, uint32_t M) {
    if (g < 2) return g;
    const uint32_t nm = n * m;
    const bool is_h = g >= 2 + nm;
    const uint32_t i = g - 2 - (is_h ? nm : 0u), j = i / n;
    return 2 + (is_h ? N * M : 0u) + j * N + (i - j * n);
}

// the shared key and draw body under this check's names (the host harness drives them so)
using rm_key = rlc_key;
BP_HD void rm_draw_thread(uint32_t gp, const rm_key &key, uint32_t dom, uint32_t *out) { rlc_draw_thread(gp, key, dom, out); }

// lane = proof p of one group: launch 1's transcript role, then the per-proof scalars times the proof's weight with the U coefficients as
// plain scalars.  The two forms k_rp_stage1<SCRIPTED> has:
//   SCRIPTED  the per-shape script from `init`'s position -- a label's state (ts_in == nullptr), or one caller-supplied state per proof
//             (ts_in) when every state of the group sits at init's (pos, pos_begin, cur_flags) and the script was compiled for it with the
//             domain separator: only the 50 sponge words differ per lane
//   else      the byte-wise replay (rp_transcript_thread with ts_flags = BP_TS_DOMSEP) from ts_in[p], whatever its position
// ts_out (optional) gets the advanced state on every path of either form (rp_ts_passthrough / rp_ts_emit).
template <bool SCRIPTED>
BP_HD void rm_front_thread(uint32_t p, const rp_shape &sh, const rp_strobe_init &init, kstate st, const rp_inputs &in, const rp_script_hdr *script,
                           uint32_t *fields, uint32_t *status, const fb_params &prm, uint32_t lg_m, uint32_t *uniq_sc, const uint8_t *rho64,
                           uint32_t ts_flags, const uint32_t *ts_in, uint32_t *ts_out) {
    if (SCRIPTED) rp_transcript_scripted(p, sh, init, st, in, script, fields, status, ts_out, ts_in);
    else rp_transcript_thread(p, sh, init, st, in, fields, status, ts_flags, ts_in, ts_out);
    rp_expand_a_thread<true>(p, sh, prm, lg_m, fields, uniq_sc, (fb_digit *)nullptr, status, rho64);
}

// lane tid = term * nstride + proof.  Unique terms (term < U) go to the combined list and the lane is done (returns 0).  Term U: returns 1
// with the weighted B_blinding / B coefficients in r0 / r1 (zero for a proof that stopped and for the padding).  Terms above: returns 2 --
// the caller forms quad `q`'s exponents.  `p` is the lane's proof, `live` whether it contributes.
BP_HD uint32_t rm_weigh_thread(uint32_t tid, const rm_group &gr, const rp_shape &sh, const uint8_t *proofs, const uint8_t *commitments,
                               const uint32_t *status, const uint32_t *fields, const uint32_t *uniq_sc, uint32_t *comb_sc, uint32_t *comb_pt,
                               uint32_t *gstatus, uint32_t &p, uint32_t &q, bool &live, sc &r0, sc &r1) {
    const uint32_t t = tid / gr.nstride;
    p = tid - t * gr.nstride;
    q = t > sh.U ? t - sh.U - 1 : 0u;
    sc_0(r0);
    sc_0(r1);
    const uint32_t st = p < gr.nproofs ? status[p] : 1u;
    live = st == 0;
    if (t < sh.U) {
        if (p >= gr.nproofs) return 0;
        if (t == 0) gstatus[gr.gp0 + p] = st;
        const uint64_t src = ((uint64_t)p * sh.U + t) * 8, dst = (uint64_t)gr.u0 * 8 + src;
        if (!live) {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                comb_sc[dst + i] = 0u;
                comb_pt[dst + i] = 0u;
            }
        } else {
            rp_inputs in;
            in.pr = proofs + (uint64_t)p * sh.proof_len;
            in.cm = commitments + (uint64_t)p * sh.m * 32;
            in.rs = nullptr;
            in.init_w = nullptr;
            uint32_t w[8];
            load_words8(w, rp_unique_point_ptr(sh, in, t));
#pragma unroll
            for (int i = 0; i < 8; i++) {
                comb_sc[dst + i] = uniq_sc[src + i];
                comb_pt[dst + i] = w[i];
            }
        }
        return 0;
    }
    if (t == sh.U) {
        if (live) {
            rp_load(r0, fields, sh.nproofs, RPF_ROW0, p);
            rp_load(r1, fields, sh.nproofs, RPF_ROW1, p);
        }
        return 1;
    }
    return 2;
}
// rows of the combined MSM of quad q's index j (0 .. 3): G_{4q + j} and H_{4q + j}
BP_HD void rm_quad_rows(const rm_group &gr, uint32_t q, uint32_t j, uint32_t &row_g, uint32_t &row_h) {
    const uint32_t i = 4 * q + j;
    row_g = rm_gen_row(2 + i, gr.n, gr.m, gr.N, gr.M);
    row_h = rm_gen_row(2 + gr.n * gr.m + i, gr.n, gr.m, gr.N, gr.M);
}

}  // namespace bp
#endif
