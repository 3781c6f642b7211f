// k_rlc_mix.hip: HIP kernels of libbpgpu.so (gfx950) for the batch-combined check over range proofs of mixed shapes (its reduce and verdict
// launches: k_rlc_comb.hip); thin __global__ wrappers around rlc_mix.h and the lane bodies of rangeproof.h.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "rlc_wave.h"

using namespace bp;

// lane = proof of the call: its 64 library-drawn bytes of domain `dom`
__global__ void __launch_bounds__(64) k_rlc_mix_draw(uint32_t n, rlc_key key, uint32_t dom, uint32_t *out) {
    const uint32_t gp = blockIdx.x * blockDim.x + threadIdx.x;
    if (gp < n) rlc_draw_thread(gp, key, dom, out);
}

// launch 1 of one group, the roles of k_rp_stage1<true> in batch-combination mode: [0, n_tr) the scripted transcript replay, then the
// per-proof scalars times the proof's weight, the U coefficients as plain scalars into uniq_sc, lane = proof  ||  [n_tr, ..) the
// decode of the proof's and the commitments' points, lane = point: an undecodable one stops its proof (the decoded point itself is
// dropped: the call's one MSM decodes the encodings of the proofs that are left)
// ts_in / ts_out (bpgpu_rangeproof_verify_rlc_mixed_ts): one caller-supplied start state per proof, all at the position the script was
// compiled for, and where the advanced states go; both null for a group that starts from its label.  (States at differing positions:
// k_rlc_mix_front_replay, k_rlc_mix_ts.hip.)
__global__ void __launch_bounds__(RP_BLOCK) k_rlc_mix_front(rp_shape sh, rp_strobe_init init, uint32_t n_tr, const uint8_t *proofs, const uint8_t *commitments,
                                                            const uint8_t *rng64, const uint8_t *rho64, uint32_t *fields, uint32_t *status, fb_params prm,
                                                            uint32_t lg_m, uint32_t *uniq_sc, const rp_script_hdr *script, const uint32_t *ts_in,
                                                            uint32_t *ts_out) {
    __shared__ uint32_t lds[50 * RP_BLOCK];   // sponge states, word-major: word w of lane t at w*RP_BLOCK + t
    rp_seg_tab segs;
    segs.n = 0;
    if (blockIdx.x < n_tr) {
        const uint32_t p = blockIdx.x * RP_BLOCK + threadIdx.x;
        kstate st;
        st.w = lds + threadIdx.x;
        st.stride = RP_BLOCK;
        if (p < sh.nproofs)
            rm_front_thread<true>(p, sh, init, st, rp_resolve(p, sh, proofs, commitments, rng64, segs), script, fields, status, prm, lg_m, uniq_sc, rho64, 0u,
                                  ts_in, ts_out);
    } else {
        const uint32_t t = (blockIdx.x - n_tr) * RP_BLOCK + threadIdx.x;
        if (t < sh.nproofs * sh.U) rp_points_thread<false>(t, sh, rp_resolve(t / sh.U, sh, proofs, commitments, nullptr, segs), (ge_cached *)nullptr, status);
    }
}

// lane = (term, proof) of one group, proof fastest, over nstride proofs.  Launched with exactly nstride * rm_terms(sh) lanes: every lane
// reaches rlc_accumulate (no early return), and a wavefront's 64 lanes share their term, so a generator row takes one atomic per limb
// per wavefront.
__global__ void __launch_bounds__(64) k_rlc_mix_weigh(rm_group gr, rp_shape sh, fb_params prm, const uint8_t *proofs, const uint8_t *commitments,
                                                      const uint32_t *status, const uint32_t *fields, const uint32_t *uniq_sc, uint32_t *comb_sc,
                                                      uint32_t *comb_pt, uint32_t *gstatus, unsigned long long *acc) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t p, q;
    bool live;
    sc r0, r1;
    const uint32_t role = rm_weigh_thread(tid, gr, sh, proofs, commitments, status, fields, uniq_sc, comb_sc, comb_pt, gstatus, p, q, live, r0, r1);
    if (role == 1) {   // (role is uniform across the wavefront)
        rlc_accumulate(acc, 0u, r0, live, true);
        rlc_accumulate(acc, 1u, r1, live, true);
    } else if (role == 2) {
        sc g[4], h[4];
        for (int j = 0; j < 4; j++) {
            sc_0(g[j]);
            sc_0(h[j]);
        }
        if (p < gr.nproofs) rp_expand_b4_thread(q * sh.nproofs + p, sh, prm, fields, nullptr, status, g, h);
#pragma unroll 1   // (unrolled, g and h are in scratch all the same: rp_expand_b4_thread stores them by its own run-time index; +12 KB of code)
        for (uint32_t j = 0; j < 4; j++) {
            uint32_t row_g, row_h;
            rm_quad_rows(gr, q, j, row_g, row_h);
            rlc_accumulate(acc, row_g, g[j], live, true);
            rlc_accumulate(acc, row_h, h[j], live, true);
        }
    }
}
