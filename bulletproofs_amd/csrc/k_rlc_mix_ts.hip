// k_rlc_mix_ts.hip: HIP kernel of libbpgpu.so (gfx950) for the batch-combined check over range proofs of mixed shapes on caller-supplied
// transcripts at DIFFERING STROBE positions; a thin __global__ wrapper around rlc_mix.h and the lane bodies of rangeproof.h.
#include <hip/hip_runtime.h>
#define BP_KECCAK_OUTOFLINE 1   // byte-wise STROBE framing reaches Keccak-f[1600] through ONE out-of-line copy in this translation unit (keccak.h), as k_rp1.hip
#include "kernels.h"

using namespace bp;

// k_rlc_mix_front with the byte-wise replay in its transcript role (the form k_rp_stage1<false> is of k_rp_stage1<true>): proof p starts from
// ts_in[p], whatever its position, and rangeproof_domain_sep(n, m) is applied here (BP_TS_DOMSEP).  The same 50 * RP_BLOCK-word sponge layout,
// one lane per proof; the weight role and the decode role are those of k_rlc_mix_front.
__global__ void __launch_bounds__(RP_BLOCK) k_rlc_mix_front_replay(rp_shape sh, rp_strobe_init init, uint32_t n_tr, const uint8_t *proofs,
                                                                   const uint8_t *commitments, const uint8_t *rng64, const uint8_t *rho64, uint32_t *fields,
                                                                   uint32_t *status, fb_params prm, uint32_t lg_m, uint32_t *uniq_sc, const uint32_t *ts_in,
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
            rm_front_thread<false>(p, sh, init, st, rp_resolve(p, sh, proofs, commitments, rng64, segs), (const rp_script_hdr *)nullptr, fields, status, prm,
                                   lg_m, uniq_sc, rho64, BP_TS_DOMSEP, ts_in, ts_out);
    } else {
        const uint32_t t = (blockIdx.x - n_tr) * RP_BLOCK + threadIdx.x;
        if (t < sh.nproofs * sh.U) rp_points_thread<false>(t, sh, rp_resolve(t / sh.U, sh, proofs, commitments, nullptr, segs), (ge_cached *)nullptr, status);
    }
}
