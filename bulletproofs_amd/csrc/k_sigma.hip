// k_sigma.hip: proofs of recorded linear relations between points (sigma.h).  Creation: k_sig_vb, lane = (instance-base term, row), built
// at two wavefronts per SIMD (209 registers; under the 168 cap it spills: DESIGN 3.12); k_sig_walk, lane = (equation, row), capped at 168
// registers (three wavefronts per SIMD) like k_opn_create; k_sig_finish, lane = row.  Verification: k_sig_front and k_sig_verdict, lane =
// proof; k_sig_rlc_weigh, lane = (term, proof).
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "rlc_wave.h"

using namespace bp;

// creation, launch 1: lane = (product, row of the slice), row fastest, nvb * ws.nstride lanes exactly (ws.nstride: the slice's rows rounded
// up to 64, so a wavefront shares its product); the 10 LDS words per lane hold the recoded nonce
template <bool CT>
__global__ void __launch_bounds__(BP_BLOCK, 2) k_sig_vb(const sig_rel *rel, sig_create_in in, sig_ws ws) {
    __shared__ uint32_t lds[10 * BP_BLOCK];
    const ped_park pk = {lds + threadIdx.x, BP_BLOCK, nullptr};
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t v = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid / ws.nstride)), row = ws.row0 + (tid - v * ws.nstride);   // (nstride is a multiple of 64)
    if (row < in.nrows) sig_vb_lane<CT>(v, row, *rel, in, pk, ws);
}
template __global__ void k_sig_vb<false>(const sig_rel *, sig_create_in, sig_ws);
template __global__ void k_sig_vb<true>(const sig_rel *, sig_create_in, sig_ws);

// launch 2: lane = (equation, row of the slice), row fastest, E * ws.nstride lanes exactly; the 50 LDS words per lane are the walk's parking space (pedersen.h ped_park), as in k_ped_commit
template <bool CT>
__global__ void __launch_bounds__(BP_BLOCK, 3) k_sig_walk(sig_rel rel, sig_create_in in, sig_ws ws, uint32_t nslice, fb_params prm, const fb_entry *table,
                                                          uint32_t *proofs_out) {
    static_assert(sizeof(ge_ext) == 40 * sizeof(uint32_t), "the points fill rows 10 .. 49");
    __shared__ __align__(16) uint32_t lds[50 * BP_BLOCK];
    const ped_park pk = {lds + threadIdx.x, BP_BLOCK, (ge_ext *)(lds + 10 * BP_BLOCK) + threadIdx.x};
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid / ws.nstride)), i = tid - k * ws.nstride;   // (nstride is a multiple of 64: the wavefront shares k)
    if (i < nslice) sig_walk_lane<CT>(k, ws.row0 + i, rel, in, pk, ws, prm, table, proofs_out);
}
template __global__ void k_sig_walk<false>(sig_rel, sig_create_in, sig_ws, uint32_t, fb_params, const fb_entry *, uint32_t *);
template __global__ void k_sig_walk<true>(sig_rel, sig_create_in, sig_ws, uint32_t, fb_params, const fb_entry *, uint32_t *);

// launch 3: lane = row of the batch, the sponge in LDS
__global__ void __launch_bounds__(RP_BLOCK) k_sig_finish(const sig_rel *rel, sig_create_in in, const uint32_t *bad, uint32_t *proofs_out, uint8_t *status,
                                                          uint32_t *ts_out) {
    __shared__ uint32_t lds[50 * RP_BLOCK];
    const uint32_t p = blockIdx.x * RP_BLOCK + threadIdx.x;
    kstate st;
    st.w = lds + threadIdx.x;
    st.stride = RP_BLOCK;
    if (p < in.nrows) sig_finish_lane(p, *rel, in, st, bad, proofs_out, status, ts_out);
}

// the verifier's front end, shared by the per-proof and the combined check
__global__ void __launch_bounds__(RP_BLOCK) k_sig_front(const sig_rel *rel, uint32_t nproofs, rp_strobe_init init, const uint32_t *proofs, const uint32_t *points,
                                                         const uint32_t *ts_in, uint32_t ts_in_stride, uint32_t *eq_sc, uint32_t *eq_pt, uint32_t *gen_sc,
                                                         uint32_t *status, uint32_t *ts_out) {
    __shared__ uint32_t lds[50 * RP_BLOCK];
    const uint32_t p = blockIdx.x * RP_BLOCK + threadIdx.x;
    kstate st;
    st.w = lds + threadIdx.x;
    st.stride = RP_BLOCK;
    if (p < nproofs) sig_front_lane(p, *rel, init, st, proofs, points, ts_in, ts_in_stride, eq_sc, eq_pt, gen_sc, status, ts_out);
}

__global__ void __launch_bounds__(64) k_sig_verdict(uint32_t n, uint32_t E, const uint32_t *status, const uint8_t *msm_status, const uint32_t *msm_out, uint8_t *verdict) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) sig_verdict_thread(p, E, status, msm_status, msm_out, verdict);
}

// lane = (term, proof), proof fastest, over nstride (a multiple of 64) proofs and P + E + 2 + G terms: launched with exactly that many
// lanes, so every lane reaches rlc_accumulate and only the wavefronts of the shared rows enter it (k_opn_rlc_weigh's shape)
__global__ void __launch_bounds__(64) k_sig_rlc_weigh(const sig_rel *rel, uint32_t nproofs, uint32_t nstride, const uint32_t *status, const uint32_t *rho,
                                                       const uint32_t *gen_sc, const uint32_t *eq_sc, const uint32_t *eq_pt, const uint32_t *points,
                                                       uint32_t *comb_sc, uint32_t *comb_pt, unsigned long long *acc) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    sc v;
    uint32_t row;
    const bool base = sig_rlc_weigh_thread(tid, nproofs, nstride, *rel, status, rho, gen_sc, eq_sc, eq_pt, points, comb_sc, comb_pt, v, row);
    if (tid / nstride >= rel->P + rel->E) rlc_accumulate(acc, row, v, base, true);   // (uniform across the wavefront)
}
