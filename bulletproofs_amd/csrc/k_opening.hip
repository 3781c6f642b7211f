// k_opening.hip: proofs of knowledge of commitment openings (opening.h), lane = proof.
// The prover is capped at 168 registers (three wavefronts per SIMD) like the neighbouring table walks (k_ped_commit).
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "rlc_wave.h"

using namespace bp;

// ONE launch: walk and encode R, barrier, transcript and responses.  The 50 LDS words per lane serve twice: first as the walk's parking
// space (pedersen.h ped_park: 10 rows of the recoded scalar as [word][lane], then the accumulated points), then as the lanes' sponges
// ([word][lane]).  Launched in whole workgroups: a lane past the batch runs along on the last proof and stores nothing, so every lane
// reaches the barrier.
template <bool CT>
__global__ void __launch_bounds__(BP_BLOCK, 3) k_opn_create(opn_shape sh, opn_create_in in, fb_params prm, const uint32_t *gen_ids,
                                                            const fb_entry *table, uint32_t *proofs_out, uint8_t *status, uint32_t *ts_out) {
    static_assert(sizeof(ge_ext) == 40 * sizeof(uint32_t), "the points fill rows 10 .. 49");
    __shared__ __align__(16) uint32_t lds[50 * BP_BLOCK];   // (ge_ext's alignment: rows 10 .. 49 start at 2 560 B, a lane's point at 160 B steps)
    const ped_park pk = {lds + threadIdx.x, BP_BLOCK, (ge_ext *)(lds + 10 * BP_BLOCK) + threadIdx.x};
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < sh.nproofs;
    const uint32_t p = live ? i : sh.nproofs - 1;
    uint32_t R[8];
    opn_create_walk<CT>(p, sh, in, pk, prm, gen_ids, table, R);
    __syncthreads();
    if (!live) return;
    kstate st;
    st.w = lds + threadIdx.x;
    st.stride = BP_BLOCK;
    opn_create_finish(p, sh, in, st, R, proofs_out, status, ts_out);
}
template __global__ void k_opn_create<false>(opn_shape, opn_create_in, fb_params, const uint32_t *, const fb_entry *, uint32_t *, uint8_t *, uint32_t *);
template __global__ void k_opn_create<true>(opn_shape, opn_create_in, fb_params, const uint32_t *, const fb_entry *, uint32_t *, uint8_t *, uint32_t *);

// the verifier's front end, shared by the per-proof and the combined check
__global__ void __launch_bounds__(RP_BLOCK) k_opn_front(opn_shape sh, rp_strobe_init init, const uint32_t *proofs, const uint32_t *commitments, const uint32_t *values,
                                                         const uint32_t *ts_in, uint32_t *uniq_sc, uint32_t *uniq_pt, uint32_t *gen_sc, uint32_t *status,
                                                         uint32_t *ts_out) {
    __shared__ uint32_t lds[50 * RP_BLOCK];
    const uint32_t p = blockIdx.x * RP_BLOCK + threadIdx.x;
    kstate st;
    st.w = lds + threadIdx.x;
    st.stride = RP_BLOCK;
    if (p < sh.nproofs) opn_front_lane(p, sh, init, st, proofs, commitments, values, ts_in, uniq_sc, uniq_pt, gen_sc, status, ts_out);
}

// lane = (term, proof), proof fastest, over nstride (a multiple of 64) proofs and 2 + 2 terms: launched with exactly 4 nstride lanes, so
// every lane reaches rlc_accumulate and only the wavefronts of the shared rows (t >= 2) enter it (k_lin_rlc_weigh's shape)
__global__ void __launch_bounds__(64) k_opn_rlc_weigh(uint32_t nproofs, uint32_t nstride, const uint32_t *status, const uint32_t *rho, const uint32_t *gen_sc,
                                                       const uint32_t *uniq_sc, const uint32_t *uniq_pt, uint32_t *comb_sc, uint32_t *comb_pt,
                                                       unsigned long long *acc) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    sc v;
    uint32_t row;
    const bool base = opn_rlc_weigh_thread(tid, nproofs, nstride, status, rho, gen_sc, uniq_sc, uniq_pt, comb_sc, comb_pt, v, row);
    if (tid / nstride >= 2) rlc_accumulate(acc, row, v, base, true);   // (uniform across the wavefront)
}
