// k_pedersen.hip: batches of Pedersen commitments and openings (pedersen.h), one launch each, lane = row.
// Capped at 168 registers (three wavefronts per SIMD) like the neighbouring table walks (k_fb_walk).
#include <hip/hip_runtime.h>
#include "kernels.h"

using namespace bp;

// a lane's parking space in LDS (pedersen.h ped_park): the recoded scalar as [word][lane], the accumulated point -- 12.5 KiB per workgroup
#define PED_PARK                                    \
    __shared__ uint32_t s_rw[10 * BP_BLOCK];        \
    __shared__ ge_ext s_pt[BP_BLOCK];               \
    const ped_park pk = {s_rw + threadIdx.x, BP_BLOCK, s_pt + threadIdx.x};

template <bool CT>
__global__ void __launch_bounds__(BP_BLOCK, 3) k_ped_commit(uint32_t nbatch, ped_in in, fb_params prm, const uint32_t *gen_ids, const fb_entry *table,
                                                            uint32_t *out_words, uint32_t *blindings_out, uint8_t *status) {
    PED_PARK
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nbatch) ped_commit_lane<CT>(i, in, pk, prm, gen_ids, table, out_words, blindings_out, status);
}
template __global__ void k_ped_commit<false>(uint32_t, ped_in, fb_params, const uint32_t *, const fb_entry *, uint32_t *, uint32_t *, uint8_t *);
template __global__ void k_ped_commit<true>(uint32_t, ped_in, fb_params, const uint32_t *, const fb_entry *, uint32_t *, uint32_t *, uint8_t *);

__global__ void __launch_bounds__(BP_BLOCK, 3) k_ped_open(uint32_t nbatch, ped_in in, const uint32_t *commitments, fb_params prm, const uint32_t *gen_ids,
                                                          const fb_entry *table, uint8_t *verdict) {
    PED_PARK
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nbatch) ped_open_lane(i, in, pk, commitments, prm, gen_ids, table, verdict);
}
