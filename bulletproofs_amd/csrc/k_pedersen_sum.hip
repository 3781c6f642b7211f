// k_pedersen_sum.hip: signed sums of Pedersen commitments and the balance check (pedersen_sum.h).  A term launch (lane = term,
// segmented reduction in LDS), reduce passes for rows of more than PSUM_SERIAL_MAX partials, a finish launch (lane = row).
// Capped at 168 registers (three wavefronts per SIMD) like the Pedersen kernels beside them (k_pedersen.hip).
#include <hip/hip_runtime.h>
#include "kernels.h"

using namespace bp;

static_assert(PSUM_BLOCK == BP_BLOCK, "pedersen_sum.h plans for workgroups of BP_BLOCK lanes");

// the workgroup's points and rows in LDS (10.25 KiB), and the log2(PSUM_BLOCK) steps between the load and the store of the partials
#define PSUM_LDS                                   \
    __shared__ ge_ext s_pt[PSUM_BLOCK];            \
    __shared__ uint32_t s_row[PSUM_BLOCK];         \
    const psum_lds l = {s_pt, s_row};
#define PSUM_REDUCE_AND_STORE                                        \
    __syncthreads();                                                 \
    _Pragma("unroll 1") for (uint32_t d = 1; d < PSUM_BLOCK; d <<= 1) {                  \
        ge_ext sum;                                                  \
        const bool on = psum_step_add(threadIdx.x, d, l, sum);       \
        __syncthreads();                                             \
        psum_step_store(threadIdx.x, l, sum, on);                    \
        __syncthreads();                                             \
    }                                                                \
    psum_store_partial(threadIdx.x, blockIdx.x, ps, l, partial);

__global__ void __launch_bounds__(BP_BLOCK, 3) k_psum_terms(psum_pass ps, const uint32_t *points, const uint8_t *signs, uint8_t *bad, ge_ext *partial) {
    PSUM_LDS
    psum_load_term(threadIdx.x, blockIdx.x, ps, points, signs, bad, l);
    PSUM_REDUCE_AND_STORE
}

__global__ void __launch_bounds__(BP_BLOCK, 3) k_psum_reduce(psum_pass ps, const ge_ext *src, ge_ext *partial) {
    PSUM_LDS
    psum_load_partial(threadIdx.x, blockIdx.x, ps, src, l);
    PSUM_REDUCE_AND_STORE
}

// the finish: a lane's parking space as in k_pedersen.hip (the recoded scalar as [word][lane], the point for the encoder)
#define PSUM_PARK                                   \
    __shared__ uint32_t s_rw[10 * BP_BLOCK];        \
    __shared__ ge_ext s_park[BP_BLOCK];             \
    const ped_park pk = {s_rw + threadIdx.x, BP_BLOCK, s_park + threadIdx.x};

template <bool CT>
__global__ void __launch_bounds__(BP_BLOCK, 3) k_psum_finish(uint32_t nbatch, ped_in in, fb_params prm, const uint32_t *gen_ids, const fb_entry *table, const uint32_t *slot,
                                                             const ge_ext *partial, const uint8_t *bad, uint32_t *out_words, uint8_t *status) {
    PSUM_PARK
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < nbatch) psum_sum_lane<CT>(r, in, pk, prm, gen_ids, table, slot, partial, bad, out_words, status);
}
template __global__ void k_psum_finish<false>(uint32_t, ped_in, fb_params, const uint32_t *, const fb_entry *, const uint32_t *, const ge_ext *, const uint8_t *, uint32_t *, uint8_t *);
template __global__ void k_psum_finish<true>(uint32_t, ped_in, fb_params, const uint32_t *, const fb_entry *, const uint32_t *, const ge_ext *, const uint8_t *, uint32_t *, uint8_t *);

__global__ void __launch_bounds__(BP_BLOCK, 3) k_psum_balance(uint32_t nbatch, ped_in in, fb_params prm, const uint32_t *gen_ids, const fb_entry *table, const uint32_t *slot,
                                                              const ge_ext *partial, const uint8_t *bad, uint8_t *verdict) {
    __shared__ uint32_t s_rw[10 * BP_BLOCK];   // (nothing is encoded: no point is parked)
    const ped_park pk = {s_rw + threadIdx.x, BP_BLOCK, nullptr};
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < nbatch) psum_balance_lane(r, in, pk, prm, gen_ids, table, slot, partial, bad, verdict);
}
