// Wavefront accumulation of batch-combination coefficients (rlc.h's ten 28-bit limb sums) for the kernels of k_rlc.hip and
// k_r1cs_rlc.hip.  Device code only: DPP and lane reads.
#ifndef BPGPU_RLC_WAVE_H
#define BPGPU_RLC_WAVE_H
#include <hip/hip_runtime.h>
#include "rlc.h"

namespace bp {

// sum over the wavefront of a value below 2^28 per lane: four DPP prefix steps inside each row of 16 lanes
// (row sums < 2^32), then the four row totals are read to scalars and added in 64 bits
__device__ __forceinline__ uint64_t wave_sum_u28(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, true);   // row_shr:1, zero fill
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, true);   // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, true);   // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, true);   // row_shr:8
    return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)x, 15) + (uint32_t)__builtin_amdgcn_readlane((int)x, 31) +
           (uint32_t)__builtin_amdgcn_readlane((int)x, 47) + (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}
// add one scalar per lane into the batch accumulator of generator row `row` (ten 64-bit limb sums).
// uniform: all 64 lanes of the wavefront hold contributions to the SAME row -> one atomic per limb per wavefront
__device__ __forceinline__ void rlc_accumulate(unsigned long long *acc, uint32_t row, const sc &v, bool active, bool uniform) {
    uint64_t l[10];
    rlc_limbs(l, v);
    if (uniform) {
#pragma unroll
        for (int i = 0; i < 10; i++) {
            const uint64_t t = wave_sum_u28(active ? (uint32_t)l[i] : 0u);
            if (__lane_id() == 0) atomicAdd(acc + (uint64_t)row * 10 + i, (unsigned long long)t);
        }
    } else if (active) {
#pragma unroll
        for (int i = 0; i < 10; i++) atomicAdd(acc + (uint64_t)row * 10 + i, (unsigned long long)l[i]);
    }
}

}  // namespace bp
#endif
