// k_r1cs_check.hip: HIP kernels of libbpgpu.so (gfx950) for the R1CS witness check; thin __global__ wrappers around r1cs_check.h.
#include <hip/hip_runtime.h>
#include "kernels.h"

using namespace bp;

// lane = (proof, challenge)
__global__ void __launch_bounds__(64) k_r1c_chal(uint32_t nthreads, r1p_shape sh, const uint8_t *chal, uint32_t *fields, uint32_t *status) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid < nthreads) r1c_chal_thread(tid, sh, chal, fields, status);
}

// lane = (unit, proof of the slice), proof fastest
__global__ void __launch_bounds__(64) k_r1c_units(uint32_t nthreads, r1p_shape sh, uint32_t p0, uint32_t cnt, const r1c_unit *units, const r1p_term *terms,
                                                   const uint32_t *aw, const uint8_t *v, const uint32_t *fields, const uint32_t *status, uint32_t mapw,
                                                   uint32_t *partial, uint32_t *first, uint32_t *count, uint32_t *map) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid < nthreads) r1c_unit_thread(tid, sh, p0, cnt, units, terms, aw, v, fields, status, mapw, partial, first, count, map);
}

// lane = (long row, proof of the slice), proof fastest
__global__ void __launch_bounds__(64) k_r1c_long(uint32_t nthreads, uint32_t p0, uint32_t cnt, const r1c_long *longs, const uint32_t *partial,
                                                  const uint32_t *status, uint32_t mapw, uint32_t *first, uint32_t *count, uint32_t *map) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid < nthreads) r1c_long_thread(tid, p0, cnt, longs, partial, status, mapw, first, count, map);
}
