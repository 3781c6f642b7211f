// k_rlc_comb.hip: HIP kernels of libbpgpu.so (gfx950) that the combined checks ending in one multiscalar multiplication share (R1CS,
// linear proofs, range proofs of mixed shapes); thin __global__ wrappers around rlc_comb.h.
#include <hip/hip_runtime.h>
#include "kernels.h"

using namespace bp;

// lane = proof of the call: its combination weight rho (plain scalar, 8 words), under the family's weight domain
__global__ void __launch_bounds__(64) k_rlc_comb_rho(uint32_t n, const uint8_t *weights64, rlc_key key, uint32_t dom, uint32_t *rho) {
    const uint32_t gp = blockIdx.x * blockDim.x + threadIdx.x;
    if (gp < n) rlc_rho_thread(gp, weights64, key, dom, rho);
}

// lane = row of the combination's MSM: the accumulated coefficient mod l
__global__ void __launch_bounds__(64) k_rlc_comb_reduce(uint32_t nrows, const unsigned long long *acc, uint32_t *out_sc) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < nrows) rlc_reduce_thread(g, (const uint64_t *)acc, out_sc);
}

// lane = proof of the call
__global__ void __launch_bounds__(64) k_rlc_comb_verdict(uint32_t n, const uint32_t *gstatus, const uint32_t *res, const uint8_t *rst, uint8_t *verdict,
                                                         uint8_t *batch_out) {
    const uint32_t gp = blockIdx.x * blockDim.x + threadIdx.x;
    if (gp < n) rlc_verdict_thread(gp, gstatus, res, rst, verdict, batch_out);
}
