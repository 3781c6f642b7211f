// k_lin_rlc.hip: HIP kernels of libbpgpu.so (gfx950) for the batch-combined LinearProof check; thin __global__ wrappers around linear_rlc.h.
// (Its rho and verdict launches are the shared ones of k_rlc_comb.hip.)
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "rlc_wave.h"

using namespace bp;

// lane = (term, proof), proof fastest, over nstride (a multiple of 64) proofs: the 64 lanes of a wavefront share their term, so the
// base rows take one atomic per limb per wavefront.  Launched with exactly nstride (U + n + 2) lanes: every lane reaches
// rlc_accumulate (no early return), and only wavefronts of shared-base terms (t >= U) enter it.
__global__ void __launch_bounds__(64) k_lin_rlc_weigh(lin_rlc_shape sh, const uint32_t *status, const uint32_t *rho, const uint32_t *gen_sc,
                                                       const uint32_t *list_sc, const uint32_t *list_pt, uint32_t *comb_sc, uint32_t *comb_pt,
                                                       unsigned long long *acc) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    sc v;
    uint32_t row;
    const bool base = lin_rlc_weigh_thread(tid, sh, status, rho, gen_sc, list_sc, list_pt, comb_sc, comb_pt, v, row);
    if (tid / sh.nstride >= sh.U) rlc_accumulate(acc, row, v, base, true);   // (uniform across the wavefront)
}

// explicit bases, lane = row of (B, F, G_0..): the accumulated coefficient mod l and the base's encoding beside it, the head of the
// combined list (generator-table mode reduces with k_rlc_comb_reduce)
__global__ void __launch_bounds__(64) k_lin_rlc_reduce(uint32_t nrows, const unsigned long long *acc, const uint8_t *B, const uint8_t *F,
                                                        const uint8_t *G, uint32_t *out_sc, uint32_t *out_pt) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < nrows) lin_rlc_reduce_thread(g, (const uint64_t *)acc, B, F, G, out_sc, out_pt);
}
