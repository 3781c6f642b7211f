// k_ipp_rlc.hip: HIP kernels of libbpgpu.so (gfx950) for the batch-combined InnerProductProof check; thin __global__ wrappers around
// ipp_rlc.h.  (Its front end is k_ipp_vs_front of k_ipp.hip; its rho, table-mode reduce and verdict launches are the shared ones of
// k_rlc_comb.hip.)
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "rlc_wave.h"

using namespace bp;

// lane = proof: its U unique terms into the combined list, rho a and rho b parked for k_ipp_rlc_weigh
__global__ void __launch_bounds__(64) k_ipp_rlc_uniq(ipp_rlc_shape sh, const uint32_t *status, const uint32_t *rho, const uint8_t *proofs, const uint8_t *P,
                                                      const uint8_t *Q, const uint32_t *u_sq, const uint32_t *u_inv_sq, uint32_t *ab, uint32_t *comb_sc,
                                                      uint32_t *comb_pt) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < sh.nproofs) ipp_rlc_uniq_thread(p, sh, status, rho, proofs, P, Q, u_sq, u_inv_sq, ab, comb_sc, comb_pt);
}

// lane = (block of B rows, proof), proof fastest, over nstride (a multiple of 64) proofs: the 64 lanes of a wavefront stand on the same
// row at every step, so every row takes one atomic per limb per wavefront.  Launched with exactly nstride 2n / B lanes: every lane
// reaches every rlc_accumulate (no early return, a uniform trip count).
__global__ void __launch_bounds__(64) k_ipp_rlc_weigh(ipp_rlc_shape sh, const uint32_t *status, const uint32_t *ab, const uint32_t *tab, const uint8_t *Gf,
                                                       const uint8_t *Hf, unsigned long long *acc) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    ipp_rlc_lane ln;
    ipp_rlc_weigh_begin(tid, sh, status, ab, tab, Gf, Hf, ln);
    for (uint32_t g = 0; g < sh.B; g++) {
        sc v;
        uint32_t row;
        const bool active = ipp_rlc_weigh_step(g, sh, ln, v, row);
        rlc_accumulate(acc, row, v, active, true);
    }
}

// explicit bases, lane = row of (G_0.., H_0..): the accumulated coefficient mod l and the base's encoding beside it, the head of the
// combined list (generator-table mode reduces with k_rlc_comb_reduce)
__global__ void __launch_bounds__(64) k_ipp_rlc_reduce(uint32_t nrows, uint32_t n, const unsigned long long *acc, const uint8_t *G, const uint8_t *H,
                                                        uint32_t *out_sc, uint32_t *out_pt) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < nrows) ipp_rlc_reduce_thread(g, n, (const uint64_t *)acc, G, H, out_sc, out_pt);
}
