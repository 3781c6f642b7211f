// k_r1cs_rlc.hip: HIP kernels of libbpgpu.so (gfx950) for the batch-combined R1CS check; thin __global__ wrappers around r1cs_rlc.h.
// (Its rho, reduce and verdict launches are the shared ones of k_rlc_comb.hip.)
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "rlc_wave.h"

using namespace bp;

// lane = (term, proof) of one slice, proof fastest, over nstride (a multiple of 64) proofs: the 64 lanes of a wavefront share their
// term, so generator rows take one atomic per limb per wavefront.  Launched with exactly nstride (U + ngen) lanes: every lane reaches
// rlc_accumulate (no early return), and only wavefronts of generator terms (t >= U) enter it.
__global__ void __launch_bounds__(64) k_r1cs_rlc_weigh(r1_rlc_slice sl, const uint32_t *status, const uint32_t *rho, const uint32_t *gen_sc,
                                                        const uint32_t *uniq_sc, const uint32_t *uniq_pt, uint32_t *comb_sc, uint32_t *comb_pt,
                                                        uint32_t *gstatus, unsigned long long *acc) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    sc v;
    uint32_t row;
    const bool gen = r1_rlc_weigh_thread(tid, sl, status, rho, gen_sc, uniq_sc, uniq_pt, comb_sc, comb_pt, gstatus, v, row);
    if (tid / sl.nstride >= sl.U) rlc_accumulate(acc, row, v, gen, true);   // (uniform across the wavefront)
}

// one lane: the combinations' points summed
__global__ void __launch_bounds__(64) k_r1cs_rlc_sum(uint32_t ncomb, const uint32_t *parts, const uint8_t *part_status, uint32_t *res, uint8_t *rst) {
    if (blockIdx.x == 0 && threadIdx.x == 0) r1_rlc_sum_thread(ncomb, parts, part_status, res, rst);
}
