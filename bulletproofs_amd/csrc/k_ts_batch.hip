// k_ts_batch.hip: HIP kernel of libbpgpu.so (gfx950) for batches of Merlin transcripts; a thin __global__ wrapper around ts_batch.h.
#include <hip/hip_runtime.h>
#include "kernels.h"

using namespace bp;

// lane = row (transcript); one wavefront per workgroup, the sponge words in LDS, strided by the workgroup size
__global__ void __launch_bounds__(TSB_BLOCK) k_ts_batch(uint32_t nbatch, const uint32_t *ts_in, uint32_t ts_in_stride, uint32_t *ts_out, const tsb_op *ops,
                                                        uint32_t nops, const uint8_t *labels) {
    __shared__ uint32_t lds[TSB_LDS_WORDS * TSB_BLOCK];
    const uint64_t r = (uint64_t)blockIdx.x * TSB_BLOCK + threadIdx.x;
    tsb_thread(threadIdx.x, r, r < nbatch, lds, ts_in, ts_in_stride, ts_out, ops, nops, labels);
}
