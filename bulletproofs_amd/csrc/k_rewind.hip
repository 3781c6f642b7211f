// k_rewind.hip: rewinding range proofs (rewind.h), lane = row.
// Capped at 168 registers (three wavefronts per SIMD) like the neighbouring table walks (k_ped_commit, k_opn_create).
#include <hip/hip_runtime.h>
#include "kernels.h"

using namespace bp;

// ONE launch: replay to x, the draws and the scalar arithmetic, barrier, walk and encode, compare.  The 50 LDS words per lane serve
// twice: first as the lanes' sponges ([word][lane]), then as the walk's parking space (pedersen.h ped_park: 10 rows of the recoded
// scalar as [word][lane], then the accumulated points) -- k_opn_create's two uses in the other order.  Launched in whole workgroups:
// a lane past the batch runs along on the last row up to the barrier and stores nothing, so every lane reaches it.
template <bool CT>
__global__ void __launch_bounds__(BP_BLOCK, 3) k_rewind(rwd_shape sh, rwd_in in, rwd_out out, fb_params prm, const uint32_t *gen_ids, const fb_entry *table) {
    static_assert(sizeof(ge_ext) == 40 * sizeof(uint32_t), "the points fill rows 10 .. 49");
    __shared__ __align__(16) uint32_t lds[50 * BP_BLOCK];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < sh.nproofs;
    const uint32_t p = live ? i : sh.nproofs - 1;
    uint32_t stat;
    {
        kstate st;
        st.w = lds + threadIdx.x;
        st.stride = BP_BLOCK;
        sc x, z;
        stat = rwd_replay(p, sh, in, st, x, z);
        stat = rwd_scalars<CT>(p, live, sh, in, out, stat, x, z);
    }
    __syncthreads();
    if (!live) return;   // (here, not at the stores: what only feeds a store under `live` would sink behind that branch, and the encoder's
                         // volatile reloads, which cannot sink, would then all be held in registers at once)
    const ped_park pk = {lds + threadIdx.x, BP_BLOCK, (ge_ext *)(lds + 10 * BP_BLOCK) + threadIdx.x};
    rwd_check<CT>(p, in, out, stat, pk, prm, gen_ids, table);
}
template __global__ void k_rewind<false>(rwd_shape, rwd_in, rwd_out, fb_params, const uint32_t *, const fb_entry *);
template __global__ void k_rewind<true>(rwd_shape, rwd_in, rwd_out, fb_params, const uint32_t *, const fb_entry *);
