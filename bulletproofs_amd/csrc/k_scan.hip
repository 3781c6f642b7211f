// k_scan.hip: scanning range proofs under many keys (scan.h): key prefixes, one replay per row, the candidate test per (row, key), the open.
// The open is capped at 168 registers (three wavefronts per SIMD) like k_rewind, whose two phases it shares.
#include <hip/hip_runtime.h>
#include "kernels.h"

using namespace bp;

// lane = key: at most SCN_MAX_KEYS lanes, once per call
__global__ void __launch_bounds__(BP_BLOCK) k_scan_prefix(scn_keys k, scn_ws ws) {
    __shared__ __align__(16) uint32_t lds[50 * BP_BLOCK];
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k.nkeys) return;
    const kstate st = {lds + threadIdx.x, BP_BLOCK};
    scn_prefix_lane(j, k, ws, st);
}

// lane = row: the replay, once per row
__global__ void __launch_bounds__(BP_BLOCK) k_scan_replay(rwd_shape sh, rwd_in in, scn_ws ws) {
    __shared__ __align__(16) uint32_t lds[50 * BP_BLOCK];
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= sh.nproofs) return;
    const kstate st = {lds + threadIdx.x, BP_BLOCK};
    scn_replay_lane(p, sh, in, ws, st);
}

// lane = (row, key): blockIdx.y is the key, so a workgroup's 50 prefix words are uniform loads and x, e_blinding and C are read along
// the rows.  CT: every lane of a replayed row sends its atomicMin; otherwise only a survivor does (almost none).
template <bool CT>
__global__ void __launch_bounds__(BP_BLOCK) k_scan_cand(rwd_shape sh, rwd_in in, scn_ws ws) {
    __shared__ __align__(16) uint32_t lds[50 * BP_BLOCK];
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (p >= sh.nproofs) return;
    if (ws.status[p] != RWD_OK) return;   // (public)
    const kstate st = {lds + threadIdx.x, BP_BLOCK};
    const uint32_t c = scn_cand_lane(p, j, sh, in, ws, st);
    if (CT || c != SCN_NONE) atomicMin(ws.jstar + p, c);
}
template __global__ void k_scan_cand<false>(rwd_shape, rwd_in, scn_ws);
template __global__ void k_scan_cand<true>(rwd_shape, rwd_in, scn_ws);

// lane = row: k_rewind's shape -- the scalars in the lane's sponge words, the barrier, the walk parked over the same words.  A lane
// past the batch only waits at the barrier.
template <bool CT>
__global__ void __launch_bounds__(BP_BLOCK, 3) k_scan_open(rwd_shape sh, rwd_in in, scn_keys k, scn_ws ws, rwd_out out, uint32_t *key_index, fb_params prm,
                                                           const uint32_t *gen_ids, const fb_entry *table) {
    static_assert(sizeof(ge_ext) == 40 * sizeof(uint32_t), "the points fill rows 10 .. 49");
    __shared__ __align__(16) uint32_t lds[50 * BP_BLOCK];
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = p < sh.nproofs;
    uint32_t stat = RWD_NOT_FOUND, jstar = SCN_NONE;
    if (live) {
        const kstate st = {lds + threadIdx.x, BP_BLOCK};
        stat = scn_open_scalars<CT>(p, sh, in, k, ws, out, st, jstar);
    }
    __syncthreads();
    if (!live) return;   // (behind the barrier, as in k_rewind)
    const ped_park pk = {lds + threadIdx.x, BP_BLOCK, (ge_ext *)(lds + 10 * BP_BLOCK) + threadIdx.x};
    scn_open_check<CT>(p, in, out, key_index, stat, jstar, pk, prm, gen_ids, table);
}
template __global__ void k_scan_open<false>(rwd_shape, rwd_in, scn_keys, scn_ws, rwd_out, uint32_t *, fb_params, const uint32_t *, const fb_entry *);
template __global__ void k_scan_open<true>(rwd_shape, rwd_in, scn_keys, scn_ws, rwd_out, uint32_t *, fb_params, const uint32_t *, const fb_entry *);
