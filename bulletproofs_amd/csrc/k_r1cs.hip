// k_r1cs.hip: HIP kernels of libbpgpu.so (gfx950) for R1CS proof verification; thin __global__ wrappers around r1cs.h.
#include <hip/hip_runtime.h>
#include "kernels.h"

using namespace bp;

// lane = proof; the 50-word sponge state in LDS, word-major (as k_ipp_vs_front)
__global__ void __launch_bounds__(RP_BLOCK) k_r1cs_front(r1cs_shape sh, rp_strobe_init init, const uint8_t *proofs, const uint32_t *proof_lens,
                                                          const uint8_t *commitments, const uint32_t *ts_in, const uint8_t *rng32, const uint32_t *lbl_off,
                                                          const uint8_t *lbl, uint32_t *fields, uint32_t *uniq_sc, uint32_t *uniq_pt, uint32_t *ts_out,
                                                          uint32_t *status) {
    __shared__ uint32_t lds[50 * RP_BLOCK];
    const uint32_t p = blockIdx.x * RP_BLOCK + threadIdx.x;
    kstate st;
    st.w = lds + threadIdx.x;
    st.stride = RP_BLOCK;
    if (p < sh.nproofs)
        r1cs_front_thread(p, sh, init, st, proofs, proof_lens, commitments, ts_in, rng32, lbl_off, lbl, fields, uniq_sc, uniq_pt, ts_out, status);
}

// lane = (column, proof), proof fastest
__global__ void __launch_bounds__(64) k_r1cs_flatten(uint32_t nthreads, r1cs_shape sh, const uint32_t *col_ptr, const r1cs_ent *ents, const uint32_t *status,
                                                      uint32_t *fields, uint32_t *gen_sc, uint32_t *uniq_sc, uint32_t *dterm) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid < nthreads) r1cs_flatten_thread(tid, sh, col_ptr, ents, status, fields, gen_sc, uniq_sc, dterm);
}

// 64 lanes summing rows [r0, r1) of dterm for proof p (a strided share each, then a tree in LDS); the sum lands in part[0..8)
__device__ void r1_block_sum(sc &out, uint32_t *part, const r1cs_shape &sh, const uint32_t *dterm, uint32_t r0, uint32_t r1, uint32_t p) {
    const uint32_t l = threadIdx.x;
    sc acc, t;
    sc_0(acc);
    for (uint32_t i = r0 + l; i < r1; i += 64) {
        const uint32_t *src = dterm + ((uint64_t)i * sh.nproofs + p) * 8;
#pragma unroll
        for (int q = 0; q < 8; q++) t.v[q] = src[q];
        sc_add(acc, acc, t);
    }
#pragma unroll
    for (int q = 0; q < 8; q++) part[l * 8 + q] = acc.v[q];
    __syncthreads();
    for (uint32_t h = 32; h > 0; h >>= 1) {
        if (l < h) {
#pragma unroll
            for (int q = 0; q < 8; q++) {
                acc.v[q] = part[l * 8 + q];
                t.v[q] = part[(l + h) * 8 + q];
            }
            sc_add(acc, acc, t);
#pragma unroll
            for (int q = 0; q < 8; q++) part[l * 8 + q] = acc.v[q];
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < 8; q++) out.v[q] = part[q];
    __syncthreads();
}

// one workgroup of 64 lanes per proof: delta = sum of rows [0, pn), wc = sum of rows [pn, pn + one_chunks); lane 0 forms the two
// basepoint coefficients
__global__ void __launch_bounds__(64) k_r1cs_finish(r1cs_shape sh, const uint32_t *status, const uint32_t *dterm, const uint32_t *fields, uint32_t *gen_sc) {
    __shared__ uint32_t part[64 * 8];
    const uint32_t p = blockIdx.x;
    if (status[p] != 0) return;   // (uniform across the workgroup)
    sc delta, wc;
    r1_block_sum(delta, part, sh, dterm, 0, sh.pn, p);
    r1_block_sum(wc, part, sh, dterm, sh.pn, sh.pn + sh.one_chunks, p);
    if (threadIdx.x == 0) r1_finish_lead(p, sh, delta, wc, fields, gen_sc);
}
