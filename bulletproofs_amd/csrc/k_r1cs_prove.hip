// k_r1cs_prove.hip: HIP kernels of libbpgpu.so (gfx950) for R1CS proof creation; thin __global__ wrappers around r1cs_prover.h.
#include <hip/hip_runtime.h>
#include "kernels.h"

using namespace bp;

// lane = (proof, committed index), then (proof, free index)
__global__ void __launch_bounds__(64) k_r1p_inputs(uint32_t nthreads, r1p_shape sh, const uint8_t *v, const uint8_t *vb, const uint8_t *freev,
                                                    uint32_t *vrows, uint32_t *status) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid < nthreads) r1p_inputs_thread(tid, sh, v, vb, freev, vrows, status);
}

// 32 lanes per proof, two proofs per workgroup; each group's sponge state in LDS
__global__ void __launch_bounds__(64) k_r1p_rng(r1p_shape sh, uint32_t *ts, const uint32_t *vout, const uint8_t *vb, const uint8_t *rng32, uint32_t *rnd) {
    __shared__ uint32_t lds[2 * 50];
    const uint32_t g = threadIdx.x >> 5;
#if defined(__HIP_DEVICE_COMPILE__)   // (the cooperative permutation is device code only)
    r1p_rng_coop(blockIdx.x * 2 + g, threadIdx.x, lds + 50 * g, sh, ts, vout, vb, rng32, rnd);
#endif
}

// lane = proof
__global__ void __launch_bounds__(64) k_r1p_witness(r1p_shape sh, const uint32_t *src_l, const uint32_t *src_r, const uint32_t *row_ptr, const r1p_term *terms,
                                                     const uint8_t *v, const uint8_t *freev, const uint32_t *fields, uint32_t *aw) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < sh.c.nproofs) r1p_witness_thread(p, sh, src_l, src_r, row_ptr, terms, v, freev, fields, aw);
}

// lane = (proof, multiplier of the phase)
__global__ void __launch_bounds__(64) k_r1p_rows(uint32_t nthreads, r1p_shape sh, uint32_t cnt, uint32_t b0, const uint32_t *aw, const uint32_t *rnd, uint32_t *rows) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid < nthreads) r1p_rows_thread(tid, sh, cnt, b0, aw, rnd, rows);
}

// lane = proof; the 50-word sponge state in LDS, word-major (as k_r1cs_front)
__global__ void __launch_bounds__(RP_BLOCK) k_r1p_chal1(r1p_shape sh, const uint32_t *mout, const uint32_t *lbl_off, const uint8_t *lbl, uint32_t *ts,
                                                         uint32_t *fields, uint32_t *recs) {
    __shared__ uint32_t lds[50 * RP_BLOCK];
    const uint32_t p = blockIdx.x * RP_BLOCK + threadIdx.x;
    kstate st;
    st.w = lds + threadIdx.x;
    st.stride = RP_BLOCK;
    if (p < sh.c.nproofs) r1p_chal1_thread(p, sh, st, mout, lbl_off, lbl, ts, fields, recs);
}
__global__ void __launch_bounds__(RP_BLOCK) k_r1p_chal2(r1p_shape sh, const uint32_t *mout, uint32_t *ts, uint32_t *fields, uint32_t *recs) {
    __shared__ uint32_t lds[50 * RP_BLOCK];
    const uint32_t p = blockIdx.x * RP_BLOCK + threadIdx.x;
    kstate st;
    st.w = lds + threadIdx.x;
    st.stride = RP_BLOCK;
    if (p < sh.c.nproofs) r1p_chal2_thread(p, sh, st, mout, ts, fields, recs);
}
__global__ void __launch_bounds__(RP_BLOCK) k_r1p_chal3(r1p_shape sh, const uint32_t *tout, const uint32_t *rnd, uint32_t *ts, uint32_t *fields, uint32_t *recs,
                                                         uint32_t *wout) {
    __shared__ uint32_t lds[50 * RP_BLOCK];
    const uint32_t p = blockIdx.x * RP_BLOCK + threadIdx.x;
    kstate st;
    st.w = lds + threadIdx.x;
    st.stride = RP_BLOCK;
    if (p < sh.c.nproofs) r1p_chal3_thread(p, sh, st, tout, rnd, ts, fields, recs, wout);
}

// lane = (column, proof), proof fastest
__global__ void __launch_bounds__(64) k_r1p_poly(uint32_t nthreads, r1p_shape sh, const uint32_t *col_ptr, const r1cs_ent *ents, const uint32_t *aw,
                                                  const uint32_t *rnd, const uint8_t *vb, const uint32_t *fields, uint32_t nrow, uint32_t *vecs, uint32_t *terms) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid < nthreads) r1p_poly_thread(tid, sh, col_ptr, ents, aw, rnd, vb, fields, nrow, vecs, terms);
}

// 64 lanes summing fields [f0, f0 + cnt) of proof p (a strided share each, then a tree in LDS)
__device__ void r1p_block_sum(sc &out, uint32_t *part, uint32_t nproofs, const uint32_t *terms, uint32_t f0, uint32_t cnt, uint32_t p) {
    const uint32_t l = threadIdx.x;
    sc acc, t;
    sc_0(acc);
    for (uint32_t i = l; i < cnt; i += 64) {
        rp_load(t, terms, nproofs, f0 + i, p);
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

// one workgroup of 64 lanes per proof: t1..t6 and <wV, v~>; lane 0 writes the T rows
__global__ void __launch_bounds__(64) k_r1p_tsum(r1p_shape sh, uint32_t nrow, const uint32_t *terms, const uint32_t *rnd, uint32_t *fields, uint32_t *trows) {
    __shared__ uint32_t part[64 * 8];
    const uint32_t p = blockIdx.x;
    sc sums[7];
#pragma unroll
    for (uint32_t s = 0; s < 7; s++) r1p_block_sum(sums[s], part, sh.c.nproofs, terms, s * nrow, s < 6 ? sh.c.n : sh.c.m, p);
    if (threadIdx.x == 0) r1p_trows_lead(p, sh, sums, rnd, fields, trows);
}

// lane = (proof, i) over padded_n
__global__ void __launch_bounds__(64) k_r1p_vecs(uint32_t nthreads, r1p_shape sh, const uint32_t *fields, const uint32_t *vecs, uint32_t *lv, uint32_t *rv,
                                                  uint32_t *gf, uint32_t *hf) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid < nthreads) r1p_vecs_thread(tid, sh, fields, vecs, lv, rv, gf, hf);
}
