// k_mpc.hip: kernels of the multi-party aggregation protocol (mpc_party.h, mpc_dealer.h).
#include <hip/hip_runtime.h>
#include "kernels.h"

using namespace bp;

// blocks [0, n_b): lane = slot (header, blindings, V row)  ||  lane = (slot, bit)
__global__ void __launch_bounds__(BP_BLOCK) k_mpc_commit1(uint32_t n_b, uint32_t nthreads, uint32_t n, uint32_t nslots, const uint32_t *slot_pos,
                                                           const uint64_t *values, const uint8_t *blindings, const uint8_t *rng, uint32_t *gsV,
                                                           uint32_t *gsAS, uint32_t *st1) {
    if (blockIdx.x < n_b) {
        const uint32_t s = blockIdx.x * BP_BLOCK + threadIdx.x;
        if (s < nslots) mpc_blind_thread(s, n, nslots, slot_pos, values, blindings, rng, gsV, gsAS, st1);
    } else {
        const uint32_t tid = (blockIdx.x - n_b) * BP_BLOCK + threadIdx.x;
        if (tid < nthreads) mpc_bits_thread(tid, n, nslots, slot_pos, values, rng, gsAS, st1);
    }
}

// the seeded twin (bpgpu_mpc_party_bit_commit_seeded): seeds [nslots][32], base [nslots] -- lane (slot, i) computes the keystream
// blocks of s_L[i] and s_R[i] itself, the slot lane those of a_blinding and s_blinding; padding slots return before any draw
__global__ void __launch_bounds__(BP_BLOCK) k_mpc_commit1_seeded(uint32_t n_b, uint32_t nthreads, uint32_t n, uint32_t nslots, const uint32_t *slot_pos,
                                                                  const uint64_t *values, const uint8_t *blindings, const uint8_t *seeds, const uint64_t *base,
                                                                  uint32_t *gsV, uint32_t *gsAS, uint32_t *st1) {
    const mpc_from_seed src{seeds, base};
    if (blockIdx.x < n_b) {
        const uint32_t s = blockIdx.x * BP_BLOCK + threadIdx.x;
        if (s < nslots) mpc_blind_lane(s, n, nslots, slot_pos, values, blindings, src, gsV, gsAS, st1);
    } else {
        const uint32_t tid = (blockIdx.x - n_b) * BP_BLOCK + threadIdx.x;
        if (tid < nthreads) mpc_bits_lane(tid, n, nslots, slot_pos, values, src, gsAS, st1);
    }
}

__global__ void __launch_bounds__(BP_BLOCK) k_mpc_poly(uint32_t n, uint32_t nslots, const uint32_t *slot_pos, const uint32_t *st1, const uint8_t *chal,
                                                        uint32_t chal_shared, const uint8_t *rng, uint32_t *st2, uint32_t *gsT, uint32_t *status) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nslots) mpc_poly_thread(s, n, nslots, slot_pos, st1, chal, chal_shared, rng, st2, gsT, status);
}
// the seeded twin (bpgpu_mpc_party_poly_commit_seeded): t_1_blinding, t_2_blinding are blocks base[s], base[s] + 1 of seeds[s]
__global__ void __launch_bounds__(BP_BLOCK) k_mpc_poly_seeded(uint32_t n, uint32_t nslots, const uint32_t *slot_pos, const uint32_t *st1, const uint8_t *chal,
                                                               uint32_t chal_shared, const uint8_t *seeds, const uint64_t *base, uint32_t *st2, uint32_t *gsT,
                                                               uint32_t *status) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nslots) mpc_poly_lane(s, n, nslots, slot_pos, st1, chal, chal_shared, mpc_from_seed{seeds, base}, st2, gsT, status);
}

__global__ void __launch_bounds__(BP_BLOCK) k_mpc_share(uint32_t nrows, uint32_t n, const uint32_t *st2, const uint8_t *xs, uint32_t x_shared, uint32_t *shares,
                                                         uint8_t *status) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < nrows) mpc_share_thread(r, n, st2, xs, x_shared, shares, status);
}

// The per-position table walk.  MSM rows are [kind][slot] (nrows = kinds * nslots, nslots a multiple of the wavefront): the 64 lanes
// of a block are 64 consecutive slots of ONE position, blk_pos[block of slots], and read that position's id list -- row blk_pos of
// ids_tab [party_capacity][ids_stride].  Everything else is k_fb_accum / k_fb_accum_ct: lane = MSM row, the pair range cut into
// nsplit partial sums.  Padding slots leave the identity.
__global__ void __launch_bounds__(FB_BLOCK) k_mpc_accum(fb_params prm, uint32_t nrows, uint32_t nslots, uint32_t nsplit, uint32_t npairs, const uint32_t *ids_tab,
                                                         uint32_t ids_stride, const uint32_t *blk_pos, const uint32_t *slot_pos, const fb_digit *digits,
                                                         const fb_entry *table, ge_ext *partial) {
    const uint32_t nblk_p = nrows / FB_BLOCK, nblk_s = nslots / FB_BLOCK;
    const uint32_t pblk = blockIdx.x % nblk_p, split = blockIdx.x / nblk_p, sblk = pblk % nblk_s;
    const uint32_t p = pblk * FB_BLOCK + threadIdx.x;
    const uint32_t per = (npairs + nsplit - 1) / nsplit;
    const uint32_t q0 = split * per, q1 = (q0 + per < npairs) ? q0 + per : npairs;
    if (slot_pos[sblk * FB_BLOCK + threadIdx.x] == MPC_NO_ROW) {
        ge_ext id;
        ge_identity(id);
        partial[(uint64_t)split * nrows + p] = id;
        return;
    }
    fb_accum_thread(p, split, q0 < npairs ? q0 : npairs, q1, prm, nrows, ids_tab + (uint64_t)blk_pos[sblk] * ids_stride, digits, table, partial);
}
// the constant-time twin (fb_accum_ct_thread: all 8 entries read, mask select, always add)
__global__ void __launch_bounds__(FB_BLOCK) k_mpc_accum_ct(fb_params prm, uint32_t nrows, uint32_t nslots, uint32_t nsplit, uint32_t npairs,
                                                            const uint32_t *__restrict__ ids_tab, uint32_t ids_stride, const uint32_t *__restrict__ blk_pos,
                                                            const uint32_t *__restrict__ slot_pos, const fb_digit *__restrict__ digits,
                                                            const fb_entry *__restrict__ table, ge_ext *__restrict__ partial) {
    const uint32_t nblk_p = nrows / FB_BLOCK, nblk_s = nslots / FB_BLOCK;
    const uint32_t pblk = blockIdx.x % nblk_p, split = blockIdx.x / nblk_p, sblk = pblk % nblk_s;
    const uint32_t p = pblk * FB_BLOCK + threadIdx.x;
    const uint32_t per = (npairs + nsplit - 1) / nsplit;
    const uint32_t q0 = split * per, q1 = (q0 + per < npairs) ? q0 + per : npairs;
    if (slot_pos[sblk * FB_BLOCK + threadIdx.x] == MPC_NO_ROW) {   // (public: which slots are padding follows from the positions)
        ge_ext id;
        ge_identity(id);
        partial[(uint64_t)split * nrows + p] = id;
        return;
    }
    fb_accum_ct_thread(p, split, q0 < npairs ? q0 : npairs, q1, prm, nrows, ids_tab + (uint64_t)blk_pos[sblk] * ids_stride, digits, table, partial);
}

// the dealer's point sums: lane = (session, column)
__global__ void __launch_bounds__(BP_BLOCK) k_mpc_ptsum(uint32_t nthreads, uint32_t m, uint32_t ncol, uint32_t rec, uint32_t off, const uint8_t *in, uint32_t *out,
                                                         uint32_t *status) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid < nthreads) mpc_ptsum_thread(tid, m, ncol, rec, off, in, out, status);
}

__global__ void __launch_bounds__(BP_BLOCK) k_mpc_vectors(uint32_t nthreads, uint32_t n, uint32_t m, const uint8_t *shares, const uint32_t *yinv, const uint8_t *skip,
                                                           uint32_t *a_vec, uint32_t *b_vec, uint32_t *Gf, uint32_t *Hf) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid < nthreads) mpc_vectors_thread(tid, n, m, shares, yinv, skip, a_vec, b_vec, Gf, Hf);
}
