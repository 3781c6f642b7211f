// Host harness for the seeded range-proof prover: rp_prover.h's rpp_draw, the three lane bodies that consume random scalars
// (rpp_blind_lane, rpp_bits_lane, rpp_tcommit_lane) under either draw source, and the separator-applying start of the first transcript
// lane (rpp_chal1_lane<true>), compiled with g++ and driven lane by lane, the way k_rpp_commit1(_seed) / k_rpp_tcommit(_seed) /
// k_rpp_chal1_sep run them.  TEST-ONLY: never part of libbpgpu.so, never a fallback.
#define BP_FE_CHECK 1
#include "../../bulletproofs_amd/csrc/rp_prover.h"
using namespace bp;

extern "C" void rppseed_draw(const uint8_t *seed32, uint64_t d, uint32_t *out8) {
    sc r;
    rpp_draw(r, seed32, d);
    for (int q = 0; q < 8; q++) out8[q] = r.v[q];
}

// a draw source that counts the requests for an index at or past D = m (2n + 2) + 2m
template <class Src>
struct counted {
    Src src;
    uint32_t D;
    uint32_t *bad;
    void draw(sc &r, const rpp_shape &sh, uint32_t p, uint32_t d) const {
        if (d >= D || p >= sh.nproofs) {
            ++*bad;
            sc_0(r);
            return;
        }
        src.draw(r, sh, p, d);
    }
};

static rpp_shape shape_of(uint32_t n, uint32_t m, uint32_t nproofs) {
    rpp_shape sh;
    sh.n = n, sh.m = m, sh.nm = n * m, sh.k = 0;
    while ((1u << sh.k) < sh.nm) sh.k++;
    sh.nproofs = nproofs;
    sh.proof_len = 32 * (9 + 2 * sh.k);
    sh.n_gen_terms = 2 * sh.nm + 2;
    sh.rng_per_proof = 64 * (m * (2 * n + 2) + 2 * m);
    return sh;
}

template <class Src>
static void run_role(int role, const rpp_shape &sh, const Src &src, const uint64_t *values, const uint8_t *blindings, uint32_t *gen_scalars, uint32_t *sL,
                     uint32_t *sR, uint32_t *party) {
    if (role == 0)
        for (uint32_t p = 0; p < sh.nproofs; p++) rpp_blind_lane(p, sh, values, blindings, src, gen_scalars, party);
    else if (role == 1)
        for (uint32_t tid = 0; tid < sh.nproofs * sh.nm; tid++) rpp_bits_lane(tid, sh, values, src, gen_scalars, sL, sR);
    else
        for (uint32_t p = 0; p < sh.nproofs; p++) rpp_tcommit_lane(p, sh, src, gen_scalars, party);
}

// every lane of one role (0: blind, 1: bits, 2: tcommit).  seeded: `randomness` holds 32 bytes per proof, else rng_per_proof bytes per proof.
// Returns the number of draws a lane asked for at an index >= D.
extern "C" int rppseed_role(int role, int seeded, uint32_t n, uint32_t m, uint32_t nproofs, const uint64_t *values, const uint8_t *blindings,
                            const uint8_t *randomness, uint32_t *gen_scalars, uint32_t *sL, uint32_t *sR, uint32_t *party) {
    const rpp_shape sh = shape_of(n, m, nproofs);
    uint32_t bad = 0;
    const uint32_t D = m * (2 * n + 2) + 2 * m;
    if (seeded) run_role(role, sh, counted<rpp_from_seed>{rpp_from_seed{randomness}, D, &bad}, values, blindings, gen_scalars, sL, sR, party);
    else run_role(role, sh, counted<rpp_from_bytes>{rpp_from_bytes{randomness}, D, &bad}, values, blindings, gen_scalars, sL, sR, party);
    return (int)bad;
}

// the buffer-fed wrappers the existing kernels call: the same arrays through rpp_blind_thread / rpp_bits_thread / rpp_tcommit_thread
extern "C" void rppseed_role_legacy(int role, uint32_t n, uint32_t m, uint32_t nproofs, const uint64_t *values, const uint8_t *blindings, const uint8_t *rng,
                                    uint32_t *gen_scalars, uint32_t *sL, uint32_t *sR, uint32_t *party) {
    const rpp_shape sh = shape_of(n, m, nproofs);
    if (role == 0)
        for (uint32_t p = 0; p < nproofs; p++) rpp_blind_thread(p, sh, values, blindings, rng, gen_scalars, party);
    else if (role == 1)
        for (uint32_t tid = 0; tid < nproofs * sh.nm; tid++) rpp_bits_thread(tid, sh, values, rng, gen_scalars, sL, sR);
    else
        for (uint32_t p = 0; p < nproofs; p++) rpp_tcommit_thread(p, sh, rng, gen_scalars, party);
}

// the first transcript lane of every proof, starting from un-separated states (ts_in_stride in words: 0 or 52); msm_out: rows 2p = A,
// 2p + 1 = S, 2 nproofs + p m + j = V_j.  ts: [proof][52] words out, fields: [RPP_FIXED][proof][8]
extern "C" void rppseed_chal1_sep(uint32_t n, uint32_t m, uint32_t nproofs, const uint32_t *msm_out, const uint32_t *ts_in, uint32_t ts_in_stride, uint32_t *ts,
                                  uint32_t *fields, uint8_t *proofs, uint8_t *commitments) {
    const rpp_shape sh = shape_of(n, m, nproofs);
    for (uint32_t p = 0; p < nproofs; p++) {
        uint32_t w[50];
        kstate st;
        st.w = w, st.stride = 1;
        rpp_chal1_lane<true>(p, sh, st, msm_out, ts_in, ts_in_stride, ts, fields, proofs, commitments);
    }
}
