// Rewinding range proofs: value, message and blinding of a commitment back out of its proof, given the seed the proof was made from
// (include/bpgpu.h, bpgpu_rangeproof_rewind_batch).  The rewindable prover (rp_prover.h, rpp_from_seed_rw) is the seeded prover with
//     a_blinding = d_0 - e  (mod l),   e = v + 2^64 msg < 2^192,   d_k = draw k of the proof's seed  (m = 1),
// so that with the proof's own challenges x and z
//     e     = d_0 + d_1 x - e_blinding                                   (e_blinding = a_blinding + s_blinding x)
//     gamma = (t_x_blinding - x (d_{2n+2} + x d_{2n+3})) z^-2            (t_x_blinding = z^2 gamma + x (t_1_blinding + x t_2_blinding))
// and the row is the holder's own iff e < 2^192 and compress((e mod 2^64) B + gamma B_blinding) == V.  Nothing here verifies the proof.
//
// Lane = row, ONE launch in three phases (k_rewind.hip):
//   rwd_replay   the transcript up to x with the sponge in the lane's 50 LDS words: rangeproof_domain_sep(n, 1), V, A, S -> y, z,
//                T_1, T_2 -> x.  The five scalars of the proof are checked first (RangeProof::from_bytes: FORMAT); A, S, T_1 or T_2 of
//                32 zero bytes stops the replay (NOT_FOUND).
//   rwd_scalars  the four draws (one ChaCha block each, in the lane), e, the test e < 2^192, gamma (z is public: its inversion is the
//                variable-time one).  The candidate (v, msg, gamma) goes to the row's OUTPUT words; nothing but the status crosses the
//                barrier in registers.
//   rwd_check    behind a workgroup barrier, over the same LDS words (pedersen.h ped_park): gamma on B_blinding, the u64 value on B with
//                its short window count, ped_encode, the compare with V; a row that fails gets its output words zeroed again.
// Variable-time form: a row that is already rejected computes no gamma and skips the walk (a scan is almost all such rows: whole
// wavefronts skip it).  CT form (context option "prover_constant_time"): every row computes gamma and walks with ped_walk_ct, a row
// rejected by the parse or the replay (public) walks zeros, and nothing branches on e: the 2^192 test and the compare fold into masks.
#ifndef BPGPU_REWIND_H
#define BPGPU_REWIND_H
#include "opening.h"

namespace bp {

#define RWD_OK 0u          // BPGPU_REWIND_OK
#define RWD_NOT_FOUND 1u   // BPGPU_REWIND_NOT_FOUND
#define RWD_FORMAT 2u      // BPGPU_REWIND_FORMAT
#define RWD_MAX_BATCH (1u << 26)

struct rwd_shape {
    uint32_t n, k;           // bits per value, k = lg n (m = 1)
    uint32_t nproofs;
    uint32_t proof_words;    // 8 * (9 + 2 k)
    uint32_t ts_in_stride;   // words between the callers' states (0: one state for every row)
};
struct rwd_in {
    const uint32_t *proofs;        // [row][proof_words]
    const uint32_t *commitments;   // [row][8]
    const uint8_t *seeds;          // [row][32]
    const uint32_t *ts_in;         // the callers' states before rangeproof_domain_sep, never null
};
struct rwd_out {
    uint8_t *status;       // [row]
    uint32_t *values;      // [row][2]: the u64 value
    uint32_t *messages;    // [row][4]
    uint32_t *blindings;   // [row][8]
};

// Phase 1: parse and replay.  Returns RWD_FORMAT, RWD_NOT_FOUND or 0 (x and z are set).  The messages are absorbed from global memory
// (the absorb loop indexes its message: a copy in registers would go to scratch, as in opn_front_lane).
BP_HD uint32_t rwd_replay(uint32_t p, const rwd_shape &sh, const rwd_in &in, kstate st, sc &x, sc &z) {
    const uint32_t *pr = in.proofs + (uint64_t)p * sh.proof_words;
    {   // from_bytes: t_x, t_x_blinding, e_blinding, a, b canonical
        bool fmt_ok = true;
#pragma unroll 1
        for (uint32_t f = 0; f < 5; f++) {
            const uint32_t *s = pr + (f < 3 ? 32 + 8 * f : 56 + 16 * sh.k + 8 * (f - 3));
            uint32_t w[8];
#pragma unroll
            for (int q = 0; q < 8; q++) w[q] = s[q];
            fmt_ok = fmt_ok & sc_is_canonical(w);
        }
        if (!fmt_ok) return RWD_FORMAT;
    }
    strobe t;
    opn_ts_load(t, st, p, nullptr, in.ts_in, sh.ts_in_stride);
    const uint8_t dsep[7] = {'d', 'o', 'm', '-', 's', 'e', 'p'}, l_n[1] = {'n'}, l_m[1] = {'m'};
    const uint8_t rpv1[13] = {'r', 'a', 'n', 'g', 'e', 'p', 'r', 'o', 'o', 'f', ' ', 'v', '1'};
    merlin_append_message(t, dsep, 7, rpv1, 13);
    merlin_append_u64(t, l_n, 1, sh.n);
    merlin_append_u64(t, l_m, 1, 1);
    const uint8_t lV[1] = {'V'}, lA[1] = {'A'}, lS[1] = {'S'}, ly[1] = {'y'}, lz[1] = {'z'}, lx[1] = {'x'};
    const uint8_t lT1[3] = {'T', '_', '1'}, lT2[3] = {'T', '_', '2'};
    merlin_append_words8(t, lV, 1, in.commitments + 8 * (uint64_t)p);
    uint32_t w[8];
#pragma unroll
    for (int q = 0; q < 8; q++) w[q] = pr[q];
    if (words8_zero(w)) return RWD_NOT_FOUND;
    merlin_append_words8(t, lA, 1, pr);
#pragma unroll
    for (int q = 0; q < 8; q++) w[q] = pr[8 + q];
    if (words8_zero(w)) return RWD_NOT_FOUND;
    merlin_append_words8(t, lS, 1, pr + 8);
    rp_challenge_scalar(t, ly, 1, z);   // y: squeezed and dropped
    rp_challenge_scalar(t, lz, 1, z);
#pragma unroll
    for (int q = 0; q < 8; q++) w[q] = pr[16 + q];
    if (words8_zero(w)) return RWD_NOT_FOUND;
    merlin_append_words8(t, lT1, 3, pr + 16);
#pragma unroll
    for (int q = 0; q < 8; q++) w[q] = pr[24 + q];
    if (words8_zero(w)) return RWD_NOT_FOUND;
    merlin_append_words8(t, lT2, 3, pr + 24);
    rp_challenge_scalar(t, lx, 1, x);
    return RWD_OK;
}

// Phase 2: e and gamma.  The candidate goes to the row's output words (zeros for a row that is rejected already); only a live lane
// stores.  Returns the status so far.
template <bool CT>
BP_HD uint32_t rwd_scalars(uint32_t p, bool live, const rwd_shape &sh, const rwd_in &in, const rwd_out &out, uint32_t stat, const sc &x, const sc &z) {
    const uint32_t *pr = in.proofs + (uint64_t)p * sh.proof_words;
    const uint8_t *seed = in.seeds + 32 * (uint64_t)p;
    sc e, g;
    sc_0(e);
    sc_0(g);
    bool cand = stat == RWD_OK;   // (public: the parse and the replay look at the proof alone)
    if (cand) {
        sc a, b;
        rpp_draw(b, seed, 1);
        sc_mul(b, b, x);
        rpp_draw(a, seed, 0);
        sc_add(a, a, b);
#pragma unroll
        for (int q = 0; q < 8; q++) b.v[q] = pr[48 + q];
        sc_sub(e, a, b);   // d_0 + d_1 x - e_blinding
        const bool small = (e.v[6] | e.v[7]) == 0;
        if (CT) stat = small ? RWD_OK : RWD_NOT_FOUND;
        else if (!small) stat = RWD_NOT_FOUND, cand = false;
    }
    if (cand) {
        sc a, b;
        rpp_draw(b, seed, 2 * (uint64_t)sh.n + 3);
        sc_mul(b, b, x);
        rpp_draw(a, seed, 2 * (uint64_t)sh.n + 2);
        sc_add(a, a, b);
        sc_mul(a, a, x);
#pragma unroll
        for (int q = 0; q < 8; q++) b.v[q] = pr[40 + q];
        sc_sub(a, b, a);   // t_x_blinding - x (t_1_blinding + x t_2_blinding)
        sc_mul(b, z, z);
        sc_invert_safegcd_var(b, b);
        sc_mul(g, a, b);
    }
    if (live) {
        const uint32_t keep = cand ? 0xffffffffu : 0u;   // (a rejected row of the variable-time form holds a stale e)
        out.values[2 * (uint64_t)p] = e.v[0] & keep;
        out.values[2 * (uint64_t)p + 1] = e.v[1] & keep;
#pragma unroll
        for (int q = 0; q < 4; q++) out.messages[4 * (uint64_t)p + q] = e.v[2 + q] & keep;
#pragma unroll
        for (int q = 0; q < 8; q++) out.blindings[8 * (uint64_t)p + q] = g.v[q];
    }
    return stat;
}

// Phase 3, live lanes only: compress(v B + gamma B_blinding) against V.  pk lies over the sponge of phase 1: every lane of the workgroup has left that
// phase.  gen_ids: [0] = B_blinding, [1] = B.  CT: table and prm are the W = 4 set.  The scalars are read back from the output words,
// each when its walk begins; the row's output words are rewritten under the final status (all zero unless it is RWD_OK), which is
// returned (scan.h derives the row's key index from it).
template <bool CT>
BP_HD uint32_t rwd_check(uint32_t p, const rwd_in &in, const rwd_out &out, uint32_t stat, const ped_park &pk, fb_params prm, const uint32_t *gen_ids,
                     const fb_entry *table) {
    if (CT || stat == RWD_OK) {
        ge_ext acc;
        ge_identity(acc);
        bool started = false;
#pragma unroll 1
        for (uint32_t term = 0; term < 2; term++) {
            uint32_t s[8];
#pragma unroll
            for (int q = 0; q < 8; q++) s[q] = 0;
            if (term == 0) {
#pragma unroll
                for (int q = 0; q < 8; q++) s[q] = out.blindings[8 * (uint64_t)p + q];
            } else {
                s[0] = out.values[2 * (uint64_t)p];
                s[1] = out.values[2 * (uint64_t)p + 1];
            }
            const uint32_t nw = term == 0 ? prm.nwin : ped_u64_windows(prm);
            if (CT) ped_walk_ct(acc, pk, s, nw, gen_ids[term], prm, table);
            else ped_walk(acc, started, pk, s, nw, gen_ids[term], prm, table);
        }
        uint32_t w[8];
        ped_encode(w, acc, pk);
        uint32_t diff = 0;
#pragma unroll
        for (int q = 0; q < 8; q++) diff |= w[q] ^ in.commitments[8 * (uint64_t)p + q];
        stat = stat != RWD_OK ? stat : (diff ? RWD_NOT_FOUND : RWD_OK);
        const uint32_t keep = stat == RWD_OK ? 0xffffffffu : 0u;
        out.values[2 * (uint64_t)p] &= keep;
        out.values[2 * (uint64_t)p + 1] &= keep;
#pragma unroll
        for (int q = 0; q < 4; q++) out.messages[4 * (uint64_t)p + q] &= keep;
#pragma unroll
        for (int q = 0; q < 8; q++) out.blindings[8 * (uint64_t)p + q] &= keep;
    }
    out.status[p] = (uint8_t)stat;
    return stat;
}

}  // namespace bp
#endif
