// Proofs of knowledge of commitment openings, in batches: a sigma protocol over C = v B + r B_blinding (include/bpgpu.h,
// bpgpu_opening_*).  Two forms, one per call:
//   OPN_FULL     (0): v and r secret.  proof = R | s_v | s_r (96 bytes),  R = k_v B + k_r B_blinding, s_v = k_v + c v, s_r = k_r + c r
//   OPN_BLINDING (1): v public, r secret.  proof = R | s_r (64 bytes),    R = k_r B_blinding,         s_r = k_r + c r ; the verifier
//                     computes s_v = c v itself.  With v = 0: a Schnorr signature under the key C on base B_blinding (an excess proof).
// The check of both: s_v B + s_r B_blinding - c C - R = identity.
// Transcript, on the caller's own state at any STROBE position (opn_bind, opn_challenge):
//   append_message("dom-sep", "openingproof v1"); append_u64("form", form); append_point("C", C); form 1: append_scalar("v", v);
//   validate_and_append_point("R", R)  [32 zero bytes: VerificationError, nothing of R absorbed];  c = challenge_scalar("c")
//
// Lane = proof everywhere.  The prover is ONE launch in two phases around a workgroup barrier: opn_create_walk (draw the nonces, walk the
// window tables of B_blinding and B through pedersen.h's ped_walk / ped_walk_ct, ped_encode: R) and opn_create_finish (the transcript
// with its sponge in the LDS words that parked the walk's scalar and point, the two multiply-adds, the stores).  Nothing is carried across
// the barrier but R: the finish reads v and r, checks them (sc_is_canonical) and draws the nonces again (one ChaCha block each).
// The verifier's front end (opn_front_lane) replays the transcript and stages the row for the multiscalar multiplication: unique terms
// (-c, C), (-1, R) and the row (s_r, s_v, 0) of generator-table coefficients (B_blinding, B, G_0); no point is decoded here.
#ifndef BPGPU_OPENING_H
#define BPGPU_OPENING_H
#include "pedersen.h"
#include "ipp.h"
#include "rlc_comb.h"

namespace bp {

#define OPN_FULL 0u
#define OPN_BLINDING 1u
#define OPN_RLC_WEIGHT_DOMAIN 0x6e706f77u   // "wopn": the combination weights the caller did not bring
#define OPN_RLC_MAX_PROOFS (1u << 23)       // 2 unique terms per proof, 2^24 of them in one combination
#define OPN_GEN_ROW 3u                      // a row of generator-table scalars: B_blinding, B, G_0 (always 0)

struct opn_shape {
    uint32_t form, nproofs;
    uint32_t value_words;    // 2: u64 values, 8: 32-byte scalars, 0: no value buffer (form 1: every value is 0)
    uint32_t ts_in_stride;   // words between the callers' states at ts_in (0: one state for every proof)
};

BP_HD uint32_t opn_proof_words(uint32_t form) { return form == OPN_FULL ? 24u : 16u; }

// proof p's value as 8 words (zero where there is no buffer)
BP_HD void opn_load_value(uint32_t p, const opn_shape &sh, const uint32_t *values, uint32_t v[8]) {
#pragma unroll
    for (int q = 0; q < 8; q++) v[q] = 0;
    if (sh.value_words == 2) {
        v[0] = values[2 * (uint64_t)p];
        v[1] = values[2 * (uint64_t)p + 1];
    } else if (sh.value_words == 8) {
#pragma unroll
        for (int q = 0; q < 8; q++) v[q] = values[8 * (uint64_t)p + q];
    }
}

// the caller's state of proof p (ts_in + p ts_in_stride words, or *init where ts_in is null) into the lane's sponge; a state whose
// position bytes are out of range (device memory, which the host cannot check) starts at position 0: never an index past the sponge
BP_HD void opn_ts_load(strobe &t, kstate st, uint32_t p, const rp_strobe_init *init, const uint32_t *ts_in, uint32_t ts_in_stride) {
    t.st = st;
    if (ts_in) {
        const uint32_t *src = ts_in + (uint64_t)p * ts_in_stride;
        for (uint32_t i = 0; i < 50; i++) ks_set32(st, i, src[i]);
        const uint32_t meta = src[50];
        t.pos = meta & 0xffu;
        t.pos_begin = (meta >> 8) & 0xffu;
        t.cur_flags = (meta >> 16) & 0xffu;
    } else {
        for (uint32_t i = 0; i < 50; i++) ks_set32(st, i, init->w[i]);
        t.pos = init->pos;
        t.pos_begin = init->pos_begin;
        t.cur_flags = init->cur_flags;
    }
    if (t.pos >= BP_STROBE_R || t.pos_begin > BP_STROBE_R) t.pos = t.pos_begin = 0;
}
// the separator, the form, C and (form 1) the public value
BP_HD void opn_bind(strobe &t, uint32_t form, const uint32_t C[8], const uint32_t v[8]) {
    const uint8_t dsep[7] = {'d', 'o', 'm', '-', 's', 'e', 'p'}, lf[4] = {'f', 'o', 'r', 'm'}, lC[1] = {'C'}, lv[1] = {'v'};
    const uint8_t name[15] = {'o', 'p', 'e', 'n', 'i', 'n', 'g', 'p', 'r', 'o', 'o', 'f', ' ', 'v', '1'};
    merlin_append_message(t, dsep, 7, name, 15);
    merlin_append_u64(t, lf, 4, form);
    merlin_append_words8(t, lC, 1, C);
    if (form == OPN_BLINDING) merlin_append_words8(t, lv, 1, v);
}
// R (the caller has looked at it: not 32 zero bytes) and the challenge
BP_HD void opn_challenge(strobe &t, const uint32_t R[8], sc &c) {
    const uint8_t lR[1] = {'R'}, lc[1] = {'c'};
    merlin_append_words8(t, lR, 1, R);
    rp_challenge_scalar(t, lc, 1, c);
}

// what a batch of creations reads
struct opn_create_in {
    const uint32_t *values;        // [proof][value_words], or null (form 1, every value 0)
    const uint32_t *blindings;     // [proof][8]
    const uint8_t *seeds;          // [proof][32]: ChaChaRng::from_seed; form 0: k_v = draw 0, k_r = draw 1; form 1: k_r = draw 0
    const uint32_t *commitments;   // [proof][8]
    const uint32_t *ts_in;         // the callers' states, never null (sh.ts_in_stride words apart)
};
// nonce `which` (0: k_r, 1: k_v) of proof p
BP_HD void opn_nonce(uint32_t p, const opn_shape &sh, const uint8_t *seeds, uint32_t which, uint32_t k[8]) {
    sc x;
    rpp_draw(x, seeds + 32 * (uint64_t)p, sh.form == OPN_FULL ? 1u - which : 0u);
#pragma unroll
    for (int q = 0; q < 8; q++) k[q] = x.v[q];
}

// Phase 1 of the prover's lane: R = k_r B_blinding (+ k_v B in form 0: in form 1 nothing of B is walked) as 8 words.  v and r
// are not looked at: a row that the finish rejects walks like any other.  gen_ids: [0] = B_blinding, [1] = B.
// CT: table and prm are the W = 4 set.
template <bool CT>
BP_HD void opn_create_walk(uint32_t p, const opn_shape &sh, const opn_create_in &in, const ped_park &pk, fb_params prm, const uint32_t *gen_ids,
                           const fb_entry *table, uint32_t R[8]) {
    ge_ext acc;
    ge_identity(acc);
    bool started = false;
    const uint32_t nterms = sh.form == OPN_FULL ? 2u : 1u;   // (public: the form is one value per call)
#pragma unroll 1
    for (uint32_t term = 0; term < nterms; term++) {
        uint32_t k[8];
        opn_nonce(p, sh, in.seeds, term, k);
        if (CT) ped_walk_ct(acc, pk, k, prm.nwin, gen_ids[term], prm, table);
        else ped_walk(acc, started, pk, k, prm.nwin, gen_ids[term], prm, table);
    }
    ped_encode(R, acc, pk);
}

// Phase 2: the transcript (sponge `st`: it may lie over the parking space of phase 1 once every lane of the workgroup has left that
// phase), s_v = k_v + c v, s_r = k_r + c r, the stores.  A rejected row: proof bytes zero, status BAD_SCALAR, state = its input.
BP_HD void opn_create_finish(uint32_t p, const opn_shape &sh, const opn_create_in &in, kstate st, const uint32_t R[8],
                             uint32_t *proofs_out, uint8_t *status, uint32_t *ts_out) {
    sc c, v, x, k;
    uint32_t vw[8];
    opn_load_value(p, sh, in.values, vw);
#pragma unroll
    for (int q = 0; q < 8; q++) x.v[q] = in.blindings[8 * (uint64_t)p + q];
    const bool ok = sc_is_canonical(vw) & sc_is_canonical_sc(x);
    strobe t;
    opn_ts_load(t, st, p, nullptr, in.ts_in, sh.ts_in_stride);
    if (ts_out && !ok) rp_ts_emit(p, st, rp_ts_meta(t.pos, t.pos_begin, t.cur_flags), ts_out);
    {
        uint32_t Cw[8];
#pragma unroll
        for (int q = 0; q < 8; q++) Cw[q] = in.commitments[8 * (uint64_t)p + q];
        opn_bind(t, sh.form, Cw, vw);
    }
#pragma unroll
    for (int q = 0; q < 8; q++) v.v[q] = vw[q];
    opn_challenge(t, R, c);
    if (ts_out && ok) rp_ts_emit(p, st, rp_ts_meta(t.pos, t.pos_begin, t.cur_flags), ts_out);
    const uint32_t nw = opn_proof_words(sh.form);
    uint32_t *out = proofs_out + (uint64_t)p * nw;
#pragma unroll
    for (int q = 0; q < 8; q++) out[q] = ok ? R[q] : 0u;
    if (sh.form == OPN_FULL) {
        opn_nonce(p, sh, in.seeds, 1, k.v);
        sc_mul(x, c, v);
        sc_add(x, x, k);
#pragma unroll
        for (int q = 0; q < 8; q++) out[8 + q] = ok ? x.v[q] : 0u;
    }
#pragma unroll
    for (int q = 0; q < 8; q++) v.v[q] = in.blindings[8 * (uint64_t)p + q];
    opn_nonce(p, sh, in.seeds, 0, k.v);
    sc_mul(x, c, v);
    sc_add(x, x, k);
#pragma unroll
    for (int q = 0; q < 8; q++) out[nw - 8 + q] = ok ? x.v[q] : 0u;
    status[p] = ok ? (uint8_t)BP_STATUS_OK : (uint8_t)BP_STATUS_BAD_SCALAR;
}

// The verifier's front end, lane = proof.  status[p]: 0, or the verdict the row already carries -- FORMAT (a scalar of the proof or the
// public value is not canonical: the input state goes out), VERIFICATION (R is 32 zero bytes: the state as of that message).  A row
// that goes on gets c, its unique terms (-c, C), (-1, R) at slots 2p, 2p + 1 of uniq_sc / uniq_pt and its generator-table row
// (s_r, s_v, 0) at gen_sc + 3 * 8 p; the outputs are pre-zeroed by the host.  c_out (optional, the host harness): the challenge.
BP_HD void opn_front_lane(uint32_t p, const opn_shape &sh, const rp_strobe_init &init, kstate st, const uint32_t *proofs, const uint32_t *commitments,
                          const uint32_t *values, const uint32_t *ts_in, uint32_t *uniq_sc, uint32_t *uniq_pt, uint32_t *gen_sc, uint32_t *status,
                          uint32_t *ts_out, uint32_t *c_out = nullptr) {
    const uint32_t nw = opn_proof_words(sh.form);
    const uint32_t *pr = proofs + (uint64_t)p * nw;
    sc sv, sr, c;
    uint32_t w[8], vw[8];
    bool fmt = false;
#pragma unroll
    for (int q = 0; q < 8; q++) sr.v[q] = pr[nw - 8 + q];
    fmt = !sc_is_canonical_sc(sr);
    opn_load_value(p, sh, values, vw);   // the public value of form 1 (form 0: no buffer, zeros)
#pragma unroll
    for (int q = 0; q < 8; q++) sv.v[q] = sh.form == OPN_FULL ? pr[8 + q] : vw[q];
    fmt = fmt || !sc_is_canonical_sc(sv);
    strobe t;
    opn_ts_load(t, st, p, &init, ts_in, sh.ts_in_stride);
    if (fmt) {
        status[p] = BP_VERDICT_FORMAT;
        if (ts_out) rp_ts_emit(p, st, rp_ts_meta(t.pos, t.pos_begin, t.cur_flags), ts_out);
        return;
    }
    // C, v and R are absorbed from global memory (the absorb loop indexes its message: a copy in registers would go to scratch); the
    // public value, zero-extended, waits for that in the row's s_v slot, which c v overwrites below
    uint32_t *grow = gen_sc + (uint64_t)p * OPN_GEN_ROW * 8;
    if (sh.form == OPN_BLINDING) {
#pragma unroll
        for (int q = 0; q < 8; q++) grow[8 + q] = vw[q];
    }
    opn_bind(t, sh.form, commitments + 8 * (uint64_t)p, grow + 8);
#pragma unroll
    for (int q = 0; q < 8; q++) w[q] = pr[q];
    if (words8_zero(w)) {
#pragma unroll
        for (int q = 0; q < 8; q++) grow[8 + q] = 0u;
        status[p] = BP_VERDICT_VERIFICATION;
        if (ts_out) rp_ts_emit(p, st, rp_ts_meta(t.pos, t.pos_begin, t.cur_flags), ts_out);
        return;
    }
    opn_challenge(t, pr, c);
    if (ts_out) rp_ts_emit(p, st, rp_ts_meta(t.pos, t.pos_begin, t.cur_flags), ts_out);
#pragma unroll
    for (int q = 0; q < 8; q++) {
        uniq_pt[16 * (uint64_t)p + q] = commitments[8 * (uint64_t)p + q];
        uniq_pt[16 * (uint64_t)p + 8 + q] = pr[q];
    }
    if (c_out) store_words8(c_out + 8 * (uint64_t)p, c);
    if (sh.form == OPN_BLINDING) sc_mul(sv, c, sv);   // s_v = c v
    sc x, one;
    sc_neg(x, c);
    store_words8(uniq_sc + 16 * (uint64_t)p, x);
    sc_from_u32(one, 1);
    sc_neg(x, one);
    store_words8(uniq_sc + 16 * (uint64_t)p + 8, x);
    store_words8(grow, sr);
    store_words8(grow + 8, sv);
    status[p] = 0;
}

// rlc_weigh_thread's index map over the front end's staging: U = 2 unique terms per proof, two shared rows (0: B_blinding, 1: B)
struct opn_rlc_map {
    const uint32_t *gen_sc;
    BP_HD uint64_t uniq(uint32_t p, uint32_t t) const { return (uint64_t)p * 2 + t; }
    BP_HD const uint32_t *shared(uint32_t p, uint32_t g) const { return gen_sc + ((uint64_t)p * OPN_GEN_ROW + g) * 8; }
    BP_HD uint32_t row(uint32_t g) const { return g; }
};
// lane tid = term * nstride + proof over 2 + 2 terms
BP_HD bool opn_rlc_weigh_thread(uint32_t tid, uint32_t nproofs, uint32_t nstride, const uint32_t *status, const uint32_t *rho, const uint32_t *gen_sc,
                                const uint32_t *uniq_sc, const uint32_t *uniq_pt, uint32_t *comb_sc, uint32_t *comb_pt, sc &v, uint32_t &row) {
    return rlc_weigh_thread(tid, nproofs, nstride, 2, opn_rlc_map{gen_sc}, status, rho, uniq_sc, uniq_pt, comb_sc, comb_pt, v, row);
}

}  // namespace bp
#endif
