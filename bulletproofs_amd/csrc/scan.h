// Scanning range proofs under many wallet keys (include/bpgpu.h, bpgpu_rangeproof_scan_batch): rewind.h's rewind with the seed of a row
// found among nkeys candidates seed_{p,j} = SEED DERIVATION(keys32[j], commitment_p), and the transcript replayed ONCE per row.
// Four launches over one working set (k_scan.hip):
//   scn_prefix_lane  lane = key.  The STROBE state after Transcript::new(b"bpgpu rewind seed v1") + append_message(b"key", key_j):
//                    52 words per key; the state before the key (the same for every key) goes to the working set once, for the open.
//   scn_replay_lane  lane = row.  rwd_replay unchanged -> status, x, z; the row's survivor starts at SCN_NONE.
//   scn_cand_lane    lane = (row, key), THE HOT PATH.  Every key's prefix stands at STROBE position 91; appending C and asking for the
//                    seed absorbs 53 more bytes (144 < 166: the rate is never crossed), so a candidate costs exactly ONE Keccak-f, at the
//                    PRF.  Then draws 0 and 1, e = d_0 + d_1 x - e_blinding and the test e < 2^192.  The kernel keeps the lowest
//                    surviving j per row (atomicMin).  Rows whose replay failed spend nothing.
//   scn_open_*       lane = row.  The key of the survivor j*, its seed derived again (into the working set), then rwd_scalars and, behind
//                    the barrier, rwd_check: rewind.h's own arithmetic, walk, encode and compare, with seed_{p,j*} as the row's seed.
// CT form ("prover_constant_time"): no lane branches on e or j* and no address depends on them: every (row, key) lane of a replayed row
// does the same work and sends its atomicMin (SCN_NONE where the test fails); the open picks key j* by mask-select over a loop across all
// keys (uniform loads: the keys are shared), every replayed row derives a seed, computes one gamma and walks with ped_walk_ct; a row
// without a survivor walks the candidate of the all-zero key and is NOT_FOUND by mask.  A row the parse or the replay rejected (public)
// computes nothing and walks zeros, as in rewind.h.
#ifndef BPGPU_SCAN_H
#define BPGPU_SCAN_H
#include "rewind.h"

namespace bp {

#define SCN_NONE 0xffffffffu
#define SCN_MAX_KEYS 1024u
#define SCN_MAX_CANDIDATES (1u << 28)
// every key's prefix: the position after new(label) [13 + 9 + 4 + 22 = 48] and append_message(b"key", 32 bytes) [+ 9 + 34 = 91]; the
// operation in progress is the key's AD, begun at 57.  scn_prefix_lane computes the same figures (tests/scan_harness compares them).
#define SCN_PREFIX_POS 91u
#define SCN_PREFIX_BEGIN 58u
#define SCN_PRF_POS 144u   // the position at which the PRF permutes: 91 + (7 + 34) for C + 10 for the challenge's label and length + 2

struct scn_ws {
    uint32_t *prefix;   // [key][BP_TS_WORDS]
    uint32_t *base;     // [BP_TS_WORDS]: the state before the key
    uint32_t *status;   // [row]: the replay's status
    uint32_t *xz;       // [row][16]: x, z
    uint32_t *jstar;    // [row]: the lowest surviving key, or SCN_NONE
    uint32_t *seeds;    // [row][8]: seed_{p,j*}
};
struct scn_keys {
    const uint32_t *keys;   // [key][8]
    uint32_t nkeys;
};

BP_HD void scn_ts_store(uint32_t *o, const strobe &t) {
    for (uint32_t i = 0; i < 50; i++) o[i] = ks_get32(t.st, i);
    o[50] = rp_ts_meta(t.pos, t.pos_begin, t.cur_flags);
    o[51] = 0;
}

BP_HD void scn_prefix_lane(uint32_t j, const scn_keys &k, const scn_ws &ws, kstate st) {
    strobe t;
    merlin_strobe_init(t, st);
    const uint8_t dsep[7] = {'d', 'o', 'm', '-', 's', 'e', 'p'}, lkey[3] = {'k', 'e', 'y'};
    const uint8_t label[20] = {'b', 'p', 'g', 'p', 'u', ' ', 'r', 'e', 'w', 'i', 'n', 'd', ' ', 's', 'e', 'e', 'd', ' ', 'v', '1'};
    merlin_append_message(t, dsep, 7, label, 20);
    if (j == 0) scn_ts_store(ws.base, t);
    merlin_append_words8(t, lkey, 3, k.keys + 8 * (uint64_t)j);
    scn_ts_store(ws.prefix + (uint64_t)j * BP_TS_WORDS, t);
}

BP_HD void scn_replay_lane(uint32_t p, const rwd_shape &sh, const rwd_in &in, const scn_ws &ws, kstate st) {
    sc x, z;
    sc_0(x);
    sc_0(z);
    const uint32_t stat = rwd_replay(p, sh, in, st, x, z);
    ws.status[p] = stat;
    ws.jstar[p] = SCN_NONE;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        ws.xz[16 * (uint64_t)p + q] = x.v[q];
        ws.xz[16 * (uint64_t)p + 8 + q] = z.v[q];
    }
}

// the rest of the derivation from a state that has the key: append_message(b"C", C), challenge_bytes(b"seed", 32)
BP_HD void scn_seed_tail(strobe &t, const uint32_t *C, uint32_t seed[8]) {
    const uint8_t lC[1] = {'C'}, lseed[4] = {'s', 'e', 'e', 'd'};
    merlin_append_words8(t, lC, 1, C);
    strobe_meta_ad(t, lseed, 4, false);
    strobe_meta_len(t, 32);
    strobe_begin_op(t, BP_FLAG_I | BP_FLAG_A | BP_FLAG_C, false);
#pragma unroll
    for (int q = 0; q < 8; q++) seed[q] = strobe_squeeze_word(t);
}

// Candidate (row p, key j): j where e_j < 2^192, else SCN_NONE.  Only rows whose replay succeeded get here.
BP_HD uint32_t scn_cand_lane(uint32_t p, uint32_t j, const rwd_shape &sh, const rwd_in &in, const scn_ws &ws, kstate st) {
    strobe t;
    t.st = st;
    const uint32_t *pre = ws.prefix + (uint64_t)j * BP_TS_WORDS;
    for (uint32_t i = 0; i < 50; i++) ks_set32(st, i, pre[i]);
    t.pos = SCN_PREFIX_POS;
    t.pos_begin = SCN_PREFIX_BEGIN;
    t.cur_flags = BP_FLAG_A;
    uint32_t seed[8];
    scn_seed_tail(t, in.commitments + 8 * (uint64_t)p, seed);
    sc a, b, x;
#pragma unroll
    for (int q = 0; q < 8; q++) x.v[q] = ws.xz[16 * (uint64_t)p + q];
    rpp_draw_key(b, seed, 1);
    sc_mul(b, b, x);
    rpp_draw_key(a, seed, 0);
    sc_add(a, a, b);
    const uint32_t *pr = in.proofs + (uint64_t)p * sh.proof_words;
#pragma unroll
    for (int q = 0; q < 8; q++) b.v[q] = pr[48 + q];
    sc_sub(a, a, b);   // d_0 + d_1 x - e_blinding
    return (a.v[6] | a.v[7]) == 0 ? j : SCN_NONE;
}

// Open, before the barrier, live lanes only: key j*, seed_{p,j*} to the working set, then rewind.h's scalars under that seed.  Returns the status so far.
template <bool CT>
BP_HD uint32_t scn_open_scalars(uint32_t p, const rwd_shape &sh, const rwd_in &in, const scn_keys &k, const scn_ws &ws, const rwd_out &out,
                                kstate st, uint32_t &jstar) {
    uint32_t stat = ws.status[p];
    jstar = ws.jstar[p];
    const bool found = jstar != SCN_NONE;
    if (!CT && !found && stat == RWD_OK) stat = RWD_NOT_FOUND;
    sc x, z;
    sc_0(x);
    sc_0(z);
    if (stat == RWD_OK) {   // (public under CT: the replay's status)
        uint32_t key[8];
        if (CT) {
#pragma unroll
            for (int q = 0; q < 8; q++) key[q] = 0;
#pragma unroll 1
            for (uint32_t j = 0; j < k.nkeys; j++) {
                const uint32_t m = j == jstar ? 0xffffffffu : 0u;
#pragma unroll
                for (int q = 0; q < 8; q++) key[q] |= k.keys[8 * (uint64_t)j + q] & m;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 8; q++) key[q] = k.keys[8 * (uint64_t)jstar + q];
        }
        strobe t;
        opn_ts_load(t, st, 0, nullptr, ws.base, 0);
        const uint8_t lkey[3] = {'k', 'e', 'y'};
        merlin_append_words8(t, lkey, 3, key);
        uint32_t seed[8];
        scn_seed_tail(t, in.commitments + 8 * (uint64_t)p, seed);
#pragma unroll
        for (int q = 0; q < 8; q++) ws.seeds[8 * (uint64_t)p + q] = seed[q];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            x.v[q] = ws.xz[16 * (uint64_t)p + q];
            z.v[q] = ws.xz[16 * (uint64_t)p + 8 + q];
        }
    }
    const rwd_in in2 = {in.proofs, in.commitments, (const uint8_t *)ws.seeds, in.ts_in};
    stat = rwd_scalars<CT>(p, true, sh, in2, out, stat, x, z);
    if (CT) stat = (stat == RWD_OK && !found) ? RWD_NOT_FOUND : stat;   // (a select, not a branch)
    return stat;
}

// Open, behind the barrier, live lanes only: rewind.h's check, then the key index under the final status
template <bool CT>
BP_HD void scn_open_check(uint32_t p, const rwd_in &in, const rwd_out &out, uint32_t *key_index, uint32_t stat, uint32_t jstar, const ped_park &pk, fb_params prm,
                          const uint32_t *gen_ids, const fb_entry *table) {
    stat = rwd_check<CT>(p, in, out, stat, pk, prm, gen_ids, table);
    key_index[p] = stat == RWD_OK ? jstar : SCN_NONE;
}

}  // namespace bp
#endif
