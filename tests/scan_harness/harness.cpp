// Host harness for scanning under many keys: scan.h's lane bodies (scn_prefix_lane, scn_replay_lane, scn_cand_lane, scn_open_scalars,
// scn_open_check) compiled with g++ and run lane by lane over the grids k_scan.hip launches -- whole workgroups of 64, so the last
// lanes of a row block run past the batch as they do on the device -- with the working set laid out at its exact size.  The window
// table is tests/pedersen_harness's.  TEST-ONLY: never part of libbpgpu.so, never a fallback.
// With -DSCN_HARNESS_MAIN it is a stand-alone program (its own main, every buffer at its exact size) for the sanitizers.
#define BP_FE_CHECK 1
#include "../../bulletproofs_amd/csrc/scan.h"
#include "../pedersen_harness/harness.cpp"

#include <cstdlib>
#include <cstring>

static rwd_shape scn_shape_of(uint32_t n, uint32_t nbatch, uint32_t ts_in_stride) {
    rwd_shape sh;
    sh.n = n;
    sh.k = 0;
    while ((1u << sh.k) < n) sh.k++;
    sh.nproofs = nbatch;
    sh.proof_words = 8 * (9 + 2 * sh.k);
    sh.ts_in_stride = ts_in_stride;
    return sh;
}
static const uint32_t SCN_WG = 64;   // BP_BLOCK

// The four launches.  ct != 0: the constant-time form (W must be BP_FB_CT_W).  prefix_meta_out (nkeys + 1 words, may be null): the
// meta word of every key's prefix, then that of the state before the key.  cand_out (nbatch * nkeys words, may be null): what each
// (row, key) lane returned, SCN_NONE - 1 where the lane did not run.  Returns the number of candidate lanes that ran.
extern "C" uint64_t scn_rows(int ct, uint32_t W, uint32_t n, uint32_t nbatch, const uint32_t *proofs, const uint32_t *commitments, const uint32_t *ts_in,
                             uint32_t ts_in_stride, const uint32_t *keys, uint32_t nkeys, const uint32_t *gen_ids, const void *table, uint8_t *status,
                             uint32_t *key_index, uint32_t *values, uint32_t *messages, uint32_t *blindings, uint32_t *prefix_meta_out, uint32_t *cand_out) {
    const fb_params prm = params_of(W, 2);
    const rwd_shape sh = scn_shape_of(n, nbatch, ts_in_stride);
    const rwd_in in = {proofs, commitments, nullptr, ts_in};
    const rwd_out out = {status, values, messages, blindings};
    const scn_keys k = {keys, nkeys};
    auto words = [](size_t nw) { return (uint32_t *)malloc(nw ? nw * 4 : 1); };
    const scn_ws ws = {words((size_t)nkeys * BP_TS_WORDS), words(BP_TS_WORDS), words(nbatch), words(16 * (size_t)nbatch), words(nbatch), words(8 * (size_t)nbatch)};
    const uint32_t row_blocks = (nbatch + SCN_WG - 1) / SCN_WG, key_blocks = (nkeys + SCN_WG - 1) / SCN_WG;
    uint64_t ran = 0;
    alignas(16) uint32_t lds[52];
    const kstate st = {lds, 1};
    for (uint32_t j = 0; j < key_blocks * SCN_WG; j++)
        if (j < nkeys) scn_prefix_lane(j, k, ws, st);
    if (prefix_meta_out) {
        for (uint32_t j = 0; j < nkeys; j++) prefix_meta_out[j] = ws.prefix[(size_t)j * BP_TS_WORDS + 50];
        prefix_meta_out[nkeys] = ws.base[50];
    }
    for (uint32_t p = 0; p < row_blocks * SCN_WG; p++)
        if (p < nbatch) scn_replay_lane(p, sh, in, ws, st);
    if (cand_out)
        for (size_t i = 0; i < (size_t)nbatch * nkeys; i++) cand_out[i] = SCN_NONE - 1;
    for (uint32_t j = 0; j < nkeys; j++)            // blockIdx.y
        for (uint32_t p = 0; p < row_blocks * SCN_WG; p++) {
            if (p >= nbatch || ws.status[p] != RWD_OK) continue;
            const uint32_t c = scn_cand_lane(p, j, sh, in, ws, st);
            ran++;
            if (cand_out) cand_out[(size_t)p * nkeys + j] = c;
            if (ct || c != SCN_NONE) ws.jstar[p] = c < ws.jstar[p] ? c : ws.jstar[p];   // atomicMin
        }
    for (uint32_t p = 0; p < row_blocks * SCN_WG; p++) {
        if (p >= nbatch) continue;   // (a lane past the batch only waits at the barrier)
        uint32_t jstar = SCN_NONE;
        const ped_park pk = {lds, 1, (ge_ext *)(lds + 12)};
        if (ct) {
            const uint32_t stat = scn_open_scalars<true>(p, sh, in, k, ws, out, st, jstar);
            scn_open_check<true>(p, in, out, key_index, stat, jstar, pk, prm, gen_ids, (const fb_entry *)table);
        } else {
            const uint32_t stat = scn_open_scalars<false>(p, sh, in, k, ws, out, st, jstar);
            scn_open_check<false>(p, in, out, key_index, stat, jstar, pk, prm, gen_ids, (const fb_entry *)table);
        }
    }
    free(ws.prefix), free(ws.base), free(ws.status), free(ws.xz), free(ws.jstar), free(ws.seeds);
    return ran;
}

// seed_{p,j} of every (row, key) through the library's two-step derivation (prefix, then the tail): [row][key][8] words
extern "C" void scn_seed_rows(uint32_t nbatch, const uint32_t *commitments, const uint32_t *keys, uint32_t nkeys, uint32_t *seeds_out) {
    const scn_keys k = {keys, nkeys};
    const scn_ws ws = {(uint32_t *)malloc((size_t)nkeys * BP_TS_WORDS * 4), (uint32_t *)malloc(BP_TS_WORDS * 4), nullptr, nullptr, nullptr, nullptr};
    uint32_t lds[50];
    const kstate st = {lds, 1};
    for (uint32_t j = 0; j < nkeys; j++) scn_prefix_lane(j, k, ws, st);
    for (uint32_t p = 0; p < nbatch; p++)
        for (uint32_t j = 0; j < nkeys; j++) {
            strobe t;
            opn_ts_load(t, st, j, nullptr, ws.prefix, BP_TS_WORDS);
            scn_seed_tail(t, commitments + 8 * (size_t)p, seeds_out + 8 * ((size_t)p * nkeys + j));
        }
    free(ws.prefix), free(ws.base);
}
extern "C" uint32_t scn_prefix_pos(void) { return SCN_PREFIX_POS; }
extern "C" uint32_t scn_prf_pos(void) { return SCN_PRF_POS; }
extern "C" uint32_t scn_prefix_meta(void) { return rp_ts_meta(SCN_PREFIX_POS, SCN_PREFIX_BEGIN, BP_FLAG_A); }

#ifdef SCN_HARNESS_MAIN
#include <cstdio>

template <class T>
static T *exact(size_t n) {
    return (T *)malloc(n ? n * sizeof(T) : 1);
}
static int fails = 0;
#define CHECK(x)                                              \
    do {                                                      \
        if (!(x)) {                                           \
            printf("FAILED %s (line %d)\n", #x, __LINE__);    \
            fails++;                                          \
        }                                                     \
    } while (0)

// Rows that scan without a prover at hand, as in tests/rewind_harness: A, S, T_1, T_2 are arbitrary non-zero bytes, x and z come from the
// replay, and e_blinding, t_x_blinding are made to fit the seed of the row's owner key.  nb rows (not a multiple of 64: the last
// workgroup runs past the batch), row i owned by key i % nkeys except the rows turned into misses.
int main() {
    const uint8_t bp_bytes[32] = {0xe2, 0xf2, 0xae, 0x0a, 0x6a, 0xbc, 0x4e, 0x71, 0xa8, 0x84, 0xa9, 0x61, 0xc5, 0x00, 0x51, 0x5f,
                                  0x58, 0xe3, 0x0b, 0x6a, 0xa5, 0x82, 0xdd, 0x8d, 0xb6, 0xa6, 0x59, 0x45, 0xe0, 0x8d, 0x2d, 0x76};
    uint32_t *gens = exact<uint32_t>(16);   // [B, B_blinding]: the Ristretto basepoint and its double, ids {1, 0}
    memcpy(gens, bp_bytes, 32);
    {
        ge_ext p;
        CHECK(ristretto_decompress(p, gens));
        ge_dbl(p, p);
        ristretto_compress(gens + 8, p);
    }
    uint32_t *ids = exact<uint32_t>(2);
    ids[0] = 1, ids[1] = 0;
    const uint32_t L[8] = BP_L_WORDS;
    const uint32_t pos[5] = {0, 40, 100, 150, 165};
    const uint32_t shapes[3][2] = {{5, 1}, {65, 3}, {7, 65}};   // (rows, keys)
    for (int si = 0; si < 3; si++) {
        const uint32_t nb = shapes[si][0], nk = shapes[si][1], n = si == 1 ? 64 : 8;
        const rwd_shape sh = scn_shape_of(n, nb, BP_TS_WORDS);
        const uint32_t pw = sh.proof_words;
        uint64_t *v64 = exact<uint64_t>(nb);
        uint32_t *bl = exact<uint32_t>(8 * nb), *msg = exact<uint32_t>(4 * nb), *keys = exact<uint32_t>(8 * (nk + 1));
        for (uint32_t i = 0; i < nb; i++) {
            v64[i] = 0x0123456789abcdefull * (i + 1);
            for (int q = 0; q < 8; q++) bl[8 * i + q] = q < 7 ? 0x9e3779b9u * (q + i + 1) : 0;
            for (int q = 0; q < 4; q++) msg[4 * i + q] = 0x01000193u * (q + i);
        }
        for (uint32_t i = 0; i < 8 * (nk + 1); i++) keys[i] = 0xc2b2ae35u * (i + 7 * n);   // (key nk: nobody's)
        uint32_t *ts = exact<uint32_t>(BP_TS_WORDS * nb);
        for (uint32_t i = 0; i < nb; i++) {
            for (int q = 0; q < 50; q++) ts[BP_TS_WORDS * i + q] = 0x01010101u * (i + 1) + q;
            ts[BP_TS_WORDS * i + 50] = rp_ts_meta(pos[i % 5], pos[i % 5] ? pos[i % 5] - 1 : 0, BP_FLAG_A);
            ts[BP_TS_WORDS * i + 51] = 0;
        }
        const uint32_t Ws[2] = {BP_FB_CT_W, 5};
        for (int wi = 0; wi < 2; wi++) {
            const uint32_t W = Ws[wi];
            void *table = malloc(ped_table_entries(W, 2) * sizeof(fb_entry));
            CHECK(ped_build_table(W, 2, gens, table) == 0);
            uint32_t *coms = exact<uint32_t>(8 * nb);
            uint8_t *cst = exact<uint8_t>(nb);
            ped_commit_rows(0, W, nb, (const uint32_t *)v64, 2, bl, nullptr, 0, ids, table, coms, nullptr, cst);
            uint32_t *pr = exact<uint32_t>(pw * nb), *seeds = exact<uint32_t>(8 * (size_t)nb * (nk + 1));
            for (uint32_t i = 0; i < pw * nb; i++) pr[i] = 0x85ebca6bu * (i + 1) >> 4;   // points: any non-zero bytes; scalars: below 2^252
            scn_seed_rows(nb, coms, keys, nk + 1, seeds);
            // the miss rows: nobody's (the extra key), A = 0, e_blinding = l
            const uint32_t miss_nobody = nb > 3 ? 3 : SCN_NONE, miss_A = nb > 4 ? 4 : SCN_NONE, miss_fmt = nb > 6 ? 6 : SCN_NONE;
            {
                const rwd_in in = {pr, coms, nullptr, ts};
                for (uint32_t i = 0; i < nb; i++) {
                    uint32_t lds[50];
                    const kstate st = {lds, 1};
                    sc x, z, a, b, e, g;
                    CHECK(rwd_replay(i, sh, in, st, x, z) == RWD_OK);
                    const uint32_t owner = i == miss_nobody ? nk : i % nk;
                    const uint32_t *seed = seeds + 8 * ((size_t)i * (nk + 1) + owner);
                    sc_0(e);
                    e.v[0] = (uint32_t)v64[i], e.v[1] = (uint32_t)(v64[i] >> 32);
                    for (int q = 0; q < 4; q++) e.v[2 + q] = msg[4 * i + q];
                    for (int q = 0; q < 8; q++) g.v[q] = bl[8 * i + q];
                    rpp_draw_key(b, seed, 1);
                    sc_mul(b, b, x);
                    rpp_draw_key(a, seed, 0);
                    sc_add(a, a, b);
                    sc_sub(a, a, e);
                    store_words8(pr + pw * i + 48, a);   // e_blinding = d_0 - e + d_1 x
                    rpp_draw_key(b, seed, 2 * n + 3);
                    sc_mul(b, b, x);
                    rpp_draw_key(a, seed, 2 * n + 2);
                    sc_add(a, a, b);
                    sc_mul(a, a, x);
                    sc_mul(b, z, z);
                    sc_mul(b, b, g);
                    sc_add(a, a, b);
                    store_words8(pr + pw * i + 40, a);   // t_x_blinding
                }
            }
            if (miss_A != SCN_NONE) memset(pr + pw * miss_A, 0, 32);
            if (miss_fmt != SCN_NONE) memcpy(pr + pw * miss_fmt + 48, L, 32);
            for (int ct = 0; ct < (W == BP_FB_CT_W ? 2 : 1); ct++) {
                uint8_t *st = exact<uint8_t>(nb);
                uint32_t *ki = exact<uint32_t>(nb), *vo = exact<uint32_t>(2 * nb), *mo = exact<uint32_t>(4 * nb), *go = exact<uint32_t>(8 * nb);
                uint32_t *meta = exact<uint32_t>(nk + 1), *cand = exact<uint32_t>((size_t)nb * nk);
                memset(st, 0x5a, nb), memset(ki, 0x5a, 4 * nb), memset(vo, 0x5a, 8 * nb), memset(mo, 0x5a, 16 * nb), memset(go, 0x5a, 32 * nb);
                const uint64_t ran = scn_rows(ct, W, n, nb, pr, coms, ts, BP_TS_WORDS, keys, nk, ids, table, st, ki, vo, mo, go, meta, cand);
                uint32_t replayed = nb - (miss_A != SCN_NONE) - (miss_fmt != SCN_NONE);
                CHECK(ran == (uint64_t)replayed * nk);   // rows whose replay failed spend nothing per key
                for (uint32_t j = 0; j < nk; j++) CHECK(meta[j] == scn_prefix_meta());
                CHECK((meta[nk] & 0xff) == 48);
                for (uint32_t i = 0; i < nb; i++) {
                    const bool ok = i != miss_nobody && i != miss_A && i != miss_fmt;
                    CHECK(st[i] == (ok ? RWD_OK : (i == miss_fmt ? RWD_FORMAT : RWD_NOT_FOUND)));
                    CHECK(ki[i] == (ok ? i % nk : SCN_NONE));
                    if (ok) {
                        CHECK(memcmp(vo + 2 * i, v64 + i, 8) == 0 && memcmp(mo + 4 * i, msg + 4 * i, 16) == 0 && memcmp(go + 8 * i, bl + 8 * i, 32) == 0);
                        for (uint32_t j = 0; j < nk; j++) CHECK(cand[(size_t)i * nk + j] == (j == i % nk ? j : SCN_NONE));
                    } else {
                        uint32_t z = 0;
                        for (int q = 0; q < 2; q++) z |= vo[2 * i + q];
                        for (int q = 0; q < 4; q++) z |= mo[4 * i + q];
                        for (int q = 0; q < 8; q++) z |= go[8 * i + q];
                        CHECK(z == 0);
                    }
                }
                free(st), free(ki), free(vo), free(mo), free(go), free(meta), free(cand);
            }
            free(pr), free(seeds), free(coms), free(cst), free(table);
        }
        free(v64), free(bl), free(msg), free(keys), free(ts);
    }
    free(gens), free(ids);
    if (fails) return 1;
    printf("scan harness ok\n");
    return 0;
}
#endif
