// Host harness for rewinding range proofs: rewind.h's lane bodies (rwd_replay, rwd_scalars, rwd_check) and the rewindable prover's draw
// source (rp_prover.h, rpp_from_seed_rw) compiled with g++ and run lane by lane, the way k_rewind runs them, over the two-generator
// window table of tests/pedersen_harness (its builders are included below).  A lane's 50 words serve as its sponge and then as the
// walk's parking space, as in the kernel.  TEST-ONLY: never part of libbpgpu.so, never a fallback.
// With -DRWD_HARNESS_MAIN it is a stand-alone program (its own main, every buffer at its exact size) for the sanitizers.
#define BP_FE_CHECK 1
#include "../../bulletproofs_amd/csrc/rewind.h"
#include "../pedersen_harness/harness.cpp"

static rwd_shape shape_of(uint32_t n, uint32_t nbatch, uint32_t ts_in_stride) {
    rwd_shape sh;
    sh.n = n;
    sh.k = 0;
    while ((1u << sh.k) < n) sh.k++;
    sh.nproofs = nbatch;
    sh.proof_words = 8 * (9 + 2 * sh.k);
    sh.ts_in_stride = ts_in_stride;
    return sh;
}

// every lane of the kernel; ct != 0: the constant-time form (W must be BP_FB_CT_W).  values: 2 words per row, messages 4, blindings 8
extern "C" void rwd_rows(int ct, uint32_t W, uint32_t n, uint32_t nbatch, const uint32_t *proofs, const uint32_t *commitments, const uint8_t *seeds,
                         const uint32_t *ts_in, uint32_t ts_in_stride, const uint32_t *gen_ids, const void *table, uint8_t *status, uint32_t *values,
                         uint32_t *messages, uint32_t *blindings) {
    const fb_params prm = params_of(W, 2);
    const rwd_shape sh = shape_of(n, nbatch, ts_in_stride);
    const rwd_in in = {proofs, commitments, seeds, ts_in};
    const rwd_out out = {status, values, messages, blindings};
    for (uint32_t p = 0; p < nbatch; p++) {
        alignas(16) uint32_t lds[52];   // (the point behind the ten scalar words, at ge_ext's alignment)
        kstate st;
        st.w = lds;
        st.stride = 1;
        sc x, z;
        sc_0(x);
        sc_0(z);
        uint32_t stat = rwd_replay(p, sh, in, st, x, z);
        const ped_park pk = {lds, 1, (ge_ext *)(lds + 12)};
        if (ct) {
            stat = rwd_scalars<true>(p, true, sh, in, out, stat, x, z);
            rwd_check<true>(p, in, out, stat, pk, prm, gen_ids, (const fb_entry *)table);
        } else {
            stat = rwd_scalars<false>(p, true, sh, in, out, stat, x, z);
            rwd_check<false>(p, in, out, stat, pk, prm, gen_ids, (const fb_entry *)table);
        }
    }
}

// the replay alone: the status it leaves and, where it is 0, the challenges x and z (8 words each per row)
extern "C" void rwd_replay_rows(uint32_t n, uint32_t nbatch, const uint32_t *proofs, const uint32_t *commitments, const uint32_t *ts_in, uint32_t ts_in_stride,
                                uint32_t *stat_out, uint32_t *x_out, uint32_t *z_out) {
    const rwd_shape sh = shape_of(n, nbatch, ts_in_stride);
    const rwd_in in = {proofs, commitments, nullptr, ts_in};
    for (uint32_t p = 0; p < nbatch; p++) {
        uint32_t lds[50];
        kstate st;
        st.w = lds;
        st.stride = 1;
        sc x, z;
        sc_0(x);
        sc_0(z);
        stat_out[p] = rwd_replay(p, sh, in, st, x, z);
        store_words8(x_out + 8 * p, x);
        store_words8(z_out + 8 * p, z);
    }
}

// draw d of every row through the rewindable prover's source (messages may be null) and through the plain seeded one
extern "C" void rwd_draw_rows(uint32_t nbatch, const uint8_t *seeds, const uint64_t *values, const uint32_t *messages, uint32_t d, uint32_t *rw_out,
                              uint32_t *seed_out) {
    rpp_shape sh = {};
    const rpp_from_seed_rw rw = {seeds, values, messages};
    const rpp_from_seed plain = {seeds};
    for (uint32_t p = 0; p < nbatch; p++) {
        sc r;
        rw.draw(r, sh, p, d);
        store_words8(rw_out + 8 * p, r);
        plain.draw(r, sh, p, d);
        store_words8(seed_out + 8 * p, r);
    }
}

#ifdef RWD_HARNESS_MAIN
#include <cstdio>
#include <cstdlib>
#include <cstring>

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

// Rows that rewind without a prover at hand: A, S, T_1, T_2 are arbitrary non-zero bytes (rewinding does not verify), x and z come from
// the replay, and e_blinding = d_0 - e + d_1 x, t_x_blinding = z^2 gamma + x (d_{2n+2} + x d_{2n+3}) are made to fit.
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
    const uint32_t nb = 6;   // rows: (0, 0, no msg), (2^64 - 1, l - 1, ff..), (7, r, msg), wrong seed, A = 0, e_blinding = l
    const uint64_t vals[nb] = {0, ~0ull, 7, 9, 11, 13};
    const uint32_t pos[nb] = {0, 100, 150, 165, 40, 164};
    for (uint32_t n = 8; n <= 64; n *= 8) {
        const rwd_shape sh = shape_of(n, nb, BP_TS_WORDS);
        const uint32_t pw = sh.proof_words;
        uint64_t *v64 = exact<uint64_t>(nb);
        uint32_t *bl = exact<uint32_t>(8 * nb), *msg = exact<uint32_t>(4 * nb);
        memset(bl, 0, 32 * nb);
        memset(msg, 0, 16 * nb);
        for (uint32_t i = 0; i < nb; i++) v64[i] = vals[i];
        memcpy(bl + 8 * 1, L, 32);
        bl[8 * 1] -= 1;
        memset(msg + 4 * 1, 0xff, 16);
        for (uint32_t i = 2; i < nb; i++) {
            for (int q = 0; q < 7; q++) bl[8 * i + q] = 0x9e3779b9u * (q + i);
            for (int q = 0; q < 4; q++) msg[4 * i + q] = 0x01000193u * (q + i);
        }
        uint8_t *seeds = exact<uint8_t>(32 * nb);
        for (uint32_t i = 0; i < 32 * nb; i++) seeds[i] = (uint8_t)(i * 7 + n);
        uint32_t *ts = exact<uint32_t>(BP_TS_WORDS * nb);
        for (uint32_t i = 0; i < nb; i++) {
            for (int q = 0; q < 50; q++) ts[BP_TS_WORDS * i + q] = 0x01010101u * (i + 1) + q;
            ts[BP_TS_WORDS * i + 50] = rp_ts_meta(pos[i], pos[i] ? pos[i] - 1 : 0, BP_FLAG_A);
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
            uint32_t *pr = exact<uint32_t>(pw * nb), *fst = exact<uint32_t>(nb), *xs = exact<uint32_t>(8 * nb), *zs = exact<uint32_t>(8 * nb);
            for (uint32_t i = 0; i < pw * nb; i++) pr[i] = 0x85ebca6bu * (i + 1) >> 4;   // points: any non-zero bytes; scalars: below 2^252
            rwd_replay_rows(n, nb, pr, coms, ts, BP_TS_WORDS, fst, xs, zs);
            uint32_t *d0 = exact<uint32_t>(8 * nb), *plain = exact<uint32_t>(8 * nb);
            rwd_draw_rows(nb, seeds, v64, msg, 0, d0, plain);   // d_0 - e, as the prover forms a_blinding
            for (uint32_t i = 0; i < nb; i++) {
                CHECK(fst[i] == 0);
                sc x, z, a, b, g;
                for (int q = 0; q < 8; q++) x.v[q] = xs[8 * i + q], z.v[q] = zs[8 * i + q], a.v[q] = d0[8 * i + q], g.v[q] = bl[8 * i + q];
                rpp_draw(b, seeds + 32 * i, 1);
                sc_mul(b, b, x);
                sc_add(a, a, b);
                store_words8(pr + pw * i + 48, a);   // e_blinding
                rpp_draw(b, seeds + 32 * i, 2 * n + 3);
                sc_mul(b, b, x);
                rpp_draw(a, seeds + 32 * i, 2 * n + 2);
                sc_add(a, a, b);
                sc_mul(a, a, x);
                sc_mul(b, z, z);
                sc_mul(b, b, g);
                sc_add(a, a, b);
                store_words8(pr + pw * i + 40, a);   // t_x_blinding
            }
            seeds[32 * 3] ^= 1;                      // row 3: another seed
            memset(pr + pw * 4, 0, 32);              // row 4: A of 32 zero bytes
            memcpy(pr + pw * 5 + 48, L, 32);         // row 5: e_blinding = l
            for (int ct = 0; ct < (W == BP_FB_CT_W ? 2 : 1); ct++) {
                uint8_t *st = exact<uint8_t>(nb);
                uint32_t *vo = exact<uint32_t>(2 * nb), *mo = exact<uint32_t>(4 * nb), *go = exact<uint32_t>(8 * nb);
                memset(st, 0x5a, nb), memset(vo, 0x5a, 8 * nb), memset(mo, 0x5a, 16 * nb), memset(go, 0x5a, 32 * nb);
                rwd_rows(ct, W, n, nb, pr, coms, seeds, ts, BP_TS_WORDS, ids, table, st, vo, mo, go);
                for (uint32_t i = 0; i < nb; i++) {
                    const uint8_t want = i < 3 ? RWD_OK : (i == 5 ? RWD_FORMAT : RWD_NOT_FOUND);
                    CHECK(st[i] == want);
                    if (want == RWD_OK) {
                        CHECK(memcmp(vo + 2 * i, v64 + i, 8) == 0 && memcmp(mo + 4 * i, msg + 4 * i, 16) == 0 && memcmp(go + 8 * i, bl + 8 * i, 32) == 0);
                    } else {
                        uint32_t z = 0;
                        for (int q = 0; q < 2; q++) z |= vo[2 * i + q];
                        for (int q = 0; q < 4; q++) z |= mo[4 * i + q];
                        for (int q = 0; q < 8; q++) z |= go[8 * i + q];
                        CHECK(z == 0);
                    }
                }
                free(st), free(vo), free(mo), free(go);
            }
            seeds[32 * 3] ^= 1;
            // one shared state (stride 0): row 0's state for row 0's proof
            {
                uint8_t st1 = 0x5a;
                uint32_t *vo = exact<uint32_t>(2), *mo = exact<uint32_t>(4), *go = exact<uint32_t>(8);
                rwd_rows(0, W, n, 1, pr, coms, seeds, ts, 0, ids, table, &st1, vo, mo, go);
                CHECK(st1 == RWD_OK && memcmp(vo, v64, 8) == 0 && memcmp(go, bl, 32) == 0);
                free(vo), free(mo), free(go);
            }
            // the prover's source: draw 0 differs from the seed's by e, every other draw is the seed's; no messages = message 0
            uint32_t *d5 = exact<uint32_t>(8 * nb), *p5 = exact<uint32_t>(8 * nb), *d0n = exact<uint32_t>(8 * nb);
            rwd_draw_rows(nb, seeds, v64, msg, 5, d5, p5);
            CHECK(memcmp(d5, p5, 32 * nb) == 0);
            rwd_draw_rows(nb, seeds, v64, nullptr, 0, d0n, p5);
            for (uint32_t i = 0; i < nb; i++) {
                sc a, b, e;
                for (int q = 0; q < 8; q++) a.v[q] = p5[8 * i + q], b.v[q] = d0n[8 * i + q];
                sc_sub(e, a, b);
                CHECK(e.v[0] == (uint32_t)vals[i] && e.v[1] == (uint32_t)(vals[i] >> 32) && (e.v[2] | e.v[3] | e.v[4] | e.v[5] | e.v[6] | e.v[7]) == 0);
            }
            free(d5), free(p5), free(d0n), free(d0), free(plain);
            free(pr), free(fst), free(xs), free(zs), free(coms), free(cst), free(table);
        }
        free(v64), free(bl), free(msg), free(seeds), free(ts);
    }
    free(gens), free(ids);
    if (fails) return 1;
    printf("rewind harness ok\n");
    return 0;
}
#endif
