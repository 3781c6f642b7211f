// Host harness for the opening proofs: opening.h's lane bodies (opn_create_walk / opn_create_finish, opn_front_lane, the weigh map of the
// combined check) compiled with g++ and run lane by lane, the way k_opn_create / k_opn_front / k_opn_rlc_weigh run them, over the
// two-generator window table of tests/pedersen_harness (its builders are included below).  A lane's 50 words serve as the walk's parking
// space and then as its sponge, as in the kernel.  TEST-ONLY: never part of libbpgpu.so, never a fallback.
// With -DOPN_HARNESS_MAIN it is a stand-alone program (its own main, every buffer at its exact size) for the sanitizers.
#define BP_FE_CHECK 1
#include "../../bulletproofs_amd/csrc/opening.h"
#include "../pedersen_harness/harness.cpp"

static opn_shape shape_of(uint32_t form, uint32_t nbatch, uint32_t value_words, uint32_t ts_in_stride) {
    opn_shape sh;
    sh.form = form;
    sh.nproofs = nbatch;
    sh.value_words = value_words;
    sh.ts_in_stride = ts_in_stride;
    return sh;
}

// every lane of the create kernel; ct != 0: the constant-time walk (W must be BP_FB_CT_W).  values may be null (value_words 0)
extern "C" void opn_create_rows(int ct, uint32_t W, uint32_t form, uint32_t nbatch, const uint32_t *values, uint32_t value_words, const uint32_t *blindings,
                                const uint8_t *seeds, const uint32_t *commitments, const uint32_t *ts_in, uint32_t ts_in_stride, const uint32_t *gen_ids,
                                const void *table, uint32_t *proofs_out, uint8_t *status, uint32_t *ts_out) {
    const fb_params prm = params_of(W, 2);
    const opn_shape sh = shape_of(form, nbatch, value_words, ts_in_stride);
    const opn_create_in in = {values, blindings, seeds, commitments, ts_in};
    for (uint32_t p = 0; p < nbatch; p++) {
        alignas(16) uint32_t lds[52];   // (the point behind the ten scalar words, at ge_ext's alignment)
        uint32_t R[8];
        const ped_park pk = {lds, 1, (ge_ext *)(lds + 12)};
        if (ct) opn_create_walk<true>(p, sh, in, pk, prm, gen_ids, (const fb_entry *)table, R);
        else opn_create_walk<false>(p, sh, in, pk, prm, gen_ids, (const fb_entry *)table, R);
        kstate st;
        st.w = lds;
        st.stride = 1;
        opn_create_finish(p, sh, in, st, R, proofs_out, status, ts_out);
    }
}

// every lane of the front end.  ts_in null: every lane starts from the one state init52 (52 words, the shared_transcript of the _dev
// forms).  The outputs must come zeroed, as the host runtime hands them to the kernel.
extern "C" void opn_front_rows(uint32_t form, uint32_t nbatch, const uint32_t *proofs, const uint32_t *commitments, const uint32_t *values, uint32_t value_words,
                               const uint32_t *ts_in, uint32_t ts_in_stride, const uint32_t *init52, uint32_t *uniq_sc, uint32_t *uniq_pt, uint32_t *gen_sc,
                               uint32_t *status, uint32_t *ts_out, uint32_t *c_out) {
    const opn_shape sh = shape_of(form, nbatch, value_words, ts_in_stride);
    rp_strobe_init init = {};
    if (init52) {
        for (int i = 0; i < 50; i++) init.w[i] = init52[i];
        init.pos = init52[50] & 0xffu;
        init.pos_begin = (init52[50] >> 8) & 0xffu;
        init.cur_flags = (init52[50] >> 16) & 0xffu;
    }
    for (uint32_t p = 0; p < nbatch; p++) {
        uint32_t lds[50];
        kstate st;
        st.w = lds;
        st.stride = 1;
        opn_front_lane(p, sh, init, st, proofs, commitments, values, ts_in, uniq_sc, uniq_pt, gen_sc, status, ts_out, c_out);
    }
}

// the weights, then every lane of the weigh launch (4 nstride lanes) with the accumulation of the two shared rows done here in the
// scalar field: comb_sc / comb_pt get the 2 nbatch weighted unique terms, rows_out the coefficients of B_blinding and B
extern "C" void opn_weigh_rows(uint32_t nbatch, const uint8_t *weights64, const uint32_t *status, const uint32_t *gen_sc, const uint32_t *uniq_sc,
                               const uint32_t *uniq_pt, uint32_t *rho, uint32_t *comb_sc, uint32_t *comb_pt, uint32_t *rows_out) {
    rlc_key key = {};
    for (uint32_t p = 0; p < nbatch; p++) rlc_rho_thread(p, weights64, key, OPN_RLC_WEIGHT_DOMAIN, rho);
    const uint32_t nstride = (nbatch + 63) / 64 * 64;
    sc rows[2];
    sc_0(rows[0]);
    sc_0(rows[1]);
    for (uint32_t tid = 0; tid < 4 * nstride; tid++) {
        sc v;
        uint32_t row;
        if (opn_rlc_weigh_thread(tid, nbatch, nstride, status, rho, gen_sc, uniq_sc, uniq_pt, comb_sc, comb_pt, v, row)) sc_add(rows[row], rows[row], v);
    }
    store_words8(rows_out, rows[0]);
    store_words8(rows_out + 8, rows[1]);
}

#ifdef OPN_HARNESS_MAIN
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

int main() {
    // two generators without the oracle: the Ristretto basepoint and its double, listed [B, B_blinding] with ids {1, 0}
    const uint8_t bp_bytes[32] = {0xe2, 0xf2, 0xae, 0x0a, 0x6a, 0xbc, 0x4e, 0x71, 0xa8, 0x84, 0xa9, 0x61, 0xc5, 0x00, 0x51, 0x5f,
                                  0x58, 0xe3, 0x0b, 0x6a, 0xa5, 0x82, 0xdd, 0x8d, 0xb6, 0xa6, 0x59, 0x45, 0xe0, 0x8d, 0x2d, 0x76};
    uint32_t *gens = exact<uint32_t>(16);
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
    const uint32_t nb = 5;   // rows: (0, 0), (2^64 - 1, l - 1), (7, r), (9, l) rejected, (1, 2^252)
    const uint64_t vals[nb] = {0, ~0ull, 7, 9, 1};
    uint64_t *v64 = exact<uint64_t>(nb);
    uint32_t *v256 = exact<uint32_t>(8 * nb), *bl = exact<uint32_t>(8 * nb);
    memset(bl, 0, 32 * nb);
    for (uint32_t i = 0; i < nb; i++) {
        v64[i] = vals[i];
        memset(v256 + 8 * i, 0, 32);
        v256[8 * i] = (uint32_t)vals[i];
        v256[8 * i + 1] = (uint32_t)(vals[i] >> 32);
    }
    memcpy(bl + 8 * 1, L, 32);
    bl[8 * 1] -= 1;
    for (int q = 0; q < 7; q++) bl[8 * 2 + q] = 0x9e3779b9u * (q + 1);
    memcpy(bl + 8 * 3, L, 32);
    bl[8 * 4 + 7] = 0x10000000u;
    uint8_t *seeds = exact<uint8_t>(32 * nb);
    for (uint32_t i = 0; i < 32 * nb; i++) seeds[i] = (uint8_t)(i * 7 + 1);
    // one state per proof: a patterned sponge at positions 0, 100, 150, 165 and 164 (the messages cross the rate boundary at different places)
    uint32_t *ts = exact<uint32_t>(BP_TS_WORDS * nb);
    const uint32_t pos[nb] = {0, 100, 150, 165, 164};
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
        for (int ct = 0; ct < (W == BP_FB_CT_W ? 2 : 1); ct++)
            for (uint32_t form = 0; form < 2; form++) {
                const uint32_t pw = opn_proof_words(form);
                uint32_t *pr8 = exact<uint32_t>(pw * nb), *pr32 = exact<uint32_t>(pw * nb), *to = exact<uint32_t>(BP_TS_WORDS * nb), *to2 = exact<uint32_t>(BP_TS_WORDS * nb);
                uint8_t *st = exact<uint8_t>(nb);
                opn_create_rows(ct, W, form, nb, (const uint32_t *)v64, 2, bl, seeds, coms, ts, BP_TS_WORDS, ids, table, pr8, st, to);
                opn_create_rows(ct, W, form, nb, v256, 8, bl, seeds, coms, ts, BP_TS_WORDS, ids, table, pr32, st, to2);
                CHECK(memcmp(pr8, pr32, 4 * pw * nb) == 0 && memcmp(to, to2, 4 * BP_TS_WORDS * nb) == 0);   // a u64 and the same value as a scalar
                for (uint32_t i = 0; i < nb; i++) CHECK(st[i] == (i == 3 ? BP_STATUS_BAD_SCALAR : BP_STATUS_OK));
                uint32_t z = 0;
                for (uint32_t q = 0; q < pw; q++) z |= pr8[pw * 3 + q];
                CHECK(z == 0 && memcmp(to + BP_TS_WORDS * 3, ts + BP_TS_WORDS * 3, 4 * BP_TS_WORDS) == 0);   // the rejected row: zero bytes, its input state
                // the front end on the same statements: the same states (contract c), then the check itself
                uint32_t *usc = exact<uint32_t>(16 * nb), *upt = exact<uint32_t>(16 * nb), *gsc = exact<uint32_t>(8 * OPN_GEN_ROW * nb), *fst = exact<uint32_t>(nb),
                         *fto = exact<uint32_t>(BP_TS_WORDS * nb), *cs = exact<uint32_t>(8 * nb);
                memset(usc, 0, 64 * nb), memset(upt, 0, 64 * nb), memset(gsc, 0, 32 * OPN_GEN_ROW * nb), memset(fst, 0, 4 * nb), memset(cs, 0, 32 * nb);
                opn_front_rows(form, nb, pr8, coms, form ? (const uint32_t *)v64 : nullptr, form ? 2 : 0, ts, BP_TS_WORDS, nullptr, usc, upt, gsc, fst, fto, cs);
                for (uint32_t i = 0; i < nb; i++) {
                    if (i == 3) {   // R = 32 zero bytes: VerificationError
                        CHECK(fst[i] == BP_VERDICT_VERIFICATION);
                        continue;
                    }
                    CHECK(fst[i] == 0 && memcmp(fto + BP_TS_WORDS * i, to + BP_TS_WORDS * i, 4 * BP_TS_WORDS) == 0);
                    // commit(s_v, s_r) == R + commit(c v, c r): the rows of generator-table scalars are (s_r, s_v, 0)
                    sc c, x;
                    uint32_t lhs[8], cvr[16], rhs[8];
                    uint8_t s1;
                    for (int q = 0; q < 8; q++) c.v[q] = cs[8 * i + q];
                    ped_commit_rows(0, W, 1, gsc + 8 * OPN_GEN_ROW * i + 8, 8, gsc + 8 * OPN_GEN_ROW * i, nullptr, 0, ids, table, lhs, nullptr, &s1);
                    for (int q = 0; q < 8; q++) x.v[q] = v256[8 * i + q];
                    sc_mul(x, c, x);
                    store_words8(cvr, x);
                    for (int q = 0; q < 8; q++) x.v[q] = bl[8 * i + q];
                    sc_mul(x, c, x);
                    store_words8(cvr + 8, x);
                    ped_commit_rows(0, W, 1, cvr, 8, cvr + 8, nullptr, 0, ids, table, rhs, nullptr, &s1);
                    ge_ext a, b;
                    CHECK(ristretto_decompress(a, rhs) && ristretto_decompress(b, pr8 + pw * i));
                    ge_add(a, a, b);
                    ristretto_compress(rhs, a);
                    CHECK(memcmp(lhs, rhs, 32) == 0);
                    CHECK(memcmp(upt + 16 * i, coms + 8 * i, 32) == 0 && memcmp(upt + 16 * i + 8, pr8 + pw * i, 32) == 0);
                }
                // the weigh map: the combined list has 2 nb terms, the rows two scalars
                uint32_t *rho = exact<uint32_t>(8 * nb), *csc = exact<uint32_t>(16 * nb), *cpt = exact<uint32_t>(16 * nb), *rows = exact<uint32_t>(16);
                uint8_t *w64 = exact<uint8_t>(64 * nb);
                for (uint32_t i = 0; i < 64 * nb; i++) w64[i] = (uint8_t)(i * 13 + 5);
                opn_weigh_rows(nb, w64, fst, gsc, usc, upt, rho, csc, cpt, rows);
                z = 0;
                for (int q = 0; q < 16; q++) z |= csc[16 * 3 + q] | cpt[16 * 3 + q];
                CHECK(z == 0);                                                // the stopped row: scalar 0 on the identity encoding
                CHECK(memcmp(cpt, upt, 32) == 0);
                free(rho), free(csc), free(cpt), free(rows), free(w64);
                free(usc), free(upt), free(gsc), free(fst), free(fto), free(cs);
                free(pr8), free(pr32), free(to), free(to2), free(st);
            }
        free(coms), free(cst), free(table);
    }
    free(gens), free(ids), free(v64), free(v256), free(bl), free(seeds), free(ts);
    if (fails) return 1;
    printf("opening harness ok\n");
    return 0;
}
#endif
