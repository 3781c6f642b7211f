// Host harness for the sigma proofs of recorded relations: sigma.h's lane bodies (sig_vb_lane / sig_walk_lane / sig_finish_lane,
// sig_front_lane, the weigh lane of the combined check) and its descriptor parser compiled with g++ and run lane by lane, the way
// k_sig_vb / k_sig_walk / k_sig_finish / k_sig_front / k_sig_rlc_weigh run them, over a window table built by tests/pedersen_harness's
// builders whose rows are listed by base id (B_blinding, B, G_0 ..).  TEST-ONLY: never part of libbpgpu.so, never a fallback.
// With -DSIG_HARNESS_MAIN it is a stand-alone program (its own main, every buffer at its exact size) for the sanitizers.
#define BP_FE_CHECK 1
#include "../../bulletproofs_amd/csrc/sigma.h"
#include "../pedersen_harness/harness.cpp"

#include <vector>

extern "C" uint32_t sig_rel_bytes() { return (uint32_t)sizeof(sig_rel); }
// 0 and the record at rel_out, or 1 when the validator refuses the descriptor
extern "C" int sig_rel_from_desc(const uint8_t *desc, uint32_t len, uint32_t gens_capacity, void *rel_out) {
    sig_rel r;
    if (sig_rel_parse(desc, len, gens_capacity, r)) return 1;
    memcpy(rel_out, &r, sizeof r);
    return 0;
}

// one lane's k P against nothing but its own inputs: 8 words out (compress of the product), returns whether the point decoded
extern "C" int sig_kP(int ct, const uint32_t *k, const uint32_t *pt, uint32_t *out) {
    uint32_t rw[10];
    std::vector<uint32_t> t(SIG_VB_WORDS);
    const ped_park pk = {rw, 1, nullptr};
    const sig_vb_tab tab = {t.data(), 1};
    ge_ext q;
    const bool ok = ct ? sig_vb_mul<true>(q, pk, tab, k, pt) : sig_vb_mul<false>(q, pk, tab, k, pt);
    ristretto_compress(out, q);
    return ok ? 1 : 0;
}

// every lane of the three creation launches, in slices of `slice` rows (a multiple of 64) as the host runtime cuts them; ct != 0: the
// constant-time forms (W must be BP_FB_CT_W).  The workspace is allocated at its exact size.
extern "C" void sig_create_rows(int ct, uint32_t W, uint32_t n_gens, const void *relp, uint32_t nbatch, uint32_t slice, const uint32_t *secrets, const uint8_t *seeds,
                                const uint32_t *points, const uint32_t *ts_in, uint32_t ts_in_stride, const void *table, uint32_t *proofs_out, uint8_t *status,
                                uint32_t *ts_out) {
    const sig_rel &rel = *(const sig_rel *)relp;
    const fb_params prm = params_of(W, n_gens);
    const sig_create_in in = {secrets, seeds, points, ts_in, ts_in_stride, nbatch};
    std::vector<uint32_t> tabw((size_t)rel.nvb * slice * SIG_VB_WORDS), prod((size_t)rel.nvb * slice * 40), bad(nbatch, 0u);
    sig_ws ws = {tabw.data(), prod.data(), bad.data(), 0, slice};
    for (uint32_t row0 = 0; row0 < nbatch; row0 += slice) {
        ws.row0 = row0;
        const uint32_t nslice = nbatch - row0 < slice ? nbatch - row0 : slice;
        for (uint32_t tid = 0; tid < rel.nvb * slice; tid++) {
            const uint32_t v = tid / slice, row = row0 + (tid - v * slice);
            if (row >= nbatch) continue;
            uint32_t rw[10];
            const ped_park pk = {rw, 1, nullptr};
            if (ct) sig_vb_lane<true>(v, row, rel, in, pk, ws);
            else sig_vb_lane<false>(v, row, rel, in, pk, ws);
        }
        for (uint32_t tid = 0; tid < rel.E * slice; tid++) {
            const uint32_t k = tid / slice, i = tid - k * slice;
            if (i >= nslice) continue;
            alignas(16) uint32_t lds[52];
            const ped_park pk = {lds, 1, (ge_ext *)(lds + 12)};
            if (ct) sig_walk_lane<true>(k, row0 + i, rel, in, pk, ws, prm, (const fb_entry *)table, proofs_out);
            else sig_walk_lane<false>(k, row0 + i, rel, in, pk, ws, prm, (const fb_entry *)table, proofs_out);
        }
    }
    for (uint32_t p = 0; p < nbatch; p++) {
        uint32_t lds[50];
        kstate st;
        st.w = lds;
        st.stride = 1;
        sig_finish_lane(p, rel, in, st, bad.data(), proofs_out, status, ts_out);
    }
}

// every lane of the front end.  ts_in null: every lane starts from the one state init52 (52 words).  The outputs must come zeroed.
extern "C" void sig_front_rows(const void *relp, uint32_t nbatch, const uint32_t *proofs, const uint32_t *points, const uint32_t *ts_in, uint32_t ts_in_stride,
                               const uint32_t *init52, uint32_t *eq_sc, uint32_t *eq_pt, uint32_t *gen_sc, uint32_t *status, uint32_t *ts_out, uint32_t *c_out) {
    const sig_rel &rel = *(const sig_rel *)relp;
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
        sig_front_lane(p, rel, init, st, proofs, points, ts_in, ts_in_stride, eq_sc, eq_pt, gen_sc, status, ts_out, c_out);
    }
}

// the nbatch E weights, then every lane of the weigh launch with the accumulation of the 2 + G shared rows done here in the scalar
// field: comb_sc / comb_pt get the nbatch (P + E) weighted unique terms, rows_out the 2 + G coefficients
extern "C" void sig_weigh_rows(const void *relp, uint32_t nbatch, const uint8_t *weights64, const uint32_t *status, const uint32_t *gen_sc, const uint32_t *eq_sc,
                               const uint32_t *eq_pt, const uint32_t *points, uint32_t *rho, uint32_t *comb_sc, uint32_t *comb_pt, uint32_t *rows_out) {
    const sig_rel &rel = *(const sig_rel *)relp;
    rlc_key key = {};
    for (uint32_t r = 0; r < nbatch * rel.E; r++) rlc_rho_thread(r, weights64, key, SIG_RLC_WEIGHT_DOMAIN, rho);
    const uint32_t nstride = (nbatch + 63) / 64 * 64, GR = sig_gen_row(rel);
    std::vector<sc> rows(GR);
    for (uint32_t g = 0; g < GR; g++) sc_0(rows[g]);
    for (uint32_t tid = 0; tid < (rel.P + rel.E + GR) * nstride; tid++) {
        sc v;
        uint32_t row;
        if (sig_rlc_weigh_thread(tid, nbatch, nstride, rel, status, rho, gen_sc, eq_sc, eq_pt, points, comb_sc, comb_pt, v, row)) sc_add(rows[row], rows[row], v);
    }
    for (uint32_t g = 0; g < GR; g++) store_words8(rows_out + 8 * g, rows[g]);
}

#ifdef SIG_HARNESS_MAIN
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
    // four generators without the oracle: the Ristretto basepoint times 1, 2, 4, 8, listed by base id (B_blinding, B, G_0, G_1)
    const uint8_t bp_bytes[32] = {0xe2, 0xf2, 0xae, 0x0a, 0x6a, 0xbc, 0x4e, 0x71, 0xa8, 0x84, 0xa9, 0x61, 0xc5, 0x00, 0x51, 0x5f,
                                  0x58, 0xe3, 0x0b, 0x6a, 0xa5, 0x82, 0xdd, 0x8d, 0xb6, 0xa6, 0x59, 0x45, 0xe0, 0x8d, 0x2d, 0x76};
    const uint32_t NG = 4;
    uint32_t *gens = exact<uint32_t>(8 * NG);
    memcpy(gens, bp_bytes, 32);
    for (uint32_t g = 1; g < NG; g++) {
        ge_ext p;
        CHECK(ristretto_decompress(p, gens + 8 * (g - 1)));
        ge_dbl(p, p);
        ristretto_compress(gens + 8 * g, p);
    }
    // P0 = x0 B + x1 B_blinding + x2 G_1, P1 = x0 P2 + x1 P0 (a slot that is an lhs and a base), S = 3, P = 3, E = 2
    const uint8_t desc[] = {3, 3, 2, 16, 3, 0, 1, 1, 0, 2, 3, 17, 2, 0, 18, 1, 16};
    uint8_t *dcopy = exact<uint8_t>(sizeof desc);
    memcpy(dcopy, desc, sizeof desc);
    sig_rel *rel = exact<sig_rel>(1);
    CHECK(sig_rel_from_desc(dcopy, sizeof desc, NG - 2, rel) == 0);
    CHECK(sig_rel_from_desc(dcopy, sizeof desc, 1, rel + 0) == 1);          // G_1 beyond one generator
    CHECK(sig_rel_from_desc(dcopy, sizeof desc - 1, NG - 2, rel) == 1);      // the bytes end early
    CHECK(sig_rel_from_desc(dcopy, sizeof desc, NG - 2, rel) == 0);
    CHECK(rel->S == 3 && rel->P == 3 && rel->E == 2 && rel->G == 2 && rel->nvb == 2);
    const uint32_t S = 3, P = 3, E = 2, pw = 8 * (E + S), U = P + 1, GR = 2 + rel->G;
    const uint32_t L[8] = BP_L_WORDS;
    const uint32_t nb = 5;   // rows 0 .. 2 true statements, row 3 a secret of l (rejected), row 4 an instance base that does not decode (rejected)
    uint32_t *xs = exact<uint32_t>(8 * S * nb), *pts = exact<uint32_t>(8 * P * nb);
    memset(xs, 0, 32 * S * nb);
    for (uint32_t i = 0; i < nb; i++)
        for (uint32_t j = 0; j < S; j++)
            for (int q = 0; q < 7; q++) xs[8 * (S * i + j) + q] = 0x9e3779b9u * (q + 1 + 3 * j + 11 * i);
    memcpy(xs + 8 * (S * 1 + 1), L, 32);
    xs[8 * (S * 1 + 1)] -= 1;                 // l - 1
    memset(xs + 8 * (S * 2 + 2), 0, 32);      // 0
    uint8_t *seeds = exact<uint8_t>(32 * nb);
    for (uint32_t i = 0; i < 32 * nb; i++) seeds[i] = (uint8_t)(i * 7 + 1);
    uint32_t *ts = exact<uint32_t>(BP_TS_WORDS * nb);
    const uint32_t pos[nb] = {0, 100, 150, 165, 164};
    for (uint32_t i = 0; i < nb; i++) {
        for (int q = 0; q < 50; q++) ts[BP_TS_WORDS * i + q] = 0x01010101u * (i + 1) + q;
        ts[BP_TS_WORDS * i + 50] = rp_ts_meta(pos[i], pos[i] ? pos[i] - 1 : 0, BP_FLAG_A);
        ts[BP_TS_WORDS * i + 51] = 0;
    }
    // the instance: P2 = 16 basepoint; P0 and P1 from the equations, by plain double-and-add on the host
    auto mul = [](ge_ext &r, const uint32_t k[8], const ge_ext &p) {
        ge_identity(r);
        for (int bit = 255; bit >= 0; bit--) {
            ge_dbl(r, r);
            if ((k[bit >> 5] >> (bit & 31)) & 1) ge_add(r, r, p);
        }
    };
    ge_ext g[NG], p2;
    for (uint32_t i = 0; i < NG; i++) CHECK(ristretto_decompress(g[i], gens + 8 * i));
    ge_dbl(p2, g[3]);
    for (uint32_t i = 0; i < nb; i++) {
        const uint32_t *x = xs + 8 * S * i;
        ge_ext a, b, p0, p1;
        mul(a, x, g[1]);
        mul(b, x + 8, g[0]);
        ge_add(p0, a, b);
        mul(b, x + 16, g[3]);
        ge_add(p0, p0, b);
        mul(a, x, p2);
        mul(b, x + 8, p0);
        ge_add(p1, a, b);
        ristretto_compress(pts + 8 * (P * i), p0);
        ristretto_compress(pts + 8 * (P * i + 1), p1);
        ristretto_compress(pts + 8 * (P * i + 2), p2);
    }
    memcpy(xs + 8 * (S * 3 + 0), L, 32);                  // row 3: x0 = l
    memset(pts + 8 * (P * 4 + 2), 0xff, 32);              // row 4: P2 does not decode
    // sig_kP against double-and-add, both forms, for 0, 1, l - 1, 2^252 and a scalar of nibbles 0xf (every window carries into the next)
    {
        uint32_t ks[5][8] = {{0}, {1}, {0}, {0}, {0}};
        memcpy(ks[2], L, 32);
        ks[2][0] -= 1;
        ks[3][7] = 0x10000000u;
        for (int q = 0; q < 8; q++) ks[4][q] = q < 7 ? 0xffffffffu : 0x0fffffffu;
        for (int i = 0; i < 5; i++) {
            uint32_t *k = exact<uint32_t>(8), *o1 = exact<uint32_t>(8), *o2 = exact<uint32_t>(8), want[8];
            memcpy(k, ks[i], 32);
            CHECK(sig_kP(0, k, pts + 16, o1) == 1 && sig_kP(1, k, pts + 16, o2) == 1);
            ge_ext r;
            mul(r, k, p2);
            ristretto_compress(want, r);
            CHECK(memcmp(o1, want, 32) == 0 && memcmp(o2, want, 32) == 0);
            free(k), free(o1), free(o2);
        }
    }
    const uint32_t Ws[2] = {BP_FB_CT_W, 5};
    uint32_t *ref = exact<uint32_t>(pw * nb);
    for (int wi = 0; wi < 2; wi++) {
        const uint32_t W = Ws[wi];
        void *table = malloc(ped_table_entries(W, NG) * sizeof(fb_entry));
        CHECK(ped_build_table(W, NG, gens, table) == 0);
        for (int ct = 0; ct < (W == BP_FB_CT_W ? 2 : 1); ct++) {
            uint32_t *pr = exact<uint32_t>(pw * nb), *to = exact<uint32_t>(BP_TS_WORDS * nb);
            uint8_t *st = exact<uint8_t>(nb);
            sig_create_rows(ct, W, NG, rel, nb, 64, xs, seeds, pts, ts, BP_TS_WORDS, table, pr, st, to);
            if (wi == 0 && ct == 0) memcpy(ref, pr, 4 * pw * nb);
            CHECK(memcmp(pr, ref, 4 * pw * nb) == 0);   // every table form: the same bytes
            for (uint32_t i = 0; i < nb; i++) CHECK(st[i] == (i == 3 ? BP_STATUS_BAD_SCALAR : i == 4 ? BP_STATUS_BAD_POINT : BP_STATUS_OK));
            for (uint32_t i = 3; i < 5; i++) {
                uint32_t z = 0;
                for (uint32_t q = 0; q < pw; q++) z |= pr[pw * i + q];
                CHECK(z == 0 && memcmp(to + BP_TS_WORDS * i, ts + BP_TS_WORDS * i, 4 * BP_TS_WORDS) == 0);   // a rejected row: zero bytes, its input state
            }
            // the front end on the same statements: the same states, then every equation's check sums to the identity
            const uint32_t rows = nb * E;
            uint32_t *esc = exact<uint32_t>(8 * U * rows), *ept = exact<uint32_t>(8 * U * rows), *gsc = exact<uint32_t>(8 * GR * rows), *fst = exact<uint32_t>(nb),
                     *fto = exact<uint32_t>(BP_TS_WORDS * nb), *cs = exact<uint32_t>(8 * nb);
            memset(esc, 0, 32 * U * rows), memset(ept, 0, 32 * U * rows), memset(gsc, 0, 32 * GR * rows), memset(fst, 0, 4 * nb), memset(cs, 0, 32 * nb);
            sig_front_rows(rel, nb, pr, pts, ts, BP_TS_WORDS, nullptr, esc, ept, gsc, fst, fto, cs);
            for (uint32_t i = 0; i < nb; i++) {
                if (i >= 3) {   // T_1 = 32 zero bytes
                    CHECK(fst[i] == BP_VERDICT_VERIFICATION);
                    continue;
                }
                CHECK(fst[i] == 0 && memcmp(fto + BP_TS_WORDS * i, to + BP_TS_WORDS * i, 4 * BP_TS_WORDS) == 0);
                for (uint32_t k = 0; k < E; k++) {
                    const uint32_t r = i * E + k;
                    ge_ext sum, term, pt;
                    ge_identity(sum);
                    for (uint32_t b = 0; b < GR; b++) {
                        mul(term, gsc + 8 * (r * GR + b), g[b]);
                        ge_add(sum, sum, term);
                    }
                    for (uint32_t u = 0; u < U; u++) {
                        CHECK(ristretto_decompress(pt, ept + 8 * (r * U + u)));
                        mul(term, esc + 8 * (r * U + u), pt);
                        ge_add(sum, sum, term);
                    }
                    uint32_t enc[8], z = 0;
                    ristretto_compress(enc, sum);
                    for (int q = 0; q < 8; q++) z |= enc[q];
                    CHECK(z == 0);
                }
            }
            // the weigh map: nb (P + E) combined terms and 2 + G rows; a stopped row contributes scalar 0 on the identity encoding
            const uint32_t NU = P + E;
            uint32_t *rho = exact<uint32_t>(8 * rows), *csc = exact<uint32_t>(8 * NU * nb), *cpt = exact<uint32_t>(8 * NU * nb), *rws = exact<uint32_t>(8 * GR);
            uint8_t *w64 = exact<uint8_t>(64 * rows);
            for (uint32_t i = 0; i < 64 * rows; i++) w64[i] = (uint8_t)(i * 13 + 5);
            sig_weigh_rows(rel, nb, w64, fst, gsc, esc, ept, pts, rho, csc, cpt, rws);
            uint32_t z = 0;
            for (uint32_t q = 0; q < 8 * NU * 2; q++) z |= csc[8 * NU * 3 + q] | cpt[8 * NU * 3 + q];
            CHECK(z == 0);
            CHECK(memcmp(cpt, pts, 32 * P) == 0 && memcmp(cpt + 8 * P, pr, 32 * E) == 0);
            {
                ge_ext sum, term, pt;
                ge_identity(sum);
                for (uint32_t b = 0; b < GR; b++) {
                    mul(term, rws + 8 * b, g[b]);
                    ge_add(sum, sum, term);
                }
                for (uint32_t u = 0; u < NU * nb; u++) {
                    CHECK(ristretto_decompress(pt, cpt + 8 * u));
                    mul(term, csc + 8 * u, pt);
                    ge_add(sum, sum, term);
                }
                uint32_t enc[8];
                ristretto_compress(enc, sum);
                z = 0;
                for (int q = 0; q < 8; q++) z |= enc[q];
                CHECK(z == 0);   // the combination of the valid rows is the identity
            }
            free(rho), free(csc), free(cpt), free(rws), free(w64);
            free(esc), free(ept), free(gsc), free(fst), free(fto), free(cs);
            free(pr), free(to), free(st);
        }
        free(table);
    }
    free(ref), free(gens), free(dcopy), free(rel), free(xs), free(pts), free(seeds), free(ts);
    if (fails) return 1;
    printf("sigma harness ok\n");
    return 0;
}
#endif
