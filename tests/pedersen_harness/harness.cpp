// Host harness for the batched Pedersen commitments: pedersen.h's lane bodies (ped_commit_lane<false>, ped_commit_lane<true>, ped_open_lane)
// compiled with g++ and run lane by lane, the way k_ped_commit / k_ped_open run them, over a window table that the host-compiled
// fb_base_thread / fb_fill_thread / fb_norm_thread build.  TEST-ONLY: never part of libbpgpu.so, never a fallback.
// With -DPED_HARNESS_MAIN it is a stand-alone program (its own main, every buffer at its exact size) for the sanitizers.
#define BP_FE_CHECK 1
#include "../../bulletproofs_amd/csrc/pedersen.h"
using namespace bp;

static fb_params params_of(uint32_t W, uint32_t n_gens) {
    fb_params prm;
    prm.W = W;
    prm.nwin = fb_nwin(W);
    prm.half = 1u << (W - 1);
    prm.n_gens = n_gens;
    return prm;
}

extern "C" uint64_t ped_table_entries(uint32_t W, uint32_t n_gens) { return (uint64_t)n_gens * fb_nwin(W) * (1ull << (W - 1)); }
extern "C" uint32_t ped_table_entry_bytes() { return (uint32_t)sizeof(fb_entry); }
extern "C" uint32_t ped_windows_u64(uint32_t W) { return ped_u64_windows(params_of(W, 2)); }

// table[g][win][k] = (k + 1) 2^(W win) P_g for the n_gens compressed points; returns 1 when one of them does not decode
extern "C" int ped_build_table(uint32_t W, uint32_t n_gens, const uint32_t *gens_compressed, void *table_out) {
    const fb_params prm = params_of(W, n_gens);
    fb_entry *table = (fb_entry *)table_out;
    ge_ext *base = new ge_ext[(size_t)n_gens * prm.nwin];
    uint32_t bad = 0;
    for (uint32_t g = 0; g < n_gens; g++) fb_base_thread(g, prm, gens_compressed, base, &bad);
    for (uint32_t t = 0; t < n_gens * prm.nwin; t++) fb_fill_thread(t, prm, base, table);
    const uint64_t entries = ped_table_entries(W, n_gens), groups = (entries + BP_FB_NORM_GROUP - 1) / BP_FB_NORM_GROUP;
    for (uint64_t g = 0; g < groups; g++) fb_norm_thread(g, entries, table);
    delete[] base;
    return (int)bad;
}

// every lane of the commit kernel; ct != 0: the constant-time body (W must be BP_FB_CT_W)
extern "C" void ped_commit_rows(int ct, uint32_t W, uint32_t nbatch, const uint32_t *values, uint32_t value_words, const uint32_t *blindings,
                                const uint8_t *seed32, uint64_t first_draw, const uint32_t *gen_ids, const void *table, uint32_t *out_words,
                                uint32_t *blindings_out, uint8_t *status) {
    const fb_params prm = params_of(W, 2);
    const ped_in in = {values, value_words, blindings, seed32, first_draw};
    for (uint32_t i = 0; i < nbatch; i++) {
        uint32_t rw[10];
        ge_ext pt;
        const ped_park pk = {rw, 1, &pt};
        if (ct) ped_commit_lane<true>(i, in, pk, prm, gen_ids, (const fb_entry *)table, out_words, blindings_out, status);
        else ped_commit_lane<false>(i, in, pk, prm, gen_ids, (const fb_entry *)table, out_words, blindings_out, status);
    }
}

extern "C" void ped_open_rows(uint32_t W, uint32_t nbatch, const uint32_t *values, uint32_t value_words, const uint32_t *blindings,
                              const uint32_t *commitments, const uint32_t *gen_ids, const void *table, uint8_t *verdict) {
    const fb_params prm = params_of(W, 2);
    const ped_in in = {values, value_words, blindings, nullptr, 0};
    for (uint32_t i = 0; i < nbatch; i++) {
        uint32_t rw[10];
        ge_ext pt;
        const ped_park pk = {rw, 1, &pt};
        ped_open_lane(i, in, pk, commitments, prm, gen_ids, (const fb_entry *)table, verdict);
    }
}

// the finish alone: ped_encode against ristretto_compress on the points k P, k = 0 .. count - 1 (returns the number of differences)
extern "C" int ped_encode_against_compress(const uint32_t *point_compressed, uint32_t count) {
    ge_ext p, acc;
    if (!ristretto_decompress(p, point_compressed)) return -1;
    ge_identity(acc);
    int diff = 0;
    for (uint32_t k = 0; k < count; k++) {
        uint32_t a[8], b[8], rw[10];
        ge_ext pt;
        const ped_park pk = {rw, 1, &pt};
        ped_encode(a, acc, pk);
        ristretto_compress(b, acc);
        for (int q = 0; q < 8; q++) diff += a[q] != b[q];
        ge_add(acc, acc, p);
    }
    return diff;
}

#ifdef PED_HARNESS_MAIN
#include <cstdio>
#include <cstdlib>
#include <cstring>

// exact-size heap buffers: an access one element past any of them is the sanitizer's to report
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
    // two generators without the oracle: the Ristretto basepoint and its double; listed [B, B_blinding] with ids {1, 0}, so that the
    // id list is what places them
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
    const uint32_t Ws[3] = {BP_FB_CT_W, 5, 7};
    const uint32_t nb = 9;
    // rows: (0, 0), (1, 0), (0, 1), (2^64 - 1, l - 1), (2^63, 1), (0x8080.., r), (v, l) rejected, (5, 0x7f..), (2^64 - 1, 2^252)
    uint64_t *v64 = exact<uint64_t>(nb);
    uint32_t *v256 = exact<uint32_t>(8 * nb), *bl = exact<uint32_t>(8 * nb);
    const uint64_t vals[nb] = {0, 1, 0, ~0ull, 1ull << 63, 0x8080808080808080ull, 7, 5, ~0ull};
    memset(bl, 0, 32 * nb);
    for (uint32_t i = 0; i < nb; i++) {
        v64[i] = vals[i];
        memset(v256 + 8 * i, 0, 32);
        v256[8 * i] = (uint32_t)vals[i];
        v256[8 * i + 1] = (uint32_t)(vals[i] >> 32);
    }
    bl[8 * 2] = 1;
    memcpy(bl + 8 * 3, L, 32);
    bl[8 * 3] -= 1;
    bl[8 * 4] = 1;
    for (int q = 0; q < 7; q++) bl[8 * 5 + q] = 0x9e3779b9u * (q + 1);
    memcpy(bl + 8 * 6, L, 32);
    for (int q = 0; q < 7; q++) bl[8 * 7 + q] = 0x7f7f7f7fu;
    bl[8 * 8 + 7] = 0x10000000u;
    uint32_t *ref = exact<uint32_t>(8 * nb);
    for (int wi = 0; wi < 3; wi++) {
        const uint32_t W = Ws[wi];
        void *table = malloc(ped_table_entries(W, 2) * sizeof(fb_entry));
        CHECK(ped_build_table(W, 2, gens, table) == 0);
        for (int form = 0; form < (W == BP_FB_CT_W ? 2 : 1); form++) {
            uint32_t *out8 = exact<uint32_t>(8 * nb), *out32 = exact<uint32_t>(8 * nb), *blo = exact<uint32_t>(8 * nb);
            uint8_t *st = exact<uint8_t>(nb), *vd = exact<uint8_t>(nb);
            ped_commit_rows(form, W, nb, (const uint32_t *)v64, 2, bl, nullptr, 0, ids, table, out8, blo, st);
            CHECK(memcmp(blo, bl, 32 * nb) == 0);
            ped_commit_rows(form, W, nb, v256, 8, bl, nullptr, 0, ids, table, out32, nullptr, st);
            CHECK(memcmp(out8, out32, 32 * nb) == 0);                 // a u64 and the same value as a scalar: the same bytes
            if (wi == 0 && form == 0) memcpy(ref, out8, 32 * nb);
            CHECK(memcmp(out8, ref, 32 * nb) == 0);                   // every window size and the constant-time body: the same bytes
            for (uint32_t i = 0; i < nb; i++) CHECK(st[i] == (i == 6 ? BP_STATUS_BAD_SCALAR : BP_STATUS_OK));
            uint32_t z = 0;
            for (int q = 0; q < 8; q++) z |= out8[q] | out8[8 * 6 + q];
            CHECK(z == 0);                                            // (0, 0) and the rejected row: 32 zero bytes
            ped_open_rows(W, nb, (const uint32_t *)v64, 2, bl, out8, ids, table, vd);
            for (uint32_t i = 0; i < nb; i++) CHECK(vd[i] == (i == 6 ? 2 : 0));
            out8[8 * 4] ^= 1;                                         // one bit of a commitment
            v64[1] ^= 1ull << 40;                                     // ... of a value
            bl[8 * 5 + 3] ^= 0x100;                                   // ... of a blinding
            memset(out8 + 8 * 7, 0xff, 32);                           // no valid encoding
            ped_open_rows(W, nb, (const uint32_t *)v64, 2, bl, out8, ids, table, vd);
            for (uint32_t i = 0; i < nb; i++) CHECK(vd[i] == (i == 6 ? 2 : (i == 1 || i == 4 || i == 5 || i == 7) ? 1 : 0));
            v64[1] ^= 1ull << 40;
            bl[8 * 5 + 3] ^= 0x100;
            // seeded: rows 3 .. 7 of a full call == first_draw = 3 with 5 rows; the draws are what the rows open with
            uint8_t *seed = exact<uint8_t>(32);
            memset(seed, 24, 32);
            uint32_t *full = exact<uint32_t>(8 * 8), *part = exact<uint32_t>(8 * 5), *bfull = exact<uint32_t>(8 * 8), *bpart = exact<uint32_t>(8 * 5);
            uint8_t *st8 = exact<uint8_t>(8);
            ped_commit_rows(form, W, 8, (const uint32_t *)v64, 2, nullptr, seed, 0, ids, table, full, bfull, st8);
            ped_commit_rows(form, W, 5, (const uint32_t *)(v64 + 3), 2, nullptr, seed, 3, ids, table, part, bpart, st8);
            CHECK(memcmp(full + 8 * 3, part, 32 * 5) == 0 && memcmp(bfull + 8 * 3, bpart, 32 * 5) == 0);
            ped_open_rows(W, 8, (const uint32_t *)v64, 2, bfull, full, ids, table, st8);
            for (uint32_t i = 0; i < 8; i++) CHECK(st8[i] == 0);
            free(seed), free(full), free(part), free(bfull), free(bpart), free(st8);
            free(out8), free(out32), free(blo), free(st), free(vd);
        }
        free(table);
    }
    CHECK(ped_encode_against_compress(gens, 40) == 0);
    free(gens), free(ids), free(v64), free(v256), free(bl), free(ref);
    if (fails) return 1;
    printf("pedersen harness ok\n");
    return 0;
}
#endif
