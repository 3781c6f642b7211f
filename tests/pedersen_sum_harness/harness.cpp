// Host harness for the signed sums of Pedersen commitments: pedersen_sum.h's host plan and lane bodies compiled with g++ and run the
// way k_psum_terms / k_psum_reduce / k_psum_finish / k_psum_balance run them -- a workgroup phase by phase (every lane of a phase
// before any lane of the next, which is what the barriers give), the launches one after the other -- over a window table built as
// tests/pedersen_harness builds it (its table builders are included, not copied).  TEST-ONLY: never part of libbpgpu.so, never a
// fallback.  With -DPSUM_HARNESS_MAIN it is a stand-alone program (its own main, every buffer at its exact size) for the sanitizers.
#include "../pedersen_harness/harness.cpp"
#include "../../bulletproofs_amd/csrc/pedersen_sum.h"

#include <cstdlib>
#include <cstring>

extern "C" uint32_t psum_block() { return PSUM_BLOCK; }
extern "C" uint32_t psum_serial_max() { return PSUM_SERIAL_MAX; }
extern "C" uint32_t psum_max_passes() { return PSUM_MAX_PASSES; }

// the plan alone: table_out holds (PSUM_MAX_PASSES + 1) x (nbatch + 1) words; returns the number of passes
extern "C" uint32_t psum_plan_table(uint32_t nbatch, const uint32_t *row_offsets, uint32_t *table_out) {
    psum_plan pl;
    psum_make_plan(pl, nbatch, row_offsets);
    memcpy(table_out, pl.table.data(), pl.table.size() * 4);
    return pl.npasses;
}

// one workgroup of a pass: load, log2(PSUM_BLOCK) steps of (add | barrier | store | barrier), store the partials.  `written` counts the
// stores per slot of the pass's output.
static void run_workgroup(uint32_t block, const psum_pass &ps, const uint32_t *points, const uint8_t *signs, const ge_ext *src, uint8_t *bad, ge_ext *partial,
                          uint32_t nslots, uint8_t *written, int *errors) {
    ge_ext *pt = (ge_ext *)malloc(PSUM_BLOCK * sizeof(ge_ext)), *sum = (ge_ext *)malloc(PSUM_BLOCK * sizeof(ge_ext));
    uint32_t *row = (uint32_t *)malloc(PSUM_BLOCK * 4);
    bool on[PSUM_BLOCK];
    const psum_lds l = {pt, row};
    for (uint32_t lane = 0; lane < PSUM_BLOCK; lane++) {
        if (src) psum_load_partial(lane, block, ps, src, l);
        else psum_load_term(lane, block, ps, points, signs, bad, l);
    }
    for (uint32_t d = 1; d < PSUM_BLOCK; d <<= 1) {
        for (uint32_t lane = 0; lane < PSUM_BLOCK; lane++) on[lane] = psum_step_add(lane, d, l, sum[lane]);
        for (uint32_t lane = 0; lane < PSUM_BLOCK; lane++) psum_step_store(lane, l, sum[lane], on[lane]);
    }
    for (uint32_t lane = 0; lane < PSUM_BLOCK; lane++) {
        const uint32_t r = row[lane];
        if (r != PSUM_NO_ROW && (lane == 0 || row[lane - 1] != r)) {   // the lane that stores: its slot must lie inside the pass's output, and be its own
            const uint64_t slot = (uint64_t)ps.slot[r] + (block - ps.off[r] / PSUM_BLOCK);
            if (slot >= nslots || written[slot]) {
                (*errors)++;
                continue;
            }
            written[slot] = 1;
        }
        psum_store_partial(lane, block, ps, l, partial);
    }
    free(pt), free(sum), free(row);
}

// The whole call.  balance == 0: out_words (8 per row) and the BPGPU_MSM_* bytes; else the verdicts (out_words unused).  ct != 0: the
// constant-time body of the sum form (W must be BP_FB_CT_W).  values / blindings may be null; gen_ids and table too when both are.
// Returns the number of passes, or -1 when a partial's slot was out of range, stored twice or never stored.
extern "C" int psum_run(int balance, int ct, uint32_t W, uint32_t nbatch, const uint32_t *row_offsets, const uint32_t *points, const uint8_t *signs,
                        const uint32_t *values, uint32_t value_words, const uint32_t *blindings, const uint32_t *gen_ids, const void *table, uint32_t *out_words,
                        uint8_t *status) {
    psum_plan pl;
    psum_make_plan(pl, nbatch, row_offsets);
    uint8_t *bad = (uint8_t *)calloc(nbatch ? nbatch : 1, 1);
    int errors = 0;
    ge_ext *src = nullptr;
    for (uint32_t k = 0; k < pl.npasses; k++) {
        const uint32_t nslots = pl.items(k + 1);
        const psum_pass ps = {pl.items(k), nbatch, pl.off(k), pl.off(k + 1)};
        ge_ext *dst = (ge_ext *)malloc(nslots ? nslots * sizeof(ge_ext) : 1);
        uint8_t *written = (uint8_t *)calloc(nslots ? nslots : 1, 1);
        const uint32_t grid = (ps.total + PSUM_BLOCK - 1) / PSUM_BLOCK;
        for (uint32_t b = 0; b < grid; b++) run_workgroup(b, ps, points, signs, src, bad, dst, nslots, written, &errors);
        for (uint32_t i = 0; i < nslots; i++) errors += !written[i];
        free(written);
        free(src);
        src = dst;
    }
    const uint32_t *slot = pl.off(pl.npasses);
    for (uint32_t r = 0; r < nbatch; r++) errors += slot[r + 1] - slot[r] > PSUM_SERIAL_MAX;
    if (!errors) {
        const fb_params prm = params_of(W, 2);
        const ped_in in = {values, value_words, blindings, nullptr, 0};
        for (uint32_t r = 0; r < nbatch; r++) {
            uint32_t rw[10];
            ge_ext pt;
            const ped_park pk = {rw, 1, &pt};
            if (balance) psum_balance_lane(r, in, pk, prm, gen_ids, (const fb_entry *)table, slot, src, bad, status);
            else if (ct) psum_sum_lane<true>(r, in, pk, prm, gen_ids, (const fb_entry *)table, slot, src, bad, out_words, status);
            else psum_sum_lane<false>(r, in, pk, prm, gen_ids, (const fb_entry *)table, slot, src, bad, out_words, status);
        }
    }
    free(src);
    free(bad);
    return errors ? -1 : (int)pl.npasses;
}

// the parked decoder against ristretto_decompress on n encodings: the same decision, and the same point where it decodes
extern "C" int psum_decode_against_decompress(const uint32_t *enc, uint32_t n) {
    int diff = 0;
    for (uint32_t i = 0; i < n; i++) {
        ge_ext a, b;
        fe park;
        const bool oka = psum_decode(a, enc + 8 * i, &park), okb = ristretto_decompress(b, enc + 8 * i);
        diff += oka != okb;
        if (oka && okb) diff += !(fe_eq(a.X, b.X) && fe_eq(a.Y, b.Y) && fe_eq(a.Z, b.Z) && fe_eq(a.T, b.T));
    }
    return diff;
}

#ifdef PSUM_HARNESS_MAIN
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

// k P by double-and-add (k may be negative)
static void small_mul(ge_ext &r, const ge_ext &p, long long k) {
    ge_ext acc, q = p;
    ge_identity(acc);
    unsigned long long a = (unsigned long long)(k < 0 ? -k : k);
    for (; a; a >>= 1) {
        if (a & 1) ge_add(acc, acc, q);
        ge_dbl(q, q);
    }
    if (k < 0) ge_neg(acc, acc);
    r = acc;
}

int main() {
    const uint8_t bp_bytes[32] = {0xe2, 0xf2, 0xae, 0x0a, 0x6a, 0xbc, 0x4e, 0x71, 0xa8, 0x84, 0xa9, 0x61, 0xc5, 0x00, 0x51, 0x5f,
                                  0x58, 0xe3, 0x0b, 0x6a, 0xa5, 0x82, 0xdd, 0x8d, 0xb6, 0xa6, 0x59, 0x45, 0xe0, 0x8d, 0x2d, 0x76};
    // generators as in the Pedersen harness: the basepoint and its double, listed [B, B_blinding] with ids {1, 0}
    uint32_t *gens = exact<uint32_t>(16);
    memcpy(gens, bp_bytes, 32);
    ge_ext base;
    CHECK(ristretto_decompress(base, gens));
    {
        ge_ext p;
        ge_dbl(p, base);
        ristretto_compress(gens + 8, p);
    }
    uint32_t *ids = exact<uint32_t>(2);
    ids[0] = 1, ids[1] = 0;
    // the terms: term t is (t % 61 + 1) times the basepoint, so that a row's sum is a small multiple of it
    const uint32_t lens[] = {0, 1, 2, 63, 1, 64, 0, 65, 255, 3, 256, 257, 700, 0, 2 * PSUM_BLOCK * PSUM_BLOCK + 1};
    const uint32_t nb = sizeof lens / sizeof lens[0];
    uint32_t *off = exact<uint32_t>(nb + 1);
    off[0] = 0;
    for (uint32_t r = 0; r < nb; r++) off[r + 1] = off[r] + lens[r];
    const uint32_t total = off[nb];
    uint32_t *mult = exact<uint32_t>(61 * 8), *pts = exact<uint32_t>((size_t)total * 8);
    {
        ge_ext p = base;
        for (uint32_t k = 0; k < 61; k++) {
            ristretto_compress(mult + 8 * k, p);
            ge_add(p, p, base);
        }
    }
    for (uint32_t t = 0; t < total; t++) memcpy(pts + 8 * (size_t)t, mult + 8 * (t % 61), 32);
    CHECK(psum_decode_against_decompress(mult, 61) == 0);
    uint8_t *sg = exact<uint8_t>(total);
    for (uint32_t t = 0; t < total; t++) sg[t] = (uint8_t)((t * 7 + t / 5) & 1);
    uint32_t *out = exact<uint32_t>(8 * nb), *want = exact<uint32_t>(8 * nb);
    uint8_t *st = exact<uint8_t>(nb), *vd = exact<uint8_t>(nb);
    // 1. no scalars, no generators: every row against (sum of +-k) times the basepoint.  With signs: all rows, the last one through
    // the reduce pass; without: the rows before it (nbf of them), which need none.
    const uint32_t nbf = nb - 1;
    for (int with_signs = 0; with_signs < 2; with_signs++) {
        const uint32_t n = with_signs ? nb : nbf;
        CHECK(psum_run(0, 0, 7, n, off, pts, with_signs ? sg : nullptr, nullptr, 0, nullptr, nullptr, nullptr, out, st) == (with_signs ? 2 : 1));
        for (uint32_t r = 0; r < n; r++) {
            long long k = 0;
            for (uint32_t t = off[r]; t < off[r + 1]; t++) k += (with_signs && sg[t]) ? -(long long)(t % 61 + 1) : (long long)(t % 61 + 1);
            ge_ext p;
            small_mul(p, base, k);
            ristretto_compress(want + 8 * r, p);
            CHECK(st[r] == BP_STATUS_OK);
        }
        CHECK(memcmp(out, want, 32 * n) == 0);
        CHECK(psum_run(1, 0, 7, nbf, off, pts, with_signs ? sg : nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, vd) == 1);
        for (uint32_t r = 0; r < nbf; r++) {
            uint32_t z = 0;
            for (int q = 0; q < 8; q++) z |= want[8 * r + q];
            CHECK(vd[r] == (z ? 1 : 0));   // balances against (0, 0) exactly when the sum is the identity
        }
    }
    // 2. with scalars at W = 4 (both bodies) and W = 7: an empty row is the commitment; the sum opens in the balance form; a changed
    // value does not; a term that does not decode and a scalar that is not canonical are told apart
    // (on the first ten rows: 454 terms, two rows without any)
    const uint32_t nbs = 10;
    const uint32_t L[8] = BP_L_WORDS;
    uint64_t *v64 = exact<uint64_t>(nb);
    uint32_t *bl = exact<uint32_t>(8 * nb), *com = exact<uint32_t>(8 * nb), *ref = exact<uint32_t>(8 * nb);
    for (uint32_t r = 0; r < nb; r++) {
        v64[r] = 0x9e3779b97f4a7c15ull * (r + 1);
        for (int q = 0; q < 8; q++) bl[8 * r + q] = q < 7 ? 0x85ebca6bu * (8 * r + q + 1) : 0x0fffffffu;
    }
    const uint32_t Ws[2] = {BP_FB_CT_W, 7};
    for (int wi = 0; wi < 2; wi++) {
        const uint32_t W = Ws[wi];
        void *table = malloc(ped_table_entries(W, 2) * sizeof(fb_entry));
        CHECK(ped_build_table(W, 2, gens, table) == 0);
        for (int form = 0; form < (W == BP_FB_CT_W ? 2 : 1); form++) {
            ped_commit_rows(form, W, nbs, (const uint32_t *)v64, 2, bl, nullptr, 0, ids, table, com, nullptr, st);
            CHECK(psum_run(0, form, W, nbs, off, pts, sg, (const uint32_t *)v64, 2, bl, ids, table, out, st) == 1);
            if (wi == 0 && form == 0) memcpy(ref, out, 32 * nbs);
            CHECK(memcmp(out, ref, 32 * nbs) == 0);                             // every window size and body: the same bytes
            CHECK(memcmp(out, com, 32) == 0 && memcmp(out + 8 * 6, com + 8 * 6, 32) == 0);   // rows 0 and 6 have no terms
            // row r of a second call: the first call's sum added, the row's own terms with their signs flipped -- it opens to (v, r)
            uint32_t *off2 = exact<uint32_t>(nbs + 1);
            off2[0] = 0;
            for (uint32_t r = 0; r < nbs; r++) off2[r + 1] = off2[r] + lens[r] + 1;
            uint32_t *pts2 = exact<uint32_t>((size_t)off2[nbs] * 8);
            uint8_t *sg2 = exact<uint8_t>(off2[nbs]);
            for (uint32_t r = 0; r < nbs; r++) {
                memcpy(pts2 + 8 * (size_t)off2[r], out + 8 * r, 32);
                sg2[off2[r]] = 0;
                memcpy(pts2 + 8 * ((size_t)off2[r] + 1), pts + 8 * (size_t)off[r], 32 * (size_t)lens[r]);
                for (uint32_t i = 0; i < lens[r]; i++) sg2[off2[r] + 1 + i] = sg[off[r] + i] ^ 1;
            }
            CHECK(psum_run(1, 0, W, nbs, off2, pts2, sg2, (const uint32_t *)v64, 2, bl, ids, table, nullptr, vd) >= 1);
            for (uint32_t r = 0; r < nbs; r++) CHECK(vd[r] == 0);
            v64[2] ^= 1ull << 33;                         // a changed value
            pts2[8 * (size_t)off2[5] + 8 * 40] ^= 1;      // row 5: an encoding whose s is odd ("negative")
            memcpy(bl + 8 * 8, L, 32);                    // row 8: blinding l
            pts2[8 * (size_t)off2[8] + 8 * 100] ^= 1;     // ... and a bad point: the scalar takes precedence
            CHECK(psum_run(1, 0, W, nbs, off2, pts2, sg2, (const uint32_t *)v64, 2, bl, ids, table, nullptr, vd) >= 1);
            for (uint32_t r = 0; r < nbs; r++) CHECK(vd[r] == (r == 8 ? 2 : (r == 2 || r == 5) ? 1 : 0));
            CHECK(psum_run(0, form, W, nbs, off2, pts2, sg2, (const uint32_t *)v64, 2, bl, ids, table, out, st) >= 1);
            for (uint32_t r = 0; r < nbs; r++) CHECK(st[r] == (r == 8 ? BP_STATUS_BAD_SCALAR : r == 5 ? BP_STATUS_BAD_POINT : BP_STATUS_OK));
            uint32_t z = 0;
            for (int q = 0; q < 8; q++) z |= out[8 * 5 + q] | out[8 * 8 + q];
            CHECK(z == 0);
            v64[2] ^= 1ull << 33;
            for (int q = 0; q < 8; q++) bl[8 * 8 + q] = q < 7 ? 0x85ebca6bu * (8 * 8 + q + 1) : 0x0fffffffu;
            free(off2), free(pts2), free(sg2);
        }
        free(table);
    }
    free(gens), free(ids), free(off), free(mult), free(pts), free(sg), free(out), free(want), free(st), free(vd), free(v64), free(bl), free(com), free(ref);
    if (fails) return 1;
    printf("pedersen sum harness ok\n");
    return 0;
}
#endif
