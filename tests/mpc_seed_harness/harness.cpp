// Host harness for the SEEDED party steps of the multi-party aggregation protocol: the step-1 and step-2 lane bodies of mpc_party.h
// compiled with g++, once over a draw source of pre-expanded bytes (mpc_from_bytes, the bodies of bpgpu_mpc_party_bit_commit /
// _poly_commit) and once over seeds and first-draw indices (mpc_from_seed, the bodies of the _seeded entry points), driven the way
// bpgpu.hip drives them: rows grouped by position with mpc_plan_slots, values, blindings, seeds and bases carried through the SAME
// row-to-slot map, every slot -- padding included -- through the lanes, results put back in the caller's order.  Every buffer has
// its logical size in a heap allocation of its own (seeds 32 x nslots, bases 8 x nslots): the sanitized build sees an overrun.
// Built as a shared library by tests/test_mpc_seed_on_cpu.py and, with -DMSH_MAIN, as a stand-alone program that compares the two
// sources on generated rows and exits 0 when they agree.  TEST-ONLY: never part of libbpgpu.so, never a fallback.
#define BP_FE_CHECK 1
#include "../../bulletproofs_amd/csrc/mpc_party.h"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace bp;

extern "C" {

uint32_t msh_state_words(uint32_t n, int which) { return which == 1 ? MPC_ST1_WORDS(n) : MPC_ST2_WORDS(n); }

// Steps 1 and 2 for nrows parties, caller order in and out.
//   seeded != 0: rng1 = seeds [nrows][32], base1 / base2 [nrows] the first draw of step 1 / step 2; rng2 is not read
//   seeded == 0: rng1 [nrows][64 (2n + 2)], rng2 [nrows][128] pre-expanded bytes; base1, base2 are not read
//   st1 [nrows][MPC_ST1_WORDS], rows_v [nrows][2][32], rows_as [nrows][2][2n + 2][32], st2 [nrows][MPC_ST2_WORDS], rows_t [nrows][2][2][32], status2 [nrows]
// Returns the number of slots, or -1 when the plan is no permutation.
int msh_party(int seeded, uint32_t n, uint32_t nrows, uint32_t npos, const uint32_t *pos, const uint64_t *values, const uint8_t *blindings, const uint8_t *rng1,
              const uint64_t *base1, const uint8_t *chal, uint32_t chal_shared, const uint8_t *rng2, const uint64_t *base2, uint8_t *st1_out, uint8_t *rows_v,
              uint8_t *rows_as, uint8_t *st2_out, uint8_t *rows_t, uint8_t *status2) {
    const size_t cap = mpc_plan_cap(nrows, npos), row_len = 2 * n + 2, per1 = seeded ? 32 : 64 * row_len, per2 = 128;
    std::vector<uint32_t> row_slot(nrows), slot_row(cap, MPC_NO_ROW), blk_pos(cap / MPC_WAVE);
    const uint32_t ns = mpc_plan_slots(nrows, pos, npos, row_slot.data(), slot_row.data(), blk_pos.data());
    std::vector<uint32_t> slot_pos(ns, MPC_NO_ROW);
    std::vector<uint64_t> v(ns, 0), b1(seeded ? ns : 0, 0), b2(seeded ? ns : 0, 0);
    std::vector<uint32_t> bl(ns * 8, 0), r1(ns * per1 / 4, 0), r2(seeded ? 0 : ns * per2 / 4, 0), ch((chal_shared ? 1 : ns) * 16, 0);
    if (chal_shared) memcpy(ch.data(), chal, 64);
    for (uint32_t r = 0; r < nrows; r++) {
        const uint32_t s = row_slot[r];
        if (s >= ns || slot_row[s] != r || blk_pos[s / MPC_WAVE] != pos[r]) return -1;
        slot_pos[s] = pos[r];
        v[s] = values[r];
        memcpy(bl.data() + 8 * (size_t)s, blindings + 32 * (size_t)r, 32);
        memcpy((uint8_t *)r1.data() + per1 * s, rng1 + per1 * r, per1);
        if (seeded) {
            b1[s] = base1[r];
            b2[s] = base2[r];
        } else {
            memcpy((uint8_t *)r2.data() + per2 * s, rng2 + per2 * r, per2);
        }
        if (!chal_shared) memcpy((uint8_t *)ch.data() + 64 * (size_t)s, chal + 64 * (size_t)r, 64);
    }
    const size_t w1 = MPC_ST1_WORDS(n), w2 = MPC_ST2_WORDS(n);
    std::vector<uint32_t> gsV((size_t)ns * 16, 0), gsAS((size_t)2 * ns * row_len * 8, 0), st1((size_t)ns * w1, 0), st2((size_t)ns * w2, 0), gsT((size_t)2 * ns * 16, 0),
        stat(ns, 0);
    if (seeded) {
        const mpc_from_seed s1{(const uint8_t *)r1.data(), b1.data()}, s2{(const uint8_t *)r1.data(), b2.data()};
        for (uint32_t s = 0; s < ns; s++) mpc_blind_lane(s, n, ns, slot_pos.data(), v.data(), (const uint8_t *)bl.data(), s1, gsV.data(), gsAS.data(), st1.data());
        for (uint32_t t = 0; t < ns * n; t++) mpc_bits_lane(t, n, ns, slot_pos.data(), v.data(), s1, gsAS.data(), st1.data());
        for (uint32_t s = 0; s < ns; s++)
            mpc_poly_lane(s, n, ns, slot_pos.data(), st1.data(), (const uint8_t *)ch.data(), chal_shared, s2, st2.data(), gsT.data(), stat.data());
    } else {
        const uint8_t *p1 = (const uint8_t *)r1.data(), *p2 = (const uint8_t *)r2.data();
        for (uint32_t s = 0; s < ns; s++) mpc_blind_thread(s, n, ns, slot_pos.data(), v.data(), (const uint8_t *)bl.data(), p1, gsV.data(), gsAS.data(), st1.data());
        for (uint32_t t = 0; t < ns * n; t++) mpc_bits_thread(t, n, ns, slot_pos.data(), v.data(), p1, gsAS.data(), st1.data());
        for (uint32_t s = 0; s < ns; s++)
            mpc_poly_thread(s, n, ns, slot_pos.data(), st1.data(), (const uint8_t *)ch.data(), chal_shared, p2, st2.data(), gsT.data(), stat.data());
    }
    for (uint32_t s = 0; s < ns; s++) {   // padding slots draw nothing and write nothing
        if (slot_pos[s] != MPC_NO_ROW) continue;
        for (size_t q = 0; q < w1; q++)
            if (st1[s * w1 + q]) return -2;
        for (size_t q = 0; q < w2; q++)
            if (st2[s * w2 + q]) return -2;
        for (size_t q = 0; q < 8 * row_len; q++)
            if (gsAS[(size_t)s * row_len * 8 + q] | gsAS[(size_t)(ns + s) * row_len * 8 + q]) return -2;
    }
    for (uint32_t r = 0; r < nrows; r++) {
        const uint32_t s = row_slot[r];
        memcpy(st1_out + 4 * w1 * r, st1.data() + (size_t)s * w1, 4 * w1);
        memcpy(st2_out + 4 * w2 * r, st2.data() + (size_t)s * w2, 4 * w2);
        memcpy(rows_v + 64 * (size_t)r, gsV.data() + 16 * (size_t)s, 64);
        memcpy(rows_as + 64 * row_len * r, gsAS.data() + (size_t)s * row_len * 8, 32 * row_len);
        memcpy(rows_as + 64 * row_len * r + 32 * row_len, gsAS.data() + (size_t)(ns + s) * row_len * 8, 32 * row_len);
        memcpy(rows_t + 128 * (size_t)r, gsT.data() + 16 * (size_t)s, 64);
        memcpy(rows_t + 128 * (size_t)r + 64, gsT.data() + 16 * (size_t)(ns + s), 64);
        status2[r] = (uint8_t)stat[s];
    }
    return (int)ns;
}

}  // extern "C"

#ifdef MSH_MAIN
// Generated rows (positions shuffled over 0..3, distinct seeds, first draws 0, 7, 2^32 - 3 -- the last straddles the carry into the
// counter's high word), the keystream expanded here with chacha20_block, both sources, every output compared.
static uint64_t lcg(uint64_t &x) {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    return x >> 11;
}
static int one(uint32_t n, uint32_t nrows, uint64_t seed) {
    const size_t row_len = 2 * n + 2, per1 = 64 * row_len, w1 = MPC_ST1_WORDS(n), w2 = MPC_ST2_WORDS(n);
    const uint64_t firsts[3] = {0, 7, 0xfffffffdull};
    std::vector<uint32_t> pos(nrows);
    std::vector<uint64_t> vals(nrows), base1(nrows), base2(nrows);
    std::vector<uint8_t> bl(32 * (size_t)nrows), seeds(32 * (size_t)nrows), rng1(per1 * nrows), rng2(128 * (size_t)nrows), chal(64 * (size_t)nrows);
    for (uint32_t r = 0; r < nrows; r++) {
        pos[r] = (uint32_t)(lcg(seed) % 4);
        vals[r] = lcg(seed) ^ (lcg(seed) << 32);
        base1[r] = firsts[lcg(seed) % 3];
        base2[r] = (r & 1) ? base1[r] + row_len : firsts[lcg(seed) % 3] + (r % 3);   // carried on, or anywhere (2^32 - 1: t_1, t_2 on either side of the carry)
        for (int q = 0; q < 32; q++) bl[32 * (size_t)r + q] = (uint8_t)lcg(seed), seeds[32 * (size_t)r + q] = (uint8_t)lcg(seed);
        for (int q = 0; q < 64; q++) chal[64 * (size_t)r + q] = (q % 32 == 31) ? 0 : (uint8_t)lcg(seed);   // canonical y, z
        if (r == 5) memset(&chal[64 * (size_t)r], 0xff, 32);                                                 // one rejected row
        uint32_t key[8], w[16];
        memcpy(key, &seeds[32 * (size_t)r], 32);
        for (size_t d = 0; d < row_len; d++) {
            chacha20_block(key, base1[r] + d, 0, 0, w);
            memcpy(&rng1[per1 * r + 64 * d], w, 64);
        }
        for (size_t d = 0; d < 2; d++) {
            chacha20_block(key, base2[r] + d, 0, 0, w);
            memcpy(&rng2[128 * (size_t)r + 64 * d], w, 64);
        }
    }
    std::vector<uint8_t> out[2][6];
    const size_t sizes[6] = {4 * w1 * nrows, 64 * (size_t)nrows, 64 * row_len * nrows, 4 * w2 * nrows, 128 * (size_t)nrows, nrows};
    int ns[2];
    for (int k = 0; k < 2; k++) {
        for (int q = 0; q < 6; q++) out[k][q].assign(sizes[q], 0);
        ns[k] = msh_party(k, n, nrows, 4, pos.data(), vals.data(), bl.data(), k ? seeds.data() : rng1.data(), k ? base1.data() : nullptr, chal.data(), 0,
                          k ? nullptr : rng2.data(), k ? base2.data() : nullptr, out[k][0].data(), out[k][1].data(), out[k][2].data(), out[k][3].data(),
                          out[k][4].data(), out[k][5].data());
    }
    if (ns[0] <= 0 || ns[0] != ns[1]) return 1;
    for (int q = 0; q < 6; q++)
        if (out[0][q] != out[1][q]) {
            fprintf(stderr, "n=%u nrows=%u: output %d differs between the seeded and the unseeded bodies\n", n, nrows, q);
            return 1;
        }
    if (nrows > 5 && out[1][5][5] != MPC_ST_BAD_SCALAR) return 1;
    return 0;
}
int main() {
    int bad = one(8, 1, 1) | one(8, 70, 2) | one(64, 70, 3) | one(16, 9, 4);
    if (!bad) printf("mpc seed harness ok\n");
    return bad;
}
#endif
