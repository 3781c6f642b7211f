// Host harness for the multi-party aggregation protocol: the per-lane bodies of mpc_party.h / mpc_dealer.h compiled with g++ and driven
// the way bpgpu_mpc_party_* / bpgpu_mpc_dealer_assemble (bpgpu.hip) drive them -- rows grouped by position with mpc_plan_slots, every
// slot through the step-1 lanes, the step-2 lane and (back in caller order) the step-3 lane; the dealer's sums, concatenation and
// H-factors per session.  Buffers have their logical sizes in heap allocations of their own.  Built as a shared library by
// tests/test_mpc_on_cpu.py.  TEST-ONLY: never part of libbpgpu.so, never a fallback.
#define BP_FE_CHECK 1
#include "../../bulletproofs_amd/csrc/mpc_dealer.h"
#include <cstring>
#include <vector>
using namespace bp;

extern "C" {

uint64_t mh_plan_cap(uint64_t nrows, uint64_t npos) { return mpc_plan_cap(nrows, npos); }
uint32_t mh_plan(uint32_t nrows, const uint32_t *pos, uint32_t npos, uint32_t *row_slot, uint32_t *slot_row, uint32_t *blk_pos) {
    return mpc_plan_slots(nrows, pos, npos, row_slot, slot_row, blk_pos);
}
void mh_ids(uint32_t n, uint32_t j, uint32_t gens_capacity, uint32_t party_capacity, uint32_t *ids) { mpc_fill_ids(ids, n, j, gens_capacity, party_capacity); }
uint32_t mh_state_words(uint32_t n, int which) { return which == 1 ? MPC_ST1_WORDS(n) : MPC_ST2_WORDS(n); }

// steps 1-3 for nrows parties (caller order in, caller order out).
//   rows_v [nrows][2][32], rows_as [nrows][2][2n + 2][32]: the scalar rows of V_j and of A_j, S_j;  rows_t [nrows][2][2][32]: of T_1_j, T_2_j
//   coeffs [nrows][3][32]: t_0, t_1, t_2;  shares [nrows][32 (3 + 2n)];  status2, status3 [nrows]
int mh_party(uint32_t n, uint32_t nrows, uint32_t npos, const uint32_t *pos, const uint64_t *values, const uint8_t *blindings, const uint8_t *rng1,
             const uint8_t *chal, uint32_t chal_shared, const uint8_t *rng2, const uint8_t *xs, uint32_t x_shared, uint8_t *rows_v, uint8_t *rows_as,
             uint8_t *rows_t, uint8_t *coeffs, uint8_t *shares, uint8_t *status2, uint8_t *status3) {
    const size_t cap = mpc_plan_cap(nrows, npos), row_len = 2 * n + 2, per1 = 64 * row_len;
    std::vector<uint32_t> row_slot(nrows), slot_row(cap, MPC_NO_ROW), blk_pos(cap / MPC_WAVE);
    const uint32_t ns = mpc_plan_slots(nrows, pos, npos, row_slot.data(), slot_row.data(), blk_pos.data());
    std::vector<uint32_t> slot_pos(ns, MPC_NO_ROW);
    std::vector<uint64_t> v(ns, 0);
    std::vector<uint32_t> bl(ns * 8, 0), r1(ns * per1 / 4, 0), r2(ns * 32, 0), ch((chal_shared ? 1 : ns) * 16, 0);
    if (chal_shared) memcpy(ch.data(), chal, 64);
    for (uint32_t r = 0; r < nrows; r++) {
        const uint32_t s = row_slot[r];
        if (s >= ns || slot_row[s] != r || blk_pos[s / MPC_WAVE] != pos[r]) return -1;
        slot_pos[s] = pos[r];
        v[s] = values[r];
        memcpy(bl.data() + 8 * (size_t)s, blindings + 32 * (size_t)r, 32);
        memcpy((uint8_t *)r1.data() + per1 * s, rng1 + per1 * r, per1);
        memcpy((uint8_t *)r2.data() + 128 * (size_t)s, rng2 + 128 * (size_t)r, 128);
        if (!chal_shared) memcpy((uint8_t *)ch.data() + 64 * (size_t)s, chal + 64 * (size_t)r, 64);
    }
    const size_t w1 = MPC_ST1_WORDS(n), w2 = MPC_ST2_WORDS(n);
    std::vector<uint32_t> gsV((size_t)ns * 16, 0), gsAS((size_t)2 * ns * row_len * 8, 0), st1((size_t)ns * w1, 0), st2((size_t)ns * w2, 0), gsT((size_t)2 * ns * 16, 0),
        stat(ns, 0);
    for (uint32_t s = 0; s < ns; s++) mpc_blind_thread(s, n, ns, slot_pos.data(), v.data(), (const uint8_t *)bl.data(), (const uint8_t *)r1.data(), gsV.data(), gsAS.data(), st1.data());
    for (uint32_t t = 0; t < ns * n; t++) mpc_bits_thread(t, n, ns, slot_pos.data(), v.data(), (const uint8_t *)r1.data(), gsAS.data(), st1.data());
    for (uint32_t s = 0; s < ns; s++)
        mpc_poly_thread(s, n, ns, slot_pos.data(), st1.data(), (const uint8_t *)ch.data(), chal_shared, (const uint8_t *)r2.data(), st2.data(), gsT.data(), stat.data());
    // back to caller order, then step 3 as the library runs it: lane = row
    std::vector<uint32_t> st2r((size_t)nrows * w2), sh((size_t)nrows * 8 * (3 + 2 * n), 0), xw((x_shared ? 1 : nrows) * 8);
    memcpy(xw.data(), xs, xw.size() * 4);
    for (uint32_t r = 0; r < nrows; r++) {
        const uint32_t s = row_slot[r];
        memcpy(st2r.data() + (size_t)r * w2, st2.data() + (size_t)s * w2, w2 * 4);
        memcpy(rows_v + 64 * (size_t)r, gsV.data() + 16 * (size_t)s, 64);
        memcpy(rows_as + 64 * row_len * r, gsAS.data() + (size_t)s * row_len * 8, 32 * row_len);
        memcpy(rows_as + 64 * row_len * r + 32 * row_len, gsAS.data() + (size_t)(ns + s) * row_len * 8, 32 * row_len);
        memcpy(rows_t + 128 * (size_t)r, gsT.data() + 16 * (size_t)s, 64);
        memcpy(rows_t + 128 * (size_t)r + 64, gsT.data() + 16 * (size_t)(ns + s), 64);
        memcpy(coeffs + 96 * (size_t)r, st2.data() + (size_t)s * w2 + 8 * MPC2_T0, 96);
        status2[r] = (uint8_t)stat[s];
    }
    std::vector<uint8_t> s3(nrows, 0xff);
    for (uint32_t r = 0; r < nrows; r++) {
        if (status2[r]) continue;
        mpc_share_thread(r, n, st2r.data(), (const uint8_t *)xw.data(), x_shared, sh.data(), s3.data());
    }
    memcpy(shares, sh.data(), sh.size() * 4);
    memcpy(status3, s3.data(), nrows);
    return (int)ns;
}

// the dealer's step-6 bodies for nsessions sessions of shape (n, m): sums [nsessions][3][32], bad [nsessions][m], a_vec, b_vec, Hf [nsessions][n m][32]
int mh_dealer(uint32_t n, uint32_t m, uint32_t nsessions, const uint8_t *shares, const uint8_t *ys, uint8_t *sums, uint8_t *bad, uint8_t *a_vec, uint8_t *b_vec,
              uint8_t *Hf) {
    const size_t share_len = 32 * (3 + 2 * (size_t)n), nm = (size_t)n * m;
    std::vector<uint32_t> sh(nsessions * m * share_len / 4), yinv((size_t)nsessions * 8), av(nsessions * nm * 8), bv(nsessions * nm * 8), gf(nsessions * nm * 8),
        hf(nsessions * nm * 8);
    std::vector<uint8_t> skip(nsessions, 0);
    memcpy(sh.data(), shares, sh.size() * 4);
    for (uint32_t p = 0; p < nsessions; p++) {
        sc t_x, t_x_bl, e_bl, y, yi;
        if (!mpc_sum_shares(n, m, (const uint8_t *)sh.data() + p * m * share_len, t_x, t_x_bl, e_bl, bad + (size_t)p * m)) skip[p] = 1;
        memcpy(sums + 96 * (size_t)p, t_x.v, 32);
        memcpy(sums + 96 * (size_t)p + 32, t_x_bl.v, 32);
        memcpy(sums + 96 * (size_t)p + 64, e_bl.v, 32);
        memcpy(y.v, ys + 32 * (size_t)p, 32);
        sc_invert_safegcd(yi, y);
        memcpy(yinv.data() + 8 * (size_t)p, yi.v, 32);
    }
    for (uint32_t t = 0; t < nsessions * nm; t++)
        mpc_vectors_thread(t, n, m, (const uint8_t *)sh.data(), yinv.data(), skip.data(), av.data(), bv.data(), gf.data(), hf.data());
    for (size_t i = 0; i < gf.size(); i += 8)
        if (gf[i] != 1 || gf[i + 1] | gf[i + 2] | gf[i + 3] | gf[i + 4] | gf[i + 5] | gf[i + 6] | gf[i + 7]) return -1;   // G_factors = 1
    memcpy(a_vec, av.data(), av.size() * 4);
    memcpy(b_vec, bv.data(), bv.size() * 4);
    memcpy(Hf, hf.data(), hf.size() * 4);
    return 0;
}

}  // extern "C"
