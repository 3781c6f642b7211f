// Signed sums of Pedersen commitments, and the balance check over them: for every row r of a batch
//     S_r = sum_{sign 0} C_i - sum_{sign 1} C_i   over the row's terms (32-byte Ristretto encodings, one flat array, CSR offsets),
//     O_r = value_r B + blinding_r B_blinding      (both optional; the context's bases, walked as pedersen.h walks them),
// the sum form stores compress(S_r + O_r), the balance form tells whether S_r == O_r (the coset identity test on S_r - O_r: nothing
// is compressed, no inversion is taken).  What a validator of confidential transactions does next to the range proofs
// (sum V_in - sum V_out - fee B == excess), and what a wallet does to a committed balance (C' = C + v B + r B_blinding).
//
// The cost of a term is its decode (an inverse square root, ~250 squarings); the additions are cheap beside it.  So:
//   1. term launch, lane = term, workgroup = PSUM_BLOCK consecutive terms: decode (ristretto_decompress_lp), negate for sign 1, park the
//      point in LDS, then a SEGMENTED reduction in log2(PSUM_BLOCK) steps -- at distance d a lane adds its neighbour only when both
//      belong to the same row (rows are contiguous, so the lanes between them do too); after the last step the first lane of every
//      row segment of the workgroup holds that segment's sum and stores it: ONE partial point per (workgroup, row) pair, at a slot
//      the HOST computed from the offsets (psum_make_plan).  A failed decode raises the row's flag byte (a plain store of 1: racing
//      writers store the same value).
//   2. reduce passes, only while some row has more than PSUM_SERIAL_MAX partials: the same body over the partials of the pass
//      before (extended coordinates instead of encodings), their own offsets being the slot table of that pass.
//   3. finish launch, lane = row: the opening O_r from the window tables (or the identity when neither scalar is given), negated in
//      the balance form, plus the row's <= PSUM_SERIAL_MAX partials; ped_encode, or ge_is_identity.
// Nothing crosses between workgroups inside a launch; the launches are the only hand-off.
//
// Each phase between two barriers is a lane body over (block-local lane, LDS pointers), so that the CPU harness
// (tests/pedersen_sum_harness) runs a workgroup phase by phase.
#ifndef BPGPU_PEDERSEN_SUM_H
#define BPGPU_PEDERSEN_SUM_H
#include <vector>

#include "pedersen.h"

namespace bp {

#define PSUM_BLOCK 64                        // lanes of a workgroup of the term and reduce launches (== BP_BLOCK, k_pedersen_sum.hip checks)
#define PSUM_SERIAL_MAX (2 * PSUM_BLOCK)     // the most points one lane of the finish launch adds serially
#define PSUM_MAX_PASSES 8                    // 2^28 items shrink below PSUM_SERIAL_MAX in four passes; the table has room for eight
#define PSUM_NO_ROW 0xffffffffu              // a lane behind the last item

// ---- the plan (host) ----------------------------------------------------------------------------------------------------------
// Pass k reads items segmented by off_k[0 .. nbatch] (pass 0: the terms, off_0 = row_offsets) in workgroups of PSUM_BLOCK and writes
// one partial per (workgroup, row) pair.  Enumerated by (workgroup, row) -- which is also by (row, workgroup): a row that continues
// in the next workgroup is the last of this one and the first of the next -- row r's pairs are contiguous and begin at
//     off_{k+1}[r] = sum_{r' < r, r' not empty} (last workgroup of r' - first workgroup of r' + 1),
// so the pair (workgroup b, row r) has slot off_{k+1}[r] + (b - off_k[r] / PSUM_BLOCK): the next pass's segmentation is this pass's
// slot table.  There are at most nblocks + nbatch pairs: a row not empty has one pair plus one per workgroup boundary inside it, and
// the workgroups have nblocks - 1 boundaries.  Returns the largest number of pairs of one row.
inline uint32_t psum_next_offsets(uint32_t nbatch, const uint32_t *off, uint32_t *next) {
    uint32_t s = 0, longest = 0;
    for (uint32_t r = 0; r < nbatch; r++) {
        next[r] = s;
        if (off[r + 1] > off[r]) {
            const uint32_t cnt = (off[r + 1] - 1) / PSUM_BLOCK - off[r] / PSUM_BLOCK + 1;
            s += cnt;
            if (cnt > longest) longest = cnt;
        }
    }
    next[nbatch] = s;
    return longest;
}
struct psum_plan {
    uint32_t nbatch = 0, npasses = 0;    // passes: the term launch and the reduce passes behind it
    std::vector<uint32_t> table;         // [npasses + 1][nbatch + 1]: row k = off_k; the finish reads off_{npasses}
    const uint32_t *off(uint32_t k) const { return table.data() + (size_t)k * (nbatch + 1); }
    uint32_t items(uint32_t k) const { return off(k)[nbatch]; }   // items pass k reads (k < npasses) / partials the finish reads
    uint64_t partials() const {                                   // points of every pass's output together
        uint64_t n = 0;
        for (uint32_t k = 1; k <= npasses; k++) n += items(k);
        return n;
    }
};
// row_offsets: nbatch + 1 values, non-decreasing from 0 (the caller has checked).  A row of more than PSUM_SERIAL_MAX pairs spans more
// than PSUM_SERIAL_MAX - 1 whole workgroups, and a pass turns n > PSUM_SERIAL_MAX items of a row into at most n / PSUM_BLOCK + 2 < n:
// the loop ends, for 2^28 terms after four passes.
inline void psum_make_plan(psum_plan &pl, uint32_t nbatch, const uint32_t *row_offsets) {
    pl.nbatch = nbatch;
    pl.npasses = 0;
    pl.table.assign(row_offsets, row_offsets + nbatch + 1);
    uint32_t longest;
    do {
        pl.table.resize((size_t)(pl.npasses + 2) * (nbatch + 1));
        longest = psum_next_offsets(nbatch, pl.off(pl.npasses), pl.table.data() + (size_t)(pl.npasses + 1) * (nbatch + 1));
        pl.npasses++;
    } while (longest > PSUM_SERIAL_MAX && pl.npasses < PSUM_MAX_PASSES);
}

// ---- the term and reduce launches: lane bodies ------------------------------------------------------------------------------------
struct psum_lds {
    ge_ext *pt;       // [PSUM_BLOCK] the lanes' points, later the sums of the row segments
    uint32_t *row;    // [PSUM_BLOCK] the lanes' rows, PSUM_NO_ROW behind the last item
};
// what a pass reads and writes: items [0, total) segmented by off[0 .. nbatch], partials to slot[r] + (workgroup - off[r] / PSUM_BLOCK)
struct psum_pass {
    uint32_t total, nbatch;
    const uint32_t *off, *slot;
};

// the row of item t < off[nbatch]: the LAST r with off[r] <= t (empty rows repeat an offset; the last one is the row not empty)
BP_HD uint32_t psum_find_row(uint32_t t, const uint32_t *off, uint32_t nbatch) {
    uint32_t lo = 0, hi = nbatch;   // off[lo] <= t, and hi == nbatch or off[hi] > t
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}
// ristretto_decompress_lp (ge25519.h) with the one field element that crosses its squaring chain, t = v u2^2, parked in `park` (the
// lane's own slot of the workgroup's points, free until the decode is done) instead of carried through the chain -- what ped_encode
// does for the encoder.  Under the 168-register cap ristretto_decompress_lp alone parks those ten words in scratch (k_bk2_prepare).
// The same result bit for bit (the CPU harness compares it with ristretto_decompress on every class of encoding).
BP_HD bool psum_decode(ge_ext &r, const uint32_t *src /*8 words, read twice*/, fe *park) {
    bool canonical = true, s_neg, ok;
    fe I;
    {
        fe tin, v3, v7, raw;
        {
            uint32_t w[8], chk[8];
#pragma unroll
            for (int i = 0; i < 8; i++) w[i] = src[i];
            fe s, u1, u2, v, u2s;
            ristretto_decode_front(s, u1, u2, v, w);
            fe_to_words(chk, s);
#pragma unroll
            for (int i = 0; i < 8; i++) canonical = canonical && (chk[i] == w[i]);
            s_neg = w[0] & 1;
            fe_sq(u2s, u2);
            fe_mul(tin, v, u2s);
        }
        *park = tin;
        fe_sq(v3, tin);            // fe_invsqrt_raw
        fe_mul(v3, v3, tin);
        fe_sq(v7, v3);
        fe_mul(v7, v7, tin);
        fe_pow22523(raw, v7);
        ped_reload(tin, park);
        fe_sq(v3, tin);
        fe_mul(v3, v3, tin);
        fe_mul(raw, raw, v3);
        ok = fe_invsqrt_fix(I, raw, tin);
    }
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = src[i];
#pragma unroll
    for (int i = 0; i < 8; i++) BP_OPAQUE2(w[i], I.v[0]);
    fe s, u1, u2, v, Dx, Dy, t;
    ristretto_decode_front(s, u1, u2, v, w);
    fe_mul(Dx, I, u2);
    fe_mul(Dy, I, Dx);
    fe_mul(Dy, Dy, v);
    fe_add(t, s, s);
    fe_mul(r.X, t, Dx);
    fe_abs(r.X);
    fe_mul(r.Y, u1, Dy);
    fe_1(r.Z);
    fe_mul(r.T, r.X, r.Y);
    return canonical && !s_neg && ok && !fe_isneg(r.T) && !fe_iszero(r.Y);
}
// phase 0 of the term launch: decode, negate for sign 1 (bit 0 of the byte; signs == nullptr: every term is added), park.  A point
// that does not decode is parked as it came out -- field elements all the same -- and its row is flagged: the row's sum is void.
BP_HD void psum_load_term(uint32_t lane, uint32_t block, const psum_pass &ps, const uint32_t *points, const uint8_t *signs, uint8_t *bad, const psum_lds &l) {
    const uint64_t t = (uint64_t)block * PSUM_BLOCK + lane;
    if (t >= ps.total) {
        l.row[lane] = PSUM_NO_ROW;
        return;
    }
    const uint32_t r = psum_find_row((uint32_t)t, ps.off, ps.nbatch);
    ge_ext p;
    if (!psum_decode(p, points + 8 * t, &l.pt[lane].X)) bad[r] = 1;
    const bool neg = signs && (signs[t] & 1);
    fe_cneg(p.X, neg);
    fe_cneg(p.T, neg);
    l.pt[lane] = p;
    l.row[lane] = r;
}
// phase 0 of a reduce pass: the item is a partial of the pass before
BP_HD void psum_load_partial(uint32_t lane, uint32_t block, const psum_pass &ps, const ge_ext *src, const psum_lds &l) {
    const uint64_t t = (uint64_t)block * PSUM_BLOCK + lane;
    if (t >= ps.total) {
        l.row[lane] = PSUM_NO_ROW;
        return;
    }
    l.pt[lane] = src[t];
    l.row[lane] = psum_find_row((uint32_t)t, ps.off, ps.nbatch);
}
// One step of the segmented reduction, distance d = 1, 2, .. PSUM_BLOCK / 2, in two phases with a barrier between them: every lane
// reads (its point, the point d lanes on) and adds; then every lane that added stores.  After the step of distance d, lane i holds the
// sum of lanes [i, min(i + 2 d, end of its row segment)).  ge_add is complete: P + P and P + (-P) need no care.
BP_HD bool psum_step_add(uint32_t lane, uint32_t d, const psum_lds &l, ge_ext &sum) {
    const bool on = lane + d < PSUM_BLOCK && l.row[lane] != PSUM_NO_ROW && l.row[lane + d] == l.row[lane];
    if (on) ge_add(sum, l.pt[lane], l.pt[lane + d]);
    return on;
}
BP_HD void psum_step_store(uint32_t lane, const psum_lds &l, const ge_ext &sum, bool on) {
    if (on) l.pt[lane] = sum;
}
// the last phase: the first lane of every row segment stores the segment's sum at the pair's slot
BP_HD void psum_store_partial(uint32_t lane, uint32_t block, const psum_pass &ps, const psum_lds &l, ge_ext *partial) {
    const uint32_t r = l.row[lane];
    if (r == PSUM_NO_ROW || (lane != 0 && l.row[lane - 1] == r)) return;
    partial[(uint64_t)ps.slot[r] + (block - ps.off[r] / PSUM_BLOCK)] = l.pt[lane];
}

// ---- the finish launch: lane = row ------------------------------------------------------------------------------------------------
// The lane sums the row's partials FIRST and walks the tables onto that sum: the walk and the encoder then run exactly as in
// ped_commit_lane, with nothing of the partials' loop alive beside them (the other order -- the opening, then the partials -- spills
// 4 registers under the 168-register cap).  Addition commutes: the bytes do not depend on the order.
// acc = the sum of the row's partials [slot[r], slot[r + 1]), at most PSUM_SERIAL_MAX of them (psum_make_plan); false (and the
// identity) when the row has none.  NEG: minus that sum, every partial subtracted (the balance form; negating the finished sum
// instead spills 3 registers around this loop).
template <bool NEG>
BP_HD bool psum_row_partials(ge_ext &acc, uint32_t r, const uint32_t *slot, const ge_ext *partial) {
    const uint32_t s0 = slot[r], s1 = slot[r + 1];
    if (s0 == s1) {
        ge_identity(acc);
        return false;
    }
    if (NEG) ge_neg(acc, partial[s0]);
    else acc = partial[s0];
    for (uint32_t s = s0 + 1; s < s1; s++) {
        ge_cached c;
        ge_to_cached(c, partial[s]);
        ge_add_cached(acc, acc, c, NEG);
    }
    return true;
}
// acc += value_r B + blinding_r B_blinding: ped_point's loop (pedersen.h) with either scalar optional -- there a missing blinding is
// DRAWN, here it is zero, and which scalars a call carries is public.  started: acc already holds a point (ped_step then adds to it
// from the first digit on).  CT: the constant-time walk over the W = 4 table.  Returns whether the scalars given are canonical; a
// rejected row walks too.
template <bool CT>
BP_HD bool psum_add_opening(ge_ext &acc, bool started, uint32_t r, const ped_in &in, const ped_park &pk, fb_params prm, const uint32_t *gen_ids,
                            const fb_entry *table) {
    bool ok = true;
#pragma unroll 1
    for (uint32_t term = 0; term < 2; term++) {
        if (!(term == 0 ? in.blindings : in.values)) continue;
        uint32_t s[8];
        if (term == 0) ped_load_blinding(r, in, s, nullptr);
        else ped_load_value(r, in, s);
        ok = ok & sc_is_canonical(s);
        const uint32_t nw = term == 0 ? prm.nwin : ped_value_windows(prm, in.value_words);
        if (CT) ped_walk_ct(acc, pk, s, nw, gen_ids[term], prm, table);
        else ped_walk(acc, started, pk, s, nw, gen_ids[term], prm, table);
    }
    return ok;
}
// sum form: 8 words out (zeros for a rejected row) and the row's BPGPU_MSM_* byte; a scalar not canonical takes precedence over a point
// that does not decode, as in ped_open_lane
template <bool CT>
BP_HD void psum_sum_lane(uint32_t r, ped_in in, ped_park pk, fb_params prm, const uint32_t *gen_ids, const fb_entry *table, const uint32_t *slot,
                         const ge_ext *partial, const uint8_t *bad, uint32_t *out_words, uint8_t *status) {
    ge_ext acc;
    const bool started = psum_row_partials<false>(acc, r, slot, partial);
    const bool ok = psum_add_opening<CT>(acc, started, r, in, pk, prm, gen_ids, table);
    uint32_t w[8];
    ped_encode(w, acc, pk);
    // the words are masked, not selected: with a select on the row's flag the compiler moves the encoder under a branch on it, and the
    // kernel then spills 25 registers under the 168-register cap
    const uint32_t b = bad[r], m = 0u - (uint32_t)(ok & (b == 0));
#pragma unroll
    for (int q = 0; q < 8; q++) out_words[8 * (uint64_t)r + q] = w[q] & m;
    status[r] = !ok ? (uint8_t)BP_STATUS_BAD_SCALAR : (b ? (uint8_t)BP_STATUS_BAD_POINT : (uint8_t)BP_STATUS_OK);
}
// balance form: verdict 0 = S_r == O_r as Ristretto elements (X == 0 or Y == 0 on O_r - S_r), 1 = it does not balance, or a term does
// not decode (a None of optional_multiscalar_mul), 2 = a scalar is not canonical.  Variable time: its inputs are public to the verifier.
BP_HD void psum_balance_lane(uint32_t r, ped_in in, ped_park pk, fb_params prm, const uint32_t *gen_ids, const fb_entry *table, const uint32_t *slot,
                             const ge_ext *partial, const uint8_t *bad, uint8_t *verdict) {
    ge_ext acc;
    const bool started = psum_row_partials<true>(acc, r, slot, partial);   // -S_r
    const bool ok = psum_add_opening<false>(acc, started, r, in, pk, prm, gen_ids, table);
    const bool balanced = ge_is_identity(acc);
    const uint32_t b = bad[r];
    verdict[r] = (uint8_t)(!ok ? 2u : (uint32_t)((b != 0) | !balanced));
}

}  // namespace bp
#endif
