// The PARTY side of the multi-party aggregation protocol (src/range_proof/party.rs), batched and stateless: rows are independent
// parties of one bitsize n, each with its own position j -- rows of many sessions with different m share a call.
//     step 1  Party::new + assign_position_with_rng (party.rs:37-144):  V_j, A_j, S_j                      -> state1
//     step 2  apply_challenge_with_rng (party.rs:182-237):  l(X), r(X), t(X); T_1_j, T_2_j      state1     -> state2
//     step 3  PartyAwaitingPolyChallenge::apply_challenge (party.rs:279-311):  the proof share   state2     -> share
// The typestate structs of the reference travel as caller-held blobs (layouts below; private to the library).
//
// The per-position walk.  V_j, A_j, S_j, T_1_j, T_2_j are multiscalar multiplications over B~, B and PARTY j's SHARE G_j(n), H_j(n) of
// the generator tables: 2n + 2 terms whatever j and party_capacity are.  The table walk wants the 64 lanes of a wavefront on one
// sub-table per step, so rows are grouped by position on the host (positions are public): mpc_plan_slots gives every position a run
// of slots padded to whole wavefronts, the device works in slot order, and the host puts the results back in the caller's order.
// A wavefront then reads ONE id list, that of its position (mpc_fill_ids: row j of a [party_capacity][2n + 2] table).
#ifndef BPGPU_MPC_PARTY_H
#define BPGPU_MPC_PARTY_H
#include "rp_prover.h"

namespace bp {

#define MPC_WAVE 64u
#define MPC_NO_ROW 0xffffffffu
#define MPC_MAGIC1 0x3143504du   // "MPC1"
#define MPC_MAGIC2 0x3243504du   // "MPC2"
// per-row status of the party and dealer entry points (include/bpgpu.h BPGPU_MPC_*)
#define MPC_ST_OK 0u
#define MPC_ST_MALICIOUS_DEALER 1u
#define MPC_ST_MALFORMED_SHARES 2u
#define MPC_ST_BAD_SCALAR 3u
#define MPC_ST_BAD_POINT 4u

// state1 (PartyAwaitingBitChallenge): header [magic, n, j, 0, v lo, v hi, 0, 0], then v_blinding, a_blinding, s_blinding, s_L[n], s_R[n]
#define MPC_ST1_WORDS(n) (8u * (4u + 2u * (n)))
enum { MPC1_VBL = 1, MPC1_ABL, MPC1_SBL, MPC1_SL };
// state2 (PartyAwaitingPolyChallenge): header [magic, n, j, 0 ...], then offset_zz, v_blinding, a_blinding, s_blinding, t_1_blinding,
// t_2_blinding, t_0, t_1, t_2, l0[n], l1[n], r0[n], r1[n]
#define MPC_ST2_WORDS(n) (8u * (10u + 4u * (n)))
enum { MPC2_OZZ = 1, MPC2_VBL, MPC2_ABL, MPC2_SBL, MPC2_T1B, MPC2_T2B, MPC2_T0, MPC2_T1, MPC2_T2, MPC2_L0 };

// ---- grouping by position (pure host logic) ---------------------------------------------------------------------------------
// row_slot[r]: the slot of caller row r; slot_row[s]: the caller row of slot s or MPC_NO_ROW (padding); blk_pos[b]: the position
// of the wavefront-sized block b of slots.  Rows keep their order inside a position.  Returns the number of slots (a multiple of
// MPC_WAVE).  Positions must be < npos (checked by the caller).
inline uint32_t mpc_plan_slots(uint32_t nrows, const uint32_t *pos, uint32_t npos, uint32_t *row_slot, uint32_t *slot_row /*cap: see mpc_plan_cap*/,
                               uint32_t *blk_pos) {
    uint32_t next = 0;
    for (uint32_t j = 0; j < npos; j++) {
        const uint32_t first = next;
        for (uint32_t r = 0; r < nrows; r++)
            if (pos[r] == j) {
                row_slot[r] = next;
                slot_row[next++] = r;
            }
        if (next == first) continue;
        while (next % MPC_WAVE) slot_row[next++] = MPC_NO_ROW;
        for (uint32_t b = first / MPC_WAVE; b < next / MPC_WAVE; b++) blk_pos[b] = j;
    }
    return next;
}
// slots mpc_plan_slots can need for nrows rows over npos positions
inline uint64_t mpc_plan_cap(uint64_t nrows, uint64_t npos) {
    const uint64_t groups = nrows < npos ? nrows : npos;
    return ((nrows + MPC_WAVE - 1) / MPC_WAVE + groups) * MPC_WAVE;
}
// the generator ids of party j's 2n + 2 terms (B~, B, G_j(n), H_j(n)) in the loaded set (as gen_ids_for)
inline void mpc_fill_ids(uint32_t *ids, uint32_t n, uint32_t j, uint32_t gens_capacity, uint32_t party_capacity) {
    const uint32_t tot = gens_capacity * party_capacity;
    ids[0] = 0;
    ids[1] = 1;
    for (uint32_t i = 0; i < n; i++) {
        ids[2 + i] = 2 + j * gens_capacity + i;
        ids[2 + n + i] = 2 + tot + j * gens_capacity + i;
    }
}

// ---- where a party's draws come from ----------------------------------------------------------------------------------------
// draw(r, s, d) = the d-th random scalar of the step for the party in slot s (the reference's order: step 1 a_blinding, s_blinding,
// s_L[0..n), s_R[0..n) (party.rs:87-118); step 2 t_1_blinding, t_2_blinding (party.rs:224-227)).  Either pre-expanded bytes, `ndraws`
// draws of 64 bytes per slot (bpgpu_mpc_party_*), or the party's ChaChaRng: a 32-byte seed and the block index of the step's first draw
// per slot (bpgpu_mpc_party_*_seeded) -- the lane that consumes a draw computes its keystream block (rpp_draw), no buffer of draws exists.
struct mpc_from_bytes {
    const uint8_t *rng;      // [slot][ndraws][64]
    uint32_t ndraws;
    BP_HD void draw(sc &r, uint32_t s, uint64_t d) const { rpp_wide(r, rng + (uint64_t)s * 64 * ndraws + 64 * d); }
};
struct mpc_from_seed {
    const uint8_t *seeds;    // [slot][32]
    const uint64_t *base;    // [slot]: the 64-bit block counter of draw 0 (the host has checked that base + draws does not wrap)
    BP_HD void draw(sc &r, uint32_t s, uint64_t d) const { rpp_draw(r, seeds + 32 * (uint64_t)s, base[s] + d); }
};

// ---- step 1 ------------------------------------------------------------------------------------------------------------------
// Scalar rows: gsV [nslots][2] (B~, B); gsAS [2 nslots][2n + 2]: row s = A, row nslots + s = S.  All pre-zeroed.
// lane = slot: header, blindings, the V row, the blinding terms of A and S
template <class Src>
BP_HD void mpc_blind_lane(uint32_t s, uint32_t n, uint32_t nslots, const uint32_t *slot_pos, const uint64_t *values, const uint8_t *blindings, const Src &src,
                          uint32_t *gsV, uint32_t *gsAS, uint32_t *st1) {
    const uint32_t j = slot_pos[s];
    if (j == MPC_NO_ROW) return;
    uint32_t *st = st1 + (uint64_t)s * MPC_ST1_WORDS(n);
    const uint64_t v = values[s];
    st[0] = MPC_MAGIC1;
    st[1] = n;
    st[2] = j;
    st[3] = 0;
    st[4] = (uint32_t)v;
    st[5] = (uint32_t)(v >> 32);
    st[6] = 0;
    st[7] = 0;
    const uint32_t row_len = 2 * n + 2;
    sc x;
    uint32_t w[16];
    load_words8(w, blindings + (uint64_t)s * 32);
    for (int q = 8; q < 16; q++) w[q] = 0;
    sc_from_wide(x, w);                                           // Scalar given by the caller, reduced mod l
    ippc_st(st + 8 * MPC1_VBL, x);
    ippc_st(gsV + (uint64_t)s * 16, x);                           // v_blinding on B_blinding
    sc vs;
    sc_0(vs);
    vs.v[0] = (uint32_t)v;
    vs.v[1] = (uint32_t)(v >> 32);
    ippc_st(gsV + (uint64_t)s * 16 + 8, vs);                      // v on B
    src.draw(x, s, 0);
    ippc_st(st + 8 * MPC1_ABL, x);
    ippc_st(gsAS + (uint64_t)s * row_len * 8, x);
    src.draw(x, s, 1);
    ippc_st(st + 8 * MPC1_SBL, x);
    ippc_st(gsAS + (uint64_t)(nslots + s) * row_len * 8, x);
}
BP_HD void mpc_blind_thread(uint32_t s, uint32_t n, uint32_t nslots, const uint32_t *slot_pos, const uint64_t *values, const uint8_t *blindings,
                            const uint8_t *rng, uint32_t *gsV, uint32_t *gsAS, uint32_t *st1) {
    mpc_blind_lane(s, n, nslots, slot_pos, values, blindings, mpc_from_bytes{rng, 2 * n + 2}, gsV, gsAS, st1);
}
// lane = (slot, bit i): a_L on G_{j,i}, a_R = a_L - 1 on H_{j,i}; s_L, s_R (party.rs:99-124)
template <class Src>
BP_HD void mpc_bits_lane(uint32_t tid, uint32_t n, uint32_t nslots, const uint32_t *slot_pos, const uint64_t *values, const Src &src, uint32_t *gsAS,
                         uint32_t *st1) {
    const uint32_t s = tid / n, i = tid - s * n;
    if (slot_pos[s] == MPC_NO_ROW) return;
    const bool bit = (values[s] >> i) & 1;
    const uint32_t row_len = 2 * n + 2;
    uint32_t *rowA = gsAS + (uint64_t)s * row_len * 8, *rowS = gsAS + (uint64_t)(nslots + s) * row_len * 8;
    uint32_t *st = st1 + (uint64_t)s * MPC_ST1_WORDS(n);
    sc one, m1, zero, x;
    sc_from_u32(one, 1);
    sc_0(zero);
    sc_neg(m1, one);
    ippc_st(rowA + 8 * (2 + i), bit ? one : zero);
    ippc_st(rowA + 8 * (2 + n + i), bit ? zero : m1);
    src.draw(x, s, 2 + (uint64_t)i);
    ippc_st(rowS + 8 * (2 + i), x);
    ippc_st(st + 8 * (MPC1_SL + i), x);
    src.draw(x, s, 2 + (uint64_t)(n + i));
    ippc_st(rowS + 8 * (2 + n + i), x);
    ippc_st(st + 8 * (MPC1_SL + n + i), x);
}
BP_HD void mpc_bits_thread(uint32_t tid, uint32_t n, uint32_t nslots, const uint32_t *slot_pos, const uint64_t *values, const uint8_t *rng,
                           uint32_t *gsAS, uint32_t *st1) {
    mpc_bits_lane(tid, n, nslots, slot_pos, values, mpc_from_bytes{rng, 2 * n + 2}, gsAS, st1);
}

// ---- step 2 ------------------------------------------------------------------------------------------------------------------
// lane = slot: l(X) = l0 + l1 X, r(X) = r0 + r1 X, t(X) = <l, r> with the offsets y^(jn), z^2 z^j of the row's position
// (party.rs:189-222, the body of rpp_poly_thread), t_1_blinding, t_2_blinding; the T rows gsT [2 nslots][2]: row s = T_1, nslots + s = T_2.
// chal: y, z per slot (64 bytes) or one pair.  st2, gsT, status pre-zeroed: a rejected row leaves zeros.
template <class Src>
BP_HD void mpc_poly_lane(uint32_t s, uint32_t n, uint32_t nslots, const uint32_t *slot_pos, const uint32_t *st1, const uint8_t *chal, uint32_t chal_shared,
                         const Src &src, uint32_t *st2, uint32_t *gsT, uint32_t *status) {
    if (slot_pos[s] == MPC_NO_ROW) return;
    const uint32_t *a = st1 + (uint64_t)s * MPC_ST1_WORDS(n);
    uint32_t *o = st2 + (uint64_t)s * MPC_ST2_WORDS(n);
    const uint32_t j = a[2];
    const uint64_t v = (uint64_t)a[4] | ((uint64_t)a[5] << 32);
    const uint8_t *ch = chal + (chal_shared ? 0 : (uint64_t)s * 64);
    sc y, z;
    load_words8(y.v, ch);
    load_words8(z.v, ch + 32);
    if (!sc_is_canonical_sc(y) || !sc_is_canonical_sc(z)) {
        status[s] = MPC_ST_BAD_SCALAR;
        return;
    }
    sc zz, one, exp_y, ozz, exp_2, t0, t1, t2;
    sc_mul(zz, z, z);
    sc_from_u32(one, 1);
    sc yn = y;
    for (uint32_t b = 1; b < n; b <<= 1) sc_mul(yn, yn, yn);      // y^n, n a power of two
    exp_y = one;
    ozz = zz;
    for (uint32_t q = 0; q < j; q++) {
        sc_mul(exp_y, exp_y, yn);                                 // y^(j n)
        sc_mul(ozz, ozz, z);                                      // z^2 z^j
    }
    exp_2 = one;
    sc_0(t0);
    sc_0(t1);
    sc_0(t2);
    for (uint32_t i = 0; i < n; i++) {
        sc aL, aR, l0, l1, r0, r1, tt, tu, ls, rs;
        sc_0(aL);
        aL.v[0] = (uint32_t)((v >> i) & 1);
        sc_sub(aR, aL, one);
        sc_sub(l0, aL, z);
        ippc_ld(l1, a + 8 * (MPC1_SL + i));
        sc_add(tt, aR, z);
        sc_mul(tt, exp_y, tt);
        sc_mul(tu, ozz, exp_2);
        sc_add(r0, tt, tu);
        ippc_ld(r1, a + 8 * (MPC1_SL + n + i));
        sc_mul(r1, exp_y, r1);
        ippc_st(o + 8 * (MPC2_L0 + i), l0);
        ippc_st(o + 8 * (MPC2_L0 + n + i), l1);
        ippc_st(o + 8 * (MPC2_L0 + 2 * n + i), r0);
        ippc_st(o + 8 * (MPC2_L0 + 3 * n + i), r1);
        sc_mul(tt, l0, r0);
        sc_add(t0, t0, tt);
        sc_mul(tt, l1, r1);
        sc_add(t2, t2, tt);
        sc_add(ls, l0, l1);
        sc_add(rs, r0, r1);
        sc_mul(tt, ls, rs);
        sc_add(t1, t1, tt);
        sc_mul(exp_y, exp_y, y);
        sc_add(exp_2, exp_2, exp_2);
    }
    sc_sub(t1, t1, t0);
    sc_sub(t1, t1, t2);                                           // (util.rs VecPoly1::inner_product)
    o[0] = MPC_MAGIC2;
    o[1] = n;
    o[2] = j;
    for (int q = 3; q < 8; q++) o[q] = 0;
    sc x;
    ippc_st(o + 8 * MPC2_OZZ, ozz);
    ippc_ld(x, a + 8 * MPC1_VBL);
    ippc_st(o + 8 * MPC2_VBL, x);
    ippc_ld(x, a + 8 * MPC1_ABL);
    ippc_st(o + 8 * MPC2_ABL, x);
    ippc_ld(x, a + 8 * MPC1_SBL);
    ippc_st(o + 8 * MPC2_SBL, x);
    ippc_st(o + 8 * MPC2_T0, t0);
    ippc_st(o + 8 * MPC2_T1, t1);
    ippc_st(o + 8 * MPC2_T2, t2);
    src.draw(x, s, 0);
    ippc_st(o + 8 * MPC2_T1B, x);
    ippc_st(gsT + (uint64_t)s * 16, x);                           // T_1 = t_1 B + t_1_blinding B~ (party.rs:224-227)
    ippc_st(gsT + (uint64_t)s * 16 + 8, t1);
    src.draw(x, s, 1);
    ippc_st(o + 8 * MPC2_T2B, x);
    ippc_st(gsT + (uint64_t)(nslots + s) * 16, x);
    ippc_st(gsT + (uint64_t)(nslots + s) * 16 + 8, t2);
}
BP_HD void mpc_poly_thread(uint32_t s, uint32_t n, uint32_t nslots, const uint32_t *slot_pos, const uint32_t *st1, const uint8_t *chal, uint32_t chal_shared,
                           const uint8_t *rng, uint32_t *st2, uint32_t *gsT, uint32_t *status) {
    mpc_poly_lane(s, n, nslots, slot_pos, st1, chal, chal_shared, mpc_from_bytes{rng, 2}, st2, gsT, status);
}

// ---- step 3 ------------------------------------------------------------------------------------------------------------------
// lane = row (no grouping: no table walk here): the share t_x, t_x_blinding, e_blinding, l_vec, r_vec at x (party.rs:279-311).
// x == 0 -> MaliciousDealer (party.rs:283-285), a non-canonical x -> BAD_SCALAR; both leave the (pre-zeroed) share zero.
BP_HD void mpc_share_thread(uint32_t r, uint32_t n, const uint32_t *st2, const uint8_t *xs, uint32_t x_shared, uint32_t *shares, uint8_t *status) {
    const uint32_t *a = st2 + (uint64_t)r * MPC_ST2_WORDS(n);
    uint32_t *o = shares + (uint64_t)r * 8 * (3 + 2 * n);
    sc x;
    load_words8(x.v, xs + (x_shared ? 0 : (uint64_t)r * 32));
    if (!sc_is_canonical_sc(x)) {
        status[r] = (uint8_t)MPC_ST_BAD_SCALAR;
        return;
    }
    if (words8_zero(x.v)) {
        status[r] = (uint8_t)MPC_ST_MALICIOUS_DEALER;
        return;
    }
    sc p, q, u;
    ippc_ld(p, a + 8 * MPC2_T2);                                  // t_x = t0 + x (t1 + x t2)
    sc_mul(p, x, p);
    ippc_ld(q, a + 8 * MPC2_T1);
    sc_add(p, p, q);
    sc_mul(p, x, p);
    ippc_ld(q, a + 8 * MPC2_T0);
    sc_add(p, p, q);
    ippc_st(o, p);
    ippc_ld(p, a + 8 * MPC2_T2B);                                 // t_x_blinding = z^2 z^j v_blinding + x (t1_blinding + x t2_blinding)
    sc_mul(p, x, p);
    ippc_ld(q, a + 8 * MPC2_T1B);
    sc_add(p, p, q);
    sc_mul(p, x, p);
    ippc_ld(q, a + 8 * MPC2_OZZ);
    ippc_ld(u, a + 8 * MPC2_VBL);
    sc_mul(q, q, u);
    sc_add(p, p, q);
    ippc_st(o + 8, p);
    ippc_ld(p, a + 8 * MPC2_SBL);                                 // e_blinding = a_blinding + x s_blinding
    sc_mul(p, p, x);
    ippc_ld(q, a + 8 * MPC2_ABL);
    sc_add(p, p, q);
    ippc_st(o + 16, p);
    for (uint32_t i = 0; i < n; i++) {
        ippc_ld(p, a + 8 * (MPC2_L0 + n + i));
        sc_mul(p, p, x);
        ippc_ld(q, a + 8 * (MPC2_L0 + i));
        sc_add(p, p, q);
        ippc_st(o + 8 * (3 + i), p);
        ippc_ld(p, a + 8 * (MPC2_L0 + 3 * n + i));
        sc_mul(p, p, x);
        ippc_ld(q, a + 8 * (MPC2_L0 + 2 * n + i));
        sc_add(p, p, q);
        ippc_st(o + 8 * (3 + n + i), p);
    }
    status[r] = (uint8_t)MPC_ST_OK;
}

}  // namespace bp
#endif
