// Proofs of recorded linear relations between points, in batches (include/bpgpu.h, bpgpu_sigma_*): the sigma protocol of opening.h
// over any set of equations   slot[lhs_k] = sum_t x[sec_{k,t}] Base[base_{k,t}] ,   k < E ,
// with S secret scalars, P instance points per row and bases that are either shared (a row of the context's window tables:
// 0 = B_blinding, 1 = B, 2 + i = G_i of party 0) or an instance slot of the row (16 + p).  The relation is recorded once (sig_rel, in
// device memory: every lane reads the same words) and batches are proved and verified against the record.
// Transcript, on the caller's own state at any STROBE position (sig_bind, then the commitments and the challenge):
//   append_message("dom-sep", "sigmaproof v1"); append_message("stmt", digest); append_point("P", P_i), i < P, as given;
//   validate_and_append_point("T", T_k), k < E  [32 zero bytes: VerificationError, nothing of that T_k absorbed]; c = challenge_scalar("c")
// Prover: k_j = draw j of ChaChaRng::from_seed(seed[row]); T_k = sum_t k[sec] Base; s_j = k_j + c x_j.  proof = T_1 | .. | T_E | s_1 | .. | s_S.
// Check of equation k: sum_t s[sec] Base - c slot[lhs_k] - T_k = identity.
//
// The prover is THREE launches, each a simple lane body (one launch around a barrier, k_opn_create's shape with the product inside, does
// not fit under the 168-register cap: DESIGN 3.12):
//   sig_vb_lane      lane = (instance-base term, row): the per-lane variable-base product k P -- the nonce drawn, the point decoded in
//                    the lane, its multiples P .. 8 P as ge_cached in a lane-fastest global workspace (320 words a lane do not fit in LDS
//                    at three wavefronts per SIMD), a signed 4-bit fixed-window walk from the top window down, the product left as
//                    ge_cached in the workspace.  CT: every window doubles four times, reads all 8 entries, selects by masks, applies
//                    the sign by mask and always adds -- no branch or address depends on the nonce.
//   sig_walk_lane    lane = (equation, row): the shared-base terms through ped_walk / ped_walk_ct, the products added, ped_encode: T_k
//   sig_finish_lane  lane = row: the transcript, the S multiply-adds, the stores
// The products are as secret as partial sums of a T_k: the workspace belongs to the prover's working set, cleared on every exit.
// The verifier's front end (sig_front_lane) replays the transcript and stages one row of the shared-generator chain per (proof, equation):
// U = P + 1 unique terms (slot i with the sum of s over the terms it serves as a base of, - c on the lhs slot, scalar 0 and the identity
// encoding where the equation does not touch it; then (-1, T_k)) and a row of 2 + G generator-table coefficients.  No point is decoded here.
#ifndef BPGPU_SIGMA_H
#define BPGPU_SIGMA_H
#include "opening.h"

namespace bp {

#define SIG_MAX 8u                          // secrets, slots, equations, terms of one equation
#define SIG_MAX_TERMS 32u
#define SIG_BASE_SLOT 16u                   // base ids from here on name instance slots
#define SIG_RLC_WEIGHT_DOMAIN 0x67697377u   // "wsig": the combination weights the caller did not bring
#define SIG_RLC_MAX_TERMS (1u << 24)        // combined terms of one call: nbatch (P + E)
#define SIG_VB_W 4u
#define SIG_VB_ENTRIES 8u                   // P .. 8 P
#define SIG_VB_WINDOWS 64u
#define SIG_VB_WORDS (SIG_VB_ENTRIES * 40u) // words of workspace per lane

struct sig_rel {
    uint32_t S, P, E;
    uint32_t G;           // columns of G_i in a generator row: 1 + the largest i in use (1 where none is)
    uint32_t digest[8];   // of the canonical descriptor bytes
    uint32_t lhs[8];      // slot index of equation k's left-hand side
    uint32_t first[9];    // terms first[k] .. first[k + 1] belong to equation k
    uint32_t sec[32], base[32];
    uint32_t nvb;         // terms on an instance base, in term order
    uint32_t vb_term[32]; // the term of product v
    uint32_t vb_of[32];   // the product of term t (where its base is a slot)
};
BP_HD uint32_t sig_proof_words(const sig_rel &rel) { return 8u * (rel.E + rel.S); }
BP_HD uint32_t sig_uniq(const sig_rel &rel) { return rel.P + 1u; }
BP_HD uint32_t sig_gen_row(const sig_rel &rel) { return 2u + rel.G; }

// The canonical descriptor bytes (include/bpgpu.h) into the record, host side: u8 S, u8 P, u8 E, then per equation u8 lhs, u8 nterms and
// nterms x (u8 secret, u8 base).  gens_capacity bounds the G_i.  Returns null, or what is wrong with the descriptor.
inline const char *sig_rel_parse(const uint8_t *desc, size_t desc_len, size_t gens_capacity, sig_rel &r) {
    r = sig_rel{};
    if (!desc || desc_len < 3) return "descriptor missing or shorter than its header";
    r.S = desc[0], r.P = desc[1], r.E = desc[2];
    if (r.S < 1 || r.S > SIG_MAX || r.P < 1 || r.P > SIG_MAX || r.E < 1 || r.E > SIG_MAX) return "S, P and E must each lie in 1 .. 8";
    size_t at = 3;
    uint32_t nt = 0, sec_used = 0, slot_used = 0, gmax = 0;
    for (uint32_t k = 0; k < r.E; k++) {
        if (at + 2 > desc_len) return "descriptor ends inside an equation";
        const uint32_t lhs = desc[at], n = desc[at + 1];
        at += 2;
        if (lhs < SIG_BASE_SLOT || lhs >= SIG_BASE_SLOT + r.P) return "an lhs must be an instance slot (16 + p, p < P)";
        if (n < 1 || n > SIG_MAX || nt + n > SIG_MAX_TERMS) return "1 .. 8 terms per equation, at most 32 in all";
        if (at + 2 * n > desc_len) return "descriptor ends inside an equation";
        r.lhs[k] = lhs - SIG_BASE_SLOT;
        slot_used |= 1u << r.lhs[k];
        r.first[k] = nt;
        for (uint32_t t = 0; t < n; t++, at += 2) {
            const uint32_t sec = desc[at], b = desc[at + 1];
            if (sec >= r.S) return "a term's secret is out of range";
            if (b >= SIG_BASE_SLOT) {
                if (b >= SIG_BASE_SLOT + r.P) return "a term's instance slot is out of range";
                slot_used |= 1u << (b - SIG_BASE_SLOT);
                r.vb_of[nt] = r.nvb;
                r.vb_term[r.nvb++] = nt;
            } else if (b >= 2) {
                if (b - 2 >= SIG_MAX || b - 2 >= gens_capacity) return "a G_i lies beyond the loaded generators";
                if (b - 1 > gmax) gmax = b - 1;
            }
            sec_used |= 1u << sec;
            r.sec[nt] = sec;
            r.base[nt] = b;
            nt++;
        }
    }
    for (uint32_t k = r.E; k < 9; k++) r.first[k] = nt;
    if (at != desc_len) return "descriptor has bytes beyond its last equation";
    if (sec_used != (1u << r.S) - 1) return "a secret is used in no term";
    if (slot_used != (1u << r.P) - 1) return "an instance slot is used nowhere";
    r.G = gmax ? gmax : 1;
    {   // the digest: Transcript("sigma statement"), append_message("desc", bytes), challenge_bytes("digest", 32)
        uint32_t w[50];
        kstate st;
        st.w = w;
        st.stride = 1;
        strobe t;
        merlin_strobe_init(t, st);
        const uint8_t dsep[7] = {'d', 'o', 'm', '-', 's', 'e', 'p'}, name[15] = {'s', 'i', 'g', 'm', 'a', ' ', 's', 't', 'a', 't', 'e', 'm', 'e', 'n', 't'},
                      ld[4] = {'d', 'e', 's', 'c'}, lg[6] = {'d', 'i', 'g', 'e', 's', 't'};
        uint8_t dg[32];
        merlin_append_message(t, dsep, 7, name, 15);
        merlin_append_message(t, ld, 4, desc, (uint32_t)desc_len);
        merlin_challenge_bytes(t, lg, 6, dg, 32);
        for (int q = 0; q < 8; q++) r.digest[q] = (uint32_t)dg[4 * q] | ((uint32_t)dg[4 * q + 1] << 8) | ((uint32_t)dg[4 * q + 2] << 16) | ((uint32_t)dg[4 * q + 3] << 24);
    }
    return nullptr;
}

// the separator, the statement's digest and the instance points in slot order, absorbed from where they lie
BP_HD void sig_bind(strobe &t, const sig_rel &rel, const uint32_t *pts) {
    const uint8_t dsep[7] = {'d', 'o', 'm', '-', 's', 'e', 'p'}, ls[4] = {'s', 't', 'm', 't'}, lP[1] = {'P'};
    const uint8_t name[13] = {'s', 'i', 'g', 'm', 'a', 'p', 'r', 'o', 'o', 'f', ' ', 'v', '1'};
    merlin_append_message(t, dsep, 7, name, 13);
    merlin_append_words8(t, ls, 4, rel.digest);
    for (uint32_t i = 0; i < rel.P; i++) merlin_append_words8(t, lP, 1, pts + 8 * i);
}

// ---- k P per lane ------------------------------------------------------------------------------------------------------
// the lane's table: word q of entry e ((e + 1) P as ge_cached) at w[(40 e + q) stride]
struct sig_vb_tab {
    uint32_t *w;
    uint32_t stride;
};
// (e + 1) P := p, coordinate by coordinate (ge_to_cached's steps: nothing but the coordinate in hand is held)
BP_HD void sig_tab_store_fe(const sig_vb_tab &tab, uint32_t at, const fe &f) {
#pragma unroll
    for (int q = 0; q < 10; q++) tab.w[(uint64_t)(at + q) * tab.stride] = f.v[q];
}
BP_HD void sig_tab_store(const sig_vb_tab &tab, uint32_t e, const ge_ext &p) {
    const fe d2 = BP_FE_D2;
    fe f;
    fe_add(f, p.Y, p.X);
    fe_carry(f);
    sig_tab_store_fe(tab, 40 * e, f);
    fe_sub(f, p.Y, p.X);
    sig_tab_store_fe(tab, 40 * e + 10, f);
    sig_tab_store_fe(tab, 40 * e + 20, p.Z);
    fe_mul(f, p.T, d2);
    sig_tab_store_fe(tab, 40 * e + 30, f);
}
// coordinate `co` (0: Y+X, 1: Y-X, 2: Z, 3: 2dT) of the entry of digit magnitude a in 0 .. 8 (0: the neutral element (1, 1, 1, 0)), read
// where it is used -- volatile: a fresh read each time, nothing of the table is kept in registers between uses.  CT: all 8 entries are
// read and the one is selected by masks.
template <bool CT>
BP_HD void sig_tab_fe(fe &f, const sig_vb_tab &tab, uint32_t a, uint32_t co) {
    const volatile uint32_t *w = tab.w;
    if (CT) {
#pragma unroll
        for (int q = 0; q < 10; q++) f.v[q] = 0;
#pragma unroll 1
        for (uint32_t e = 0; e < SIG_VB_ENTRIES; e++) {
            const uint32_t m = 0u - (uint32_t)(a == e + 1);
#pragma unroll
            for (int q = 0; q < 10; q++) f.v[q] |= w[(uint64_t)(40 * e + 10 * co + q) * tab.stride] & m;
        }
        f.v[0] |= (co < 3 ? 1u : 0u) & (0u - (uint32_t)(a == 0));
    } else {
#pragma unroll
        for (int q = 0; q < 10; q++) f.v[q] = w[(uint64_t)(40 * (a - 1) + 10 * co + q) * tab.stride];   // (the caller skips a == 0)
    }
}
// r += (neg ? -1 : 1) a P: ge_add_cached with each operand of the entry fetched when its product comes up.  CT: the sign is applied by
// fe_select on both candidates; else it picks which coordinate is read.
template <bool CT>
BP_HD void sig_tab_add(ge_ext &r, const sig_vb_tab &tab, uint32_t a, bool neg) {
    fe t, u, A, B, C, D;
    if (CT) {
        fe ypx, ymx;
        sig_tab_fe<true>(ypx, tab, a, 0);
        sig_tab_fe<true>(ymx, tab, a, 1);
        fe_select(t, ymx, ypx, neg);
        fe_select(u, ypx, ymx, neg);
    } else {
        sig_tab_fe<false>(t, tab, a, neg ? 0u : 1u);
    }
    fe_sub_rr(A, r.Y, r.X);   // lazy (the coordinates of r are reduced)
    fe_mul(A, A, t);
    if (!CT) sig_tab_fe<false>(u, tab, a, neg ? 1u : 0u);
    fe_add(B, r.Y, r.X);      // lazy
    fe_mul(B, B, u);
    sig_tab_fe<CT>(t, tab, a, 3);
    fe_mul(C, r.T, t);
    sig_tab_fe<CT>(t, tab, a, 2);
    fe_mul(D, r.Z, t);
    fe_add(D, D, D);          // lazy (2x)
    fe e, h, dmc, dpc, f, g;
    fe_sub_rr(e, B, A);       // lazy
    fe_add(h, B, A);          // lazy (2x)
    fe_sub(dmc, D, C);
    fe_add(dpc, D, C);        // lazy (3x)
    fe_select(f, dmc, dpc, neg);
    fe_select(g, dpc, dmc, neg);
    fe_mul(r.X, f, e);
    fe_mul(r.Y, h, g);
    fe_mul(r.Z, f, g);
    fe_mul(r.T, h, e);
}
// q = k P for the encoding at pt (read twice); false when it does not decode (public: the walk then runs on the identity).  pk.rw holds
// the recoded scalar (ped_bias_add: the 64 windows of 4 bits are digit + 8, digits in -8 .. 7).
// PRECONDITION: k < 2^253 (every reduced scalar; the callers pass nonces out of rpp_draw).  The bias is 8 (16^64 - 1) / 15 < 0.534 * 2^256, so
// k + bias < 2^256 and nothing carries out of the top window: its nibble is at most 1 + 8 + 1.  A k from about 0.467 * 2^256 on would lose
// that carry silently (the 64 windows hold 256 bits), which is why the bound is asserted where assertions are compiled in.
template <bool CT>
BP_HD bool sig_vb_mul(ge_ext &q, const ped_park &pk, const sig_vb_tab &tab, const uint32_t k[8], const uint32_t *pt) {
    BP_ASSERT((k[7] >> 29) == 0);
    ped_bias_add(pk, k, SIG_VB_W, SIG_VB_WINDOWS);
    const bool ok = ristretto_decompress_lp(q, pt);
    if (!ok) ge_identity(q);
    sig_tab_store(tab, 0, q);
#pragma unroll 1
    for (uint32_t e = 1; e < SIG_VB_ENTRIES; e++) {   // (e + 1) P = e P + P, P read back from entry 0
        sig_tab_add<false>(q, tab, 1, false);
        sig_tab_store(tab, e, q);
    }
    ge_identity(q);
    bool started = false;
#pragma unroll 1
    for (uint32_t i = 0; i < SIG_VB_WINDOWS; i++) {
        const uint32_t win = SIG_VB_WINDOWS - 1 - i;
        if (CT || started) {
            ge_dbl(q, q, false);
            ge_dbl(q, q, false);
            ge_dbl(q, q, false);
            ge_dbl(q, q);
        }
        const int d = (int)ped_window(pk, win, SIG_VB_W) - 8;
        const int sgn = d >> 31;                          // all ones for a negative digit
        const uint32_t a = (uint32_t)((d ^ sgn) - sgn);   // |d| in 0 .. 8
        if (CT) {
            sig_tab_add<true>(q, tab, a, sgn != 0);
        } else if (a != 0) {
            sig_tab_add<false>(q, tab, a, d < 0);
            started = true;
        }
    }
    return ok;
}

// ---- creation ----------------------------------------------------------------------------------------------------------
struct sig_create_in {
    const uint32_t *secrets;   // [row][S][8]
    const uint8_t *seeds;      // [row][32]: ChaChaRng::from_seed; k_j = draw j
    const uint32_t *points;    // [row][P][8]
    const uint32_t *ts_in;     // the callers' states, never null (ts_in_stride words apart)
    uint32_t ts_in_stride, nrows;
};
// the creation's workspace for rows row0 .. row0 + nstride of a batch (a slice), lane fastest:
//   tab  : SIG_VB_WORDS words per lane of the product launch (lane = v nstride + row - row0)
//   prod : word q of product v of a row at prod[(40 v + q) nstride + row - row0], as ge_cached
//   bad  : per row of the BATCH, non-zero where an instance base did not decode (pre-zeroed)
struct sig_ws {
    uint32_t *tab, *prod, *bad;
    uint32_t row0, nstride;
};

// Launch 1, lane = (product v, row): k[sec] P for term vb_term[v].  A row past the batch has no lane (the caller bounds it).
template <bool CT>
BP_HD void sig_vb_lane(uint32_t v, uint32_t row, const sig_rel &rel, const sig_create_in &in, const ped_park &pk, const sig_ws &ws) {
    const uint32_t t = rel.vb_term[v], lane = v * ws.nstride + (row - ws.row0), nlanes = rel.nvb * ws.nstride;
    uint32_t kk[8];
    {
        sc x;
        rpp_draw(x, in.seeds + 32 * (uint64_t)row, rel.sec[t]);
#pragma unroll
        for (int q = 0; q < 8; q++) kk[q] = x.v[q];
    }
    const sig_vb_tab tab = {ws.tab + lane, nlanes};
    ge_ext q;
    const bool ok = sig_vb_mul<CT>(q, pk, tab, kk, in.points + 8 * ((uint64_t)row * rel.P + (rel.base[t] - SIG_BASE_SLOT)));
    const sig_vb_tab prod = {ws.prod + (uint64_t)40 * v * ws.nstride + (row - ws.row0), ws.nstride};
    sig_tab_store(prod, 0, q);
    if (!ok) ws.bad[row] = 1u;   // (every lane that writes here writes the same word)
}

// Launch 2, lane = (equation k, row p): T_k into words 8 k .. of the row's proof -- ped_commit_lane's shape, one encoding per lane.  The
// secrets are not looked at: a row that the finish rejects walks like any other.  CT: table and prm are the W = 4 set.
template <bool CT>
BP_HD void sig_walk_lane(uint32_t k, uint32_t p, const sig_rel &rel, const sig_create_in &in, const ped_park &pk, const sig_ws &ws, fb_params prm,
                         const fb_entry *table, uint32_t *proofs_out) {
    ge_ext acc;
    ge_identity(acc);
    bool started = false;
    // two passes over the equation's terms (the sum does not mind the order): the table walks, then the products
#pragma unroll 1
    for (uint32_t t = rel.first[k]; t < rel.first[k + 1]; t++) {
        const uint32_t b = rel.base[t];   // (the same in every lane)
        if (b >= SIG_BASE_SLOT) continue;
        uint32_t kk[8];
        {
            sc x;
            rpp_draw(x, in.seeds + 32 * (uint64_t)p, rel.sec[t]);
#pragma unroll
            for (int q = 0; q < 8; q++) kk[q] = x.v[q];
        }
        if (CT) ped_walk_ct(acc, pk, kk, prm.nwin, b, prm, table);
        else ped_walk(acc, started, pk, kk, prm.nwin, b, prm, table);
    }
#pragma unroll 1
    for (uint32_t t = rel.first[k]; t < rel.first[k + 1]; t++) {
        if (rel.base[t] < SIG_BASE_SLOT) continue;
        const sig_vb_tab prod = {ws.prod + (uint64_t)40 * rel.vb_of[t] * ws.nstride + (p - ws.row0), ws.nstride};
        sig_tab_add<false>(acc, prod, 1, false);   // (acc is the identity where no walk has started it)
    }
    uint32_t T[8];
    ped_encode(T, acc, pk);
    uint32_t *out = proofs_out + (uint64_t)p * sig_proof_words(rel) + 8 * k;
#pragma unroll
    for (int q = 0; q < 8; q++) out[q] = T[q];
}

// Launch 3, lane = row: the transcript (T_k is absorbed from the proof's own bytes), s_j = k_j + c x_j, the stores.  A rejected row: proof bytes zero, status
// BAD_SCALAR (a secret is not canonical) or BAD_POINT (an instance base does not decode), state = its input.
BP_HD void sig_finish_lane(uint32_t p, const sig_rel &rel, const sig_create_in &in, kstate st, const uint32_t *bad, uint32_t *proofs_out, uint8_t *status,
                            uint32_t *ts_out) {
    const bool pts_ok = bad[p] == 0;
    const uint32_t *xs = in.secrets + 8 * (uint64_t)p * rel.S;
    uint32_t *out = proofs_out + (uint64_t)p * sig_proof_words(rel);
    bool sc_ok = true;
    for (uint32_t j = 0; j < rel.S; j++) sc_ok = sc_is_canonical(xs + 8 * j) & sc_ok;
    const bool ok = sc_ok & pts_ok;
    strobe t;
    opn_ts_load(t, st, p, nullptr, in.ts_in, in.ts_in_stride);
    if (ts_out && !ok) rp_ts_emit(p, st, rp_ts_meta(t.pos, t.pos_begin, t.cur_flags), ts_out);
    sig_bind(t, rel, in.points + 8 * (uint64_t)p * rel.P);
    const uint8_t lT[1] = {'T'}, lc[1] = {'c'};
    // (no zero check of T_k here, where validate_and_append_point has one: T_k is the identity only when the nonces of equation k hit a
    // relation among its bases -- probability about 2^-252 for honest draws, the case tests/sigma_twin.py's create raises in -- and such a
    // proof is stopped by the verifier's front end)
    for (uint32_t k = 0; k < rel.E; k++) merlin_append_words8(t, lT, 1, out + 8 * k);
    sc c;
    rp_challenge_scalar(t, lc, 1, c);
    if (ts_out && ok) rp_ts_emit(p, st, rp_ts_meta(t.pos, t.pos_begin, t.cur_flags), ts_out);
    if (!ok)
        for (uint32_t q = 0; q < 8 * rel.E; q++) out[q] = 0u;
#pragma unroll 1
    for (uint32_t j = 0; j < rel.S; j++) {
        sc x, k;
#pragma unroll
        for (int q = 0; q < 8; q++) x.v[q] = xs[8 * j + q];
        rpp_draw(k, in.seeds + 32 * (uint64_t)p, j);
        sc_mul(x, c, x);
        sc_add(x, x, k);
#pragma unroll
        for (int q = 0; q < 8; q++) out[8 * (rel.E + j) + q] = ok ? x.v[q] : 0u;
    }
    status[p] = !sc_ok ? (uint8_t)BP_STATUS_BAD_SCALAR : (!pts_ok ? (uint8_t)BP_STATUS_BAD_POINT : (uint8_t)BP_STATUS_OK);
}

// ---- verification ------------------------------------------------------------------------------------------------------
// The front end, lane = proof.  status[p]: 0, or the verdict the row already carries -- FORMAT (an s_j is not canonical: the input
// state goes out), VERIFICATION (a T_k is 32 zero bytes: the state as of that message).  A row that goes on gets c and, per equation k
// (row r = p E + k of the chain): eq_sc / eq_pt [r U + i] and gen_sc [r (2 + G) + b] as described at the top; the outputs are pre-zeroed
// by the host and a lane adds into its own rows only.  c_out (optional, the host harness): the challenge.
BP_HD void sig_front_lane(uint32_t p, const sig_rel &rel, const rp_strobe_init &init, kstate st, const uint32_t *proofs, const uint32_t *points,
                          const uint32_t *ts_in, uint32_t ts_in_stride, uint32_t *eq_sc, uint32_t *eq_pt, uint32_t *gen_sc, uint32_t *status, uint32_t *ts_out,
                          uint32_t *c_out = nullptr) {
    const uint32_t U = sig_uniq(rel), GR = sig_gen_row(rel);
    const uint32_t *pr = proofs + (uint64_t)p * sig_proof_words(rel), *pts = points + 8 * (uint64_t)p * rel.P;
    bool fmt = false;
    for (uint32_t j = 0; j < rel.S; j++) fmt = !sc_is_canonical(pr + 8 * (rel.E + j)) || fmt;
    strobe t;
    opn_ts_load(t, st, p, &init, ts_in, ts_in_stride);
    if (fmt) {
        status[p] = BP_VERDICT_FORMAT;
        if (ts_out) rp_ts_emit(p, st, rp_ts_meta(t.pos, t.pos_begin, t.cur_flags), ts_out);
        return;
    }
    sig_bind(t, rel, pts);
    const uint8_t lT[1] = {'T'}, lc[1] = {'c'};
    for (uint32_t k = 0; k < rel.E; k++) {
        uint32_t w[8];
#pragma unroll
        for (int q = 0; q < 8; q++) w[q] = pr[8 * k + q];
        if (words8_zero(w)) {
            status[p] = BP_VERDICT_VERIFICATION;
            if (ts_out) rp_ts_emit(p, st, rp_ts_meta(t.pos, t.pos_begin, t.cur_flags), ts_out);
            return;
        }
        merlin_append_words8(t, lT, 1, pr + 8 * k);
    }
    sc c, x, s;
    rp_challenge_scalar(t, lc, 1, c);
    if (ts_out) rp_ts_emit(p, st, rp_ts_meta(t.pos, t.pos_begin, t.cur_flags), ts_out);
    if (c_out) store_words8(c_out + 8 * (uint64_t)p, c);
#pragma unroll 1
    for (uint32_t k = 0; k < rel.E; k++) {
        const uint64_t r = (uint64_t)p * rel.E + k;
#pragma unroll 1
        for (uint32_t i = rel.first[k]; i <= rel.first[k + 1]; i++) {   // the terms, then the left-hand side
            const bool is_lhs = i == rel.first[k + 1];
            const uint32_t b = is_lhs ? SIG_BASE_SLOT + rel.lhs[k] : rel.base[i];
            uint32_t *dst = b < SIG_BASE_SLOT ? gen_sc + (r * GR + b) * 8 : eq_sc + (r * U + (b - SIG_BASE_SLOT)) * 8;
#pragma unroll
            for (int q = 0; q < 8; q++) x.v[q] = dst[q];
            if (is_lhs) {
                sc_sub(x, x, c);
            } else {
#pragma unroll
                for (int q = 0; q < 8; q++) s.v[q] = pr[8 * (rel.E + rel.sec[i]) + q];
                sc_add(x, x, s);
            }
            store_words8(dst, x);
            if (b >= SIG_BASE_SLOT) {
#pragma unroll
                for (int q = 0; q < 8; q++) eq_pt[(r * U + (b - SIG_BASE_SLOT)) * 8 + q] = pts[8 * (b - SIG_BASE_SLOT) + q];
            }
        }
        sc_from_u32(s, 1);
        sc_neg(x, s);
        store_words8(eq_sc + (r * U + rel.P) * 8, x);
#pragma unroll
        for (int q = 0; q < 8; q++) eq_pt[(r * U + rel.P) * 8 + q] = pr[8 * k + q];
    }
    status[p] = 0;
}

// per-proof verdict, lane = proof: the front end's code, else OK only if each of the E rows decoded and is the identity
BP_HD void sig_verdict_thread(uint32_t p, uint32_t E, const uint32_t *status, const uint8_t *msm_status, const uint32_t *msm_out, uint8_t *verdict) {
    const uint32_t st = status[p];
    uint32_t nz = 0;
    for (uint32_t k = 0; k < E; k++) {
        nz |= msm_status[(uint64_t)p * E + k];
#pragma unroll
        for (int q = 0; q < 8; q++) nz |= msm_out[((uint64_t)p * E + k) * 8 + q];
    }
    verdict[p] = st ? (uint8_t)st : (nz ? (uint8_t)BP_VERDICT_VERIFICATION : (uint8_t)BP_VERDICT_OK);
}

// The combined check's weigh, lane tid = term * nstride + proof (rlc_weigh_thread's shape and contract) over P + E unique terms and then
// the 2 + G shared rows, with one weight per (proof, equation), rho[p E + k].  Unique term i < P: slot i with sum_k rho_k eq_sc[k][i]
// (a proof contributes P + E points, not one per term); P + k: (-rho_k, T_k); both to slot p (P + E) + term of the combined list, scalar
// 0 and the identity encoding for a proof that stopped.  A shared row b returns true with v = sum_k rho_k gen_sc[k][b] and row = b.
BP_HD bool sig_rlc_weigh_thread(uint32_t tid, uint32_t nproofs, uint32_t nstride, const sig_rel &rel, const uint32_t *status, const uint32_t *rho,
                                const uint32_t *gen_sc, const uint32_t *eq_sc, const uint32_t *eq_pt, const uint32_t *points, uint32_t *comb_sc,
                                uint32_t *comb_pt, sc &v, uint32_t &row) {
    const uint32_t t = tid / nstride, p = tid - t * nstride, NU = rel.P + rel.E, U = sig_uniq(rel), GR = sig_gen_row(rel);
    sc_0(v);
    row = t < NU ? 0u : t - NU;
    if (p >= nproofs) return false;
    const bool stopped = status[p] != 0;
    sc x, r;
    if (t < NU) {
        const uint64_t dst = ((uint64_t)p * NU + t) * 8;
        const uint32_t *src_pt = t < rel.P ? points + 8 * ((uint64_t)p * rel.P + t) : eq_pt + (((uint64_t)p * rel.E + (t - rel.P)) * U + rel.P) * 8;
        sc_0(v);
        if (!stopped) {
            for (uint32_t k = (t < rel.P ? 0u : t - rel.P); k < (t < rel.P ? rel.E : t - rel.P + 1u); k++) {
                const uint64_t rr = (uint64_t)p * rel.E + k;
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    r.v[q] = rho[8 * rr + q];
                    x.v[q] = eq_sc[(rr * U + (t < rel.P ? t : rel.P)) * 8 + q];
                }
                sc_mul(x, x, r);
                sc_add(v, v, x);
            }
        }
#pragma unroll
        for (int q = 0; q < 8; q++) comb_pt[dst + q] = stopped ? 0u : src_pt[q];
        store_words8(comb_sc + dst, v);
        sc_0(v);
        return false;
    }
    if (stopped) return false;
    for (uint32_t k = 0; k < rel.E; k++) {
        const uint64_t rr = (uint64_t)p * rel.E + k;
#pragma unroll
        for (int q = 0; q < 8; q++) {
            r.v[q] = rho[8 * rr + q];
            x.v[q] = gen_sc[(rr * GR + row) * 8 + q];
        }
        sc_mul(x, x, r);
        sc_add(v, v, x);
    }
    return true;
}

}  // namespace bp
#endif
