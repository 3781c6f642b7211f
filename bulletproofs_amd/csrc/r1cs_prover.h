// R1CS constraint-system proof CREATION on the device: r1cs::Prover::prove (src/r1cs/prover.rs:380-655 of the reference) for
// nbatch proofs of one recorded gadget (bpgpu_r1cs_circuit + bpgpu_r1cs_witness, include/bpgpu.h).
//   r1p_inputs_thread   : lane = (proof, committed / free index)   canonical inputs; the V_j = v_j B + v~_j B~ rows
//   r1p_rng_coop        : 32 lanes = proof   Prover::new, the m appends of V, "m"; then the witness-rekeyed TranscriptRng
//                                        (prover.rs:403-413) and every Scalar::random of the proof, on the cooperative
//                                        Keccak-f permutation (keccak.h); the sponge state is the group's, in LDS
//   r1p_witness_thread  : lane = proof   a_L, a_R, a_O of multipliers [i0, i1) from the witness program (free inputs, LC
//                                        rows evaluated as Prover::eval, prover.rs:340-356, or zero)
//   r1p_rows_thread     : lane = (proof, multiplier)   generator-table rows of A_I, A_O, S of one phase
//   r1p_chal1/2/3_thread: lane = proof   the transcript between the commitments: phase-2 challenges, y, z, u, x, w
//   r1p_poly_thread     : lane = (column, proof)   wL, wR, wO (r1cs.h's per-variable lists), l1..r3 (prover.rs:549-579) and
//                                        the terms of t1..t6; wV_j v~_j
//   r1p_vecs_thread     : lane = (proof, i)   l_vec, r_vec (padding: prover.rs:628-631), G_factors, H_factors of the IPP
// Per-proof scalars live field-major ([field][proof][10 words], rangeproof.h's rp_store layout); the witness and the
// vectors likewise with the multiplier index as the field.
#ifndef BPGPU_R1CS_PROVER_H
#define BPGPU_R1CS_PROVER_H
#include "r1cs.h"

namespace bp {

#define R1P_SRC_ZERO 0xffffffffu
#define R1P_SRC_FREE 0x80000000u

// one term of a witness LC row: kind (0 L, 1 R, 2 O, 3 V, 4 ONE), index, challenge (R1_NO_CHAL or j | power << 16),
// coefficient in Montgomery form (no sign flip: Prover::eval sums plainly)
struct r1p_term {
    uint32_t kind, index, chal;
    uint32_t coeff[10];
};

// fixed per-proof fields (Montgomery unless noted); the tables follow
enum {
    R1P_U_M = 0, R1P_X_M, R1P_Y_M,
    R1P_T1, R1P_T2, R1P_T3, R1P_T4, R1P_T5, R1P_T6, R1P_T2B,   // plain: <l, r> coefficients and <wV, v~>
    R1P_FIXED
};
// the per-proof point / scalar record of the proof (8 words each)
enum { R1P_AI1 = 0, R1P_AO1, R1P_S1, R1P_AI2, R1P_AO2, R1P_S2, R1P_T_1, R1P_T_3, R1P_T_4, R1P_T_5, R1P_T_6, R1P_TX, R1P_TXB, R1P_EB, R1P_NREC };

struct r1p_shape {
    r1cs_shape c;                  // m, n1, n, pn, k, two_phase, nch, Q, the z / y^-1 / challenge tables, nfields, nproofs
    uint32_t f_yplo, f_yphi;       // y^(0..63), (y^64)^(0..nyhi-1)
    uint32_t nfree, nrand;         // free inputs and random scalars per proof
    uint32_t o_sl1, o_sr1, o_b2, o_sl2, o_sr2, o_tb;   // offsets of the draws in the rng stream (prover.rs:416-418, 528-541, 583)
    uint32_t i0, i1;               // multipliers of the current phase
};
// the draw of s_L[i] / s_R[i] for multiplier i
BP_HD uint32_t r1p_sl(const r1p_shape &sh, uint32_t i) { return i < sh.c.n1 ? sh.o_sl1 + i : sh.o_sl2 + (i - sh.c.n1); }
BP_HD uint32_t r1p_sr(const r1p_shape &sh, uint32_t i) { return i < sh.c.n1 ? sh.o_sr1 + i : sh.o_sr2 + (i - sh.c.n1); }
BP_HD void r1p_ld(sc &s, const uint32_t *buf, uint32_t nproofs, uint32_t f, uint32_t p) { rp_load(s, buf, nproofs, f, p); }
BP_HD void r1p_ld_bytes(sc &s, const uint8_t *src) { load_words8(s.v, src); }

// ---- inputs: lane = (proof, j) over [0, m) then the free inputs -----------------------------------------------------------
// V rows are (B~, B, G_0) rows of the g_only generator walk: (v~_j, v_j, 0)
BP_HD void r1p_inputs_thread(uint32_t tid, const r1p_shape &sh, const uint8_t *v, const uint8_t *vb, const uint8_t *freev, uint32_t *vrows,
                             uint32_t *status) {
    const uint32_t nvm = sh.c.nproofs * sh.c.m;
    sc a, b;
    if (tid < nvm) {
        const uint32_t p = tid / sh.c.m;
        r1p_ld_bytes(a, v + (uint64_t)tid * 32);
        if (!vrows) {   // the stand-alone constraint check (r1cs_check.h): no blindings, no V rows
            if (!sc_is_canonical_sc(a)) status_raise(status + p, BP_STATUS_BAD_SCALAR);
            return;
        }
        r1p_ld_bytes(b, vb + (uint64_t)tid * 32);
        if (!sc_is_canonical_sc(a) || !sc_is_canonical_sc(b)) status_raise(status + p, BP_STATUS_BAD_SCALAR);
        uint32_t *row = vrows + (uint64_t)tid * 24;
        store_words8(row, b);
        store_words8(row + 8, a);
        return;
    }
    const uint32_t f = tid - nvm, p = f / sh.nfree;
    r1p_ld_bytes(a, freev + (uint64_t)f * 32);
    if (!sc_is_canonical_sc(a)) status_raise(status + p, BP_STATUS_BAD_SCALAR);
}

// ---- the cooperative STROBE: one 32-lane group per transcript ---------------------------------------------------------------
// Every lane of the group runs the same control flow (STROBE's positions depend on the gadget's shape only, so they are uniform
// across the wavefront); the group's leader alone writes the 50 state words in LDS, and every permutation is the cooperative one,
// bracketed by workgroup barriers (keccak_f1600_masked_coop's contract).
#if defined(__HIP_DEVICE_COMPILE__)
struct cstrobe {
    uint32_t *w;                  // the group's 50 state words (stride 1)
    uint32_t pos, pos_begin, cur_flags;
    uint32_t lane;                // lane in the wavefront
    bool lead;
};
__device__ __forceinline__ void cs_xor8(cstrobe &t, uint32_t pos, uint32_t b) {
    if (t.lead) t.w[pos >> 2] ^= b << (8 * (pos & 3));
}
__device__ void cs_run_f(cstrobe &t) {
    cs_xor8(t, t.pos, t.pos_begin);
    cs_xor8(t, t.pos + 1, 0x04);
    cs_xor8(t, BP_STROBE_R + 1, 0x80);
    __syncthreads();
    kstate st;
    st.w = t.w;
    st.stride = 1;
    keccak_f1600_masked_coop(st, nullptr, 0, t.lane);
    __syncthreads();
    t.pos = 0;
    t.pos_begin = 0;
}
__device__ void cs_absorb1(cstrobe &t, uint32_t b) {
    cs_xor8(t, t.pos++, b);
    if (t.pos == BP_STROBE_R) cs_run_f(t);
}
__device__ void cs_absorb(cstrobe &t, const uint8_t *d, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) cs_absorb1(t, d[i]);
}
__device__ void cs_absorb_words(cstrobe &t, const uint32_t *w, uint32_t n32) {
    for (uint32_t i = 0; i < n32; i++) {
        const uint32_t x = w[i];
        cs_absorb1(t, x & 0xffu);
        cs_absorb1(t, (x >> 8) & 0xffu);
        cs_absorb1(t, (x >> 16) & 0xffu);
        cs_absorb1(t, x >> 24);
    }
}
__device__ void cs_begin_op(cstrobe &t, uint32_t flags, bool more) {
    if (more) return;
    const uint32_t old_begin = t.pos_begin;
    t.pos_begin = t.pos + 1;
    t.cur_flags = flags;
    cs_absorb1(t, old_begin);
    cs_absorb1(t, flags);
    if ((flags & (BP_FLAG_C | BP_FLAG_K)) && t.pos != 0) cs_run_f(t);
}
__device__ void cs_meta_ad(cstrobe &t, const uint8_t *d, uint32_t n, bool more) {
    cs_begin_op(t, BP_FLAG_M | BP_FLAG_A, more);
    cs_absorb(t, d, n);
}
__device__ void cs_u32le(cstrobe &t, uint32_t n) {   // meta_ad(u32le(n), more = true)
    const uint8_t b[4] = {(uint8_t)n, (uint8_t)(n >> 8), (uint8_t)(n >> 16), (uint8_t)(n >> 24)};
    cs_meta_ad(t, b, 4, true);
}
// append_message(label, 32 bytes held as 8 words)
__device__ void cs_append_words8(cstrobe &t, const uint8_t *label, uint32_t label_len, const uint32_t w[8]) {
    cs_meta_ad(t, label, label_len, false);
    cs_u32le(t, 32);
    cs_begin_op(t, BP_FLAG_A, false);
    cs_absorb_words(t, w, 8);
}
__device__ void cs_append_message(cstrobe &t, const uint8_t *label, uint32_t label_len, const uint8_t *msg, uint32_t n) {
    cs_meta_ad(t, label, label_len, false);
    cs_u32le(t, n);
    cs_begin_op(t, BP_FLAG_A, false);
    cs_absorb(t, msg, n);
}
// STROBE KEY: begin_op(A | C), then the state bytes are overwritten
__device__ void cs_key_words8(cstrobe &t, const uint32_t w[8]) {
    cs_begin_op(t, BP_FLAG_A | BP_FLAG_C, false);
    for (uint32_t i = 0; i < 32; i++) {
        const uint32_t b = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
        if (t.lead) t.w[t.pos >> 2] = (t.w[t.pos >> 2] & ~(0xffu << (8 * (t.pos & 3)))) | (b << (8 * (t.pos & 3)));
        if (++t.pos == BP_STROBE_R) cs_run_f(t);
    }
}
// TranscriptRng::fill_bytes(64 bytes) + Scalar::from_bytes_mod_order_wide: meta_ad(u32le(64)), PRF(64).  The value is the leader's.
__device__ void cs_random_scalar(cstrobe &t, sc &r) {
    const uint8_t len64[4] = {64, 0, 0, 0};
    cs_meta_ad(t, len64, 4, false);
    cs_begin_op(t, BP_FLAG_I | BP_FLAG_A | BP_FLAG_C, false);
    uint32_t w[16];
    for (uint32_t i = 0; i < 16; i++) w[i] = 0;
    for (uint32_t i = 0; i < 64; i++) {
        const uint32_t wi = t.pos >> 2, shf = 8 * (t.pos & 3);
        const uint32_t b = (t.w[wi] >> shf) & 0xffu;
        w[i >> 2] |= b << (8 * (i & 3));
        if (t.lead) t.w[wi] &= ~(0xffu << shf);
        if (++t.pos == BP_STROBE_R) cs_run_f(t);
    }
    sc_from_wide(r, w);
}

// 32 lanes per proof (p >= nproofs: a group that only runs along).  ts: the proofs' transcripts before Prover::new, advanced to
// after "m" in place; vout: V_j encodings (the V launch); rnd: every random scalar of the proof, in draw order
__device__ void r1p_rng_coop(uint32_t p, uint32_t lane, uint32_t *w, const r1p_shape &sh, uint32_t *ts, const uint32_t *vout, const uint8_t *vb,
                             const uint8_t *rng32, uint32_t *rnd) {
    const bool valid = p < sh.c.nproofs;
    cstrobe t;
    t.w = w;
    t.lane = lane;
    t.lead = valid && (lane & 31) == 0;
    const uint32_t *src = ts + (uint64_t)(valid ? p : 0) * BP_TS_WORDS;
    if (t.lead)
        for (uint32_t i = 0; i < 50; i++) w[i] = src[i];
    const uint32_t meta = src[50];
    t.pos = meta & 0xffu;
    t.pos_begin = (meta >> 8) & 0xffu;
    t.cur_flags = (meta >> 16) & 0xffu;
    __syncthreads();
    const uint8_t dsep[7] = {'d', 'o', 'm', '-', 's', 'e', 'p'}, v1[7] = {'r', '1', 'c', 's', ' ', 'v', '1'}, lV[1] = {'V'}, lm[1] = {'m'};
    cs_append_message(t, dsep, 7, v1, 7);                      // Prover::new (prover.rs:277-282)
    for (uint32_t j = 0; j < sh.c.m; j++) {                    // commit (prover.rs:296-306)
        uint32_t vw[8];
        const uint32_t *vs = vout + ((uint64_t)(valid ? p : 0) * sh.c.m + j) * 8;
#pragma unroll
        for (int q = 0; q < 8; q++) vw[q] = vs[q];
        cs_append_words8(t, lV, 1, vw);
    }
    {
        uint8_t mb[8];
        for (int i = 0; i < 8; i++) mb[i] = (uint8_t)((uint64_t)sh.c.m >> (8 * i));
        cs_append_message(t, lm, 1, mb, 8);                    // prove (prover.rs:388)
    }
    __syncthreads();
    if (t.lead) {
        uint32_t *o = ts + (uint64_t)p * BP_TS_WORDS;
        for (uint32_t i = 0; i < 50; i++) o[i] = w[i];
        o[50] = rp_ts_meta(t.pos, t.pos_begin, t.cur_flags);
        o[51] = 0;
    }
    __syncthreads();
    // build_rng on the transcript as it is now (a clone: the state just stored stays the transcript's)
    const uint8_t lvb[10] = {'v', '_', 'b', 'l', 'i', 'n', 'd', 'i', 'n', 'g'}, lrng[3] = {'r', 'n', 'g'};
    for (uint32_t j = 0; j < sh.c.m; j++) {                    // rekey_with_witness_bytes(b"v_blinding", v~_j)
        uint32_t kw[8];
        load_words8(kw, vb + ((uint64_t)(valid ? p : 0) * sh.c.m + j) * 32);
        cs_meta_ad(t, lvb, 10, false);
        cs_u32le(t, 32);
        cs_key_words8(t, kw);
    }
    {                                                          // finalize(&mut thread_rng())
        uint32_t kw[8];
        load_words8(kw, rng32 + (uint64_t)(valid ? p : 0) * 32);
        cs_meta_ad(t, lrng, 3, false);
        cs_key_words8(t, kw);
    }
    for (uint32_t d = 0; d < sh.nrand; d++) {
        sc r;
        cs_random_scalar(t, r);
        if (t.lead) rp_store(rnd, sh.c.nproofs, d, p, r);
    }
}
#endif

// ---- witness: lane = proof, multipliers [i0, i1) in order ------------------------------------------------------------------
BP_HD void r1p_term_value(sc &val, const r1p_shape &sh, const r1p_term &e, const uint32_t *aw, const uint8_t *v, uint32_t p) {
    const uint32_t np = sh.c.nproofs, n = sh.c.n;
    switch (e.kind) {
    case 0: case 1: case 2: r1p_ld(val, aw, np, e.kind * n + e.index, p); break;
    case 3: r1p_ld_bytes(val, v + ((uint64_t)p * sh.c.m + e.index) * 32); break;
    default: sc_from_u32(val, 1);
    }
}
// coeff * ch_j^e * value of one term, reduced (the witness rows and the constraint check of r1cs_check.h both sum these)
BP_HD void r1p_term_product(sc &s, const r1p_shape &sh, const r1p_term &e, const uint32_t *aw, const uint8_t *v, const uint32_t *fields, uint32_t p) {
    sc val;
    sc28 c, vm, prod;
#pragma unroll
    for (int q = 0; q < 10; q++) c.v[q] = e.coeff[q];
    r1p_term_value(val, sh, e, aw, v, p);
    sc_to_mont28(vm, val);
    sc28_montmul(prod, c, vm);
    if (e.chal != R1_NO_CHAL) {   // ch_j^e (1 <= e < 256), left-to-right from the top bit
        const uint32_t j = e.chal & 0xffffu, pw = e.chal >> 16;
        sc28 ch, cp;
        r1_load28(ch, fields, sh.c, sh.c.f_ch + j, p);
        cp = ch;
        for (int bit = 30 - __builtin_clz(pw); bit >= 0; bit--) {
            sc28_montsq(cp, cp);
            if ((pw >> bit) & 1u) sc28_montmul(cp, cp, ch);
        }
        sc28_montmul(prod, prod, cp);
    }
    sc_from_mont28(s, prod);
}
// sum of coeff * ch_j^e * value over the row (Prover::eval)
BP_HD void r1p_eval_row(sc &acc, const r1p_shape &sh, const uint32_t *row_ptr, const r1p_term *terms, uint32_t r, const uint32_t *aw, const uint8_t *v,
                        const uint32_t *fields, uint32_t p) {
    sc_0(acc);
    for (uint32_t t = row_ptr[r]; t < row_ptr[r + 1]; t++) {
        sc s;
        r1p_term_product(s, sh, terms[t], aw, v, fields, p);
        sc_add(acc, acc, s);
    }
}
BP_HD void r1p_source(sc &out, const r1p_shape &sh, uint32_t src, const uint32_t *row_ptr, const r1p_term *terms, const uint32_t *aw, const uint8_t *v,
                      const uint8_t *freev, const uint32_t *fields, uint32_t p) {
    if (src == R1P_SRC_ZERO) sc_0(out);
    else if (src & R1P_SRC_FREE) r1p_ld_bytes(out, freev + ((uint64_t)p * sh.nfree + (src & ~R1P_SRC_FREE)) * 32);
    else r1p_eval_row(out, sh, row_ptr, terms, src, aw, v, fields, p);
}
// aw: a_L, a_R, a_O as fields [0, n), [n, 2n), [2n, 3n)
BP_HD void r1p_witness_thread(uint32_t p, const r1p_shape &sh, const uint32_t *src_l, const uint32_t *src_r, const uint32_t *row_ptr, const r1p_term *terms,
                              const uint8_t *v, const uint8_t *freev, const uint32_t *fields, uint32_t *aw) {
    const uint32_t np = sh.c.nproofs, n = sh.c.n;
    for (uint32_t i = sh.i0; i < sh.i1; i++) {
        sc l, r, o;
        r1p_source(l, sh, src_l[i], row_ptr, terms, aw, v, freev, fields, p);
        r1p_source(r, sh, src_r[i], row_ptr, terms, aw, v, freev, fields, p);
        sc_mul(o, l, r);
        rp_store(aw, np, i, p, l);
        rp_store(aw, np, n + i, p, r);
        rp_store(aw, np, 2 * n + i, p, o);
    }
}

// ---- generator rows of one phase: lane = (proof, i - i0); rows [proof][A_I, A_O, S][B~, B, G(pn), H(pn)] (pre-zeroed) ------
// blindings: i_blinding, o_blinding, s_blinding of the phase at draws b0, b0 + 1, b0 + 2
BP_HD void r1p_rows_thread(uint32_t tid, const r1p_shape &sh, uint32_t cnt, uint32_t b0, const uint32_t *aw, const uint32_t *rnd, uint32_t *rows) {
    const uint32_t per = cnt ? cnt : 1u, p = tid / per, ii = tid - p * per, pn = sh.c.pn, np = sh.c.nproofs, n = sh.c.n;
    const uint64_t ncol = 2 * (uint64_t)pn + 2;
    uint32_t *ai = rows + (uint64_t)(3 * p) * ncol * 8, *ao = ai + ncol * 8, *ss = ao + ncol * 8;
    sc x;
    if (ii == 0) {
        r1p_ld(x, rnd, np, b0, p);
        store_words8(ai, x);
        r1p_ld(x, rnd, np, b0 + 1, p);
        store_words8(ao, x);
        r1p_ld(x, rnd, np, b0 + 2, p);
        store_words8(ss, x);
    }
    if (ii >= cnt) return;
    const uint32_t i = sh.i0 + ii;
    r1p_ld(x, aw, np, i, p);
    store_words8(ai + (2 + i) * 8, x);
    r1p_ld(x, aw, np, n + i, p);
    store_words8(ai + (2 + pn + i) * 8, x);
    r1p_ld(x, aw, np, 2 * n + i, p);
    store_words8(ao + (2 + i) * 8, x);
    r1p_ld(x, rnd, np, r1p_sl(sh, i), p);
    store_words8(ss + (2 + i) * 8, x);
    r1p_ld(x, rnd, np, r1p_sr(sh, i), p);
    store_words8(ss + (2 + pn + i) * 8, x);
}

// ---- transcript steps, lane = proof (strobe in LDS, word-major as k_r1cs_front) --------------------------------------------
BP_HD void r1p_ts_load(strobe &t, kstate st, const uint32_t *ts, uint32_t p) {
    t.st = st;
    const uint32_t *src = ts + (uint64_t)p * BP_TS_WORDS;
    for (uint32_t i = 0; i < 50; i++) ks_set32(st, i, src[i]);
    const uint32_t meta = src[50];
    t.pos = meta & 0xffu;
    t.pos_begin = (meta >> 8) & 0xffu;
    t.cur_flags = (meta >> 16) & 0xffu;
}
BP_HD void r1p_ts_save(const strobe &t, uint32_t *ts, uint32_t p) { rp_ts_emit(p, t.st, rp_ts_meta(t.pos, t.pos_begin, t.cur_flags), ts); }
// append the three points of MSM rows [3p, 3p + 3) (or the identity) under labels A_I<ph>, A_O<ph>, S<ph>; keep them in rec
template <uint32_t ph>
BP_HD void r1p_append3(strobe &t, const uint32_t *mout, uint32_t p, uint32_t *rec) {
    const uint8_t lAI[4] = {'A', '_', 'I', (uint8_t)('0' + ph)}, lAO[4] = {'A', '_', 'O', (uint8_t)('0' + ph)}, lS[2] = {'S', (uint8_t)('0' + ph)};
    const uint8_t *lb[3] = {lAI, lAO, lS};
    const uint32_t ln[3] = {4, 4, 2};
#pragma unroll
    for (uint32_t e = 0; e < 3; e++) {
        uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (mout)
            for (int q = 0; q < 8; q++) w[q] = mout[(3 * (uint64_t)p + e) * 8 + q];
        merlin_append_words8(t, lb[e], ln[e], w);
        for (int q = 0; q < 8; q++) rec[(3 * (ph - 1) + e) * 8 + q] = w[q];
    }
}
// A_I1, A_O1, S1; create_randomized_constraints (prover.rs:384-407): the phase-2 challenges
BP_HD void r1p_chal1_thread(uint32_t p, const r1p_shape &sh, kstate st, const uint32_t *mout, const uint32_t *lbl_off, const uint8_t *lbl, uint32_t *ts,
                            uint32_t *fields, uint32_t *recs) {
    strobe t;
    r1p_ts_load(t, st, ts, p);
    r1p_append3<1>(t, mout, p, recs + (uint64_t)p * R1P_NREC * 8);
    const uint8_t dsep[7] = {'d', 'o', 'm', '-', 's', 'e', 'p'};
    if (sh.c.two_phase) {
        const uint8_t ph[11] = {'r', '1', 'c', 's', '-', '2', 'p', 'h', 'a', 's', 'e'};
        merlin_append_message(t, dsep, 7, ph, 11);
        for (uint32_t j = 0; j < sh.c.nch; j++) {
            sc c;
            sc28 cm;
            rp_challenge_scalar(t, lbl + lbl_off[j], lbl_off[j + 1] - lbl_off[j], c);
            sc_to_mont28(cm, c);
            r1_store28(fields, sh.c, sh.c.f_ch + j, p, cm);
        }
    } else {
        const uint8_t ph[11] = {'r', '1', 'c', 's', '-', '1', 'p', 'h', 'a', 's', 'e'};
        merlin_append_message(t, dsep, 7, ph, 11);
    }
    r1p_ts_save(t, ts, p);
}
// A_I2, A_O2, S2 (the identity when n2 = 0, prover.rs:480-525), y, z; the power tables of z, y^-1 and y
BP_HD void r1p_chal2_thread(uint32_t p, const r1p_shape &sh, kstate st, const uint32_t *mout, uint32_t *ts, uint32_t *fields, uint32_t *recs) {
    strobe t;
    r1p_ts_load(t, st, ts, p);
    r1p_append3<2>(t, mout, p, recs + (uint64_t)p * R1P_NREC * 8);
    sc y, z;
    const uint8_t ly[1] = {'y'}, lz[1] = {'z'};
    rp_challenge_scalar(t, ly, 1, y);
    rp_challenge_scalar(t, lz, 1, z);
    r1p_ts_save(t, ts, p);
    sc28 ym, zm, yinv;
    sc_to_mont28(ym, y);
    sc_to_mont28(zm, z);
    sc28_invert_mont_safegcd(yinv, ym);
    r1_store28(fields, sh.c, R1P_Y_M, p, ym);
    r1_build_tables(fields, sh.c, sh.c.f_zlo, sh.c.f_zhi, sh.c.nzhi, zm, p);
    r1_build_tables(fields, sh.c, sh.c.f_ylo, sh.c.f_yhi, sh.c.nyhi, yinv, p);
    r1_build_tables(fields, sh.c, sh.f_yplo, sh.f_yphi, sh.c.nyhi, ym, p);
}

// ---- polynomials: lane = (column, proof); columns [0, n) multipliers, [n, n + m) committed variables -------------------------
// vecs: l1, l2, l3, r0, r1, r3 as fields [0, n), [n, 2n), ...; terms: slot s (0..5: t1..t6, 6: wV v~) as fields s * nrow + column
BP_HD void r1p_poly_thread(uint32_t tid, const r1p_shape &sh, const uint32_t *col_ptr, const r1cs_ent *ents, const uint32_t *aw, const uint32_t *rnd,
                           const uint8_t *vb, const uint32_t *fields, uint32_t nrow, uint32_t *vecs, uint32_t *terms) {
    const uint32_t np = sh.c.nproofs, n = sh.c.n, i = tid / np, p = tid - i * np;
    if (i >= n) {
        const uint32_t j = i - n;
        sc wv, b, s;
        r1_weight(wv, sh.c, col_ptr, ents, 3 * n + j, fields, p);   // wV (its list holds -coeff: flattened_constraints' sign)
        r1p_ld_bytes(b, vb + ((uint64_t)p * sh.c.m + j) * 32);
        sc_mul(s, wv, b);
        rp_store(terms, np, 6 * nrow + j, p, s);
        return;
    }
    sc wl, wr, wo;
    r1_weight(wl, sh.c, col_ptr, ents, 3 * i, fields, p);
    r1_weight(wr, sh.c, col_ptr, ents, 3 * i + 1, fields, p);
    r1_weight(wo, sh.c, col_ptr, ents, 3 * i + 2, fields, p);
    sc28 yinv, yp, m0, m1;
    r1_pow_from_tables(yinv, fields, sh.c, sh.c.f_ylo, sh.c.f_yhi, i, p);
    r1_pow_from_tables(yp, fields, sh.c, sh.f_yplo, sh.f_yphi, i, p);
    sc aL, aR, aO, sL, sR, l1, l3, r0, r1, r3, s0, ypi;
    r1p_ld(aL, aw, np, i, p);
    r1p_ld(aR, aw, np, n + i, p);
    r1p_ld(aO, aw, np, 2 * n + i, p);
    r1p_ld(sL, rnd, np, r1p_sl(sh, i), p);
    r1p_ld(sR, rnd, np, r1p_sr(sh, i), p);
    // l1 = a_L + y^-i wR, l2 = a_O, l3 = s_L; r0 = wO - y^i, r1 = y^i a_R + wL, r3 = y^i s_R (prover.rs:549-579)
    sc_to_mont28(m0, wr);
    r1_mulp(s0, yinv, m0);
    sc_add(l1, aL, s0);
    l3 = sL;
    sc_from_mont28(ypi, yp);
    sc_sub(r0, wo, ypi);
    sc_to_mont28(m0, aR);
    r1_mulp(s0, yp, m0);
    sc_add(r1, s0, wl);
    sc_to_mont28(m1, sR);
    r1_mulp(r3, yp, m1);
    rp_store(vecs, np, i, p, l1);
    rp_store(vecs, np, n + i, p, aO);
    rp_store(vecs, np, 2 * n + i, p, l3);
    rp_store(vecs, np, 3 * n + i, p, r0);
    rp_store(vecs, np, 4 * n + i, p, r1);
    rp_store(vecs, np, 5 * n + i, p, r3);
    // VecPoly3::special_inner_product (util.rs:127-145), term i
    sc t, u;
    sc_mul(t, l1, r0);
    rp_store(terms, np, 0 * nrow + i, p, t);
    sc_mul(t, l1, r1);
    sc_mul(u, aO, r0);
    sc_add(t, t, u);
    rp_store(terms, np, 1 * nrow + i, p, t);
    sc_mul(t, aO, r1);
    sc_mul(u, l3, r0);
    sc_add(t, t, u);
    rp_store(terms, np, 2 * nrow + i, p, t);
    sc_mul(t, l1, r3);
    sc_mul(u, l3, r1);
    sc_add(t, t, u);
    rp_store(terms, np, 3 * nrow + i, p, t);
    sc_mul(t, aO, r3);
    rp_store(terms, np, 4 * nrow + i, p, t);
    sc_mul(t, l3, r3);
    rp_store(terms, np, 5 * nrow + i, p, t);
}

// the T rows (B~: t_blinding, B: t_i) of proof p from the sums; lane 0 of the proof's workgroup
BP_HD void r1p_trows_lead(uint32_t p, const r1p_shape &sh, const sc sums[7], const uint32_t *rnd, uint32_t *fields, uint32_t *trows) {
    const uint32_t np = sh.c.nproofs;
#pragma unroll
    for (uint32_t s = 0; s < 7; s++) r1_store(fields, sh.c, R1P_T1 + s, p, sums[s]);
    const uint32_t which[5] = {0, 2, 3, 4, 5};   // t1, t3, t4, t5, t6
#pragma unroll
    for (uint32_t e = 0; e < 5; e++) {
        sc b;
        r1p_ld(b, rnd, np, sh.o_tb + e, p);
        uint32_t *row = trows + (uint64_t)(5 * p + e) * 24;
        store_words8(row, b);
        store_words8(row + 8, sums[which[e]]);
    }
}

// T_1, T_3..T_6, u, x, t_x, t_x_blinding, e_blinding, w (prover.rs:587-626); innerproduct_domain_sep(padded_n)
BP_HD void r1p_horner_step(sc &acc, const sc28 &xm, const sc &c) {   // acc = c + x acc
    sc28 am;
    sc_to_mont28(am, acc);
    r1_mulp(acc, xm, am);
    sc_add(acc, acc, c);
}
// x (c0 + x (c1 + x (c2 + x (c3 + x (c4 + x c5)))))
BP_HD void r1p_horner6(sc &r, const sc28 &xm, const sc &c0, const sc &c1, const sc &c2, const sc &c3, const sc &c4, const sc &c5) {
    sc acc = c5, z;
    r1p_horner_step(acc, xm, c4);
    r1p_horner_step(acc, xm, c3);
    r1p_horner_step(acc, xm, c2);
    r1p_horner_step(acc, xm, c1);
    r1p_horner_step(acc, xm, c0);
    sc_0(z);
    r1p_horner_step(acc, xm, z);
    r = acc;
}
BP_HD void r1p_blinding(sc &b, const r1p_shape &sh, const uint32_t *rnd, const sc28 &um, uint32_t e, uint32_t p) {
    r1p_ld(b, rnd, sh.c.nproofs, e, p);
    if (sh.c.n > sh.c.n1) {
        sc b2, s0;
        sc28 bm;
        r1p_ld(b2, rnd, sh.c.nproofs, sh.o_b2 + e, p);
        sc_to_mont28(bm, b2);
        r1_mulp(s0, um, bm);
        sc_add(b, b, s0);
    }
}
BP_HD void r1p_chal3_thread(uint32_t p, const r1p_shape &sh, kstate st, const uint32_t *tout, const uint32_t *rnd, uint32_t *ts, uint32_t *fields,
                            uint32_t *recs, uint32_t *wout) {
    const uint32_t np = sh.c.nproofs;
    strobe t;
    r1p_ts_load(t, st, ts, p);
    uint32_t *rec = recs + (uint64_t)p * R1P_NREC * 8;
    const uint8_t lT[3] = {'T', '_', '1'}, digits[5] = {'1', '3', '4', '5', '6'};
#pragma unroll
    for (uint32_t e = 0; e < 5; e++) {
        uint8_t l[3] = {lT[0], lT[1], digits[e]};
        uint32_t w[8];
        for (int q = 0; q < 8; q++) w[q] = tout[(5 * (uint64_t)p + e) * 8 + q];
        merlin_append_words8(t, l, 3, w);
        for (int q = 0; q < 8; q++) rec[(R1P_T_1 + e) * 8 + q] = w[q];
    }
    sc u, x, w_;
    const uint8_t lu[1] = {'u'}, lx[1] = {'x'}, lw[1] = {'w'};
    rp_challenge_scalar(t, lu, 1, u);
    rp_challenge_scalar(t, lx, 1, x);
    sc28 xm, um;
    sc_to_mont28(xm, x);
    sc_to_mont28(um, u);
    sc t1, t2, t3, t4, t5, t6, b1, b2, b3, b4, b5, b6, tx, txb, eb, zero;
    r1_load(t1, fields, sh.c, R1P_T1, p);
    r1_load(t2, fields, sh.c, R1P_T2, p);
    r1_load(t3, fields, sh.c, R1P_T3, p);
    r1_load(t4, fields, sh.c, R1P_T4, p);
    r1_load(t5, fields, sh.c, R1P_T5, p);
    r1_load(t6, fields, sh.c, R1P_T6, p);
    r1p_ld(b1, rnd, np, sh.o_tb, p);
    r1_load(b2, fields, sh.c, R1P_T2B, p);
    r1p_ld(b3, rnd, np, sh.o_tb + 1, p);
    r1p_ld(b4, rnd, np, sh.o_tb + 2, p);
    r1p_ld(b5, rnd, np, sh.o_tb + 3, p);
    r1p_ld(b6, rnd, np, sh.o_tb + 4, p);
    r1p_horner6(tx, xm, t1, t2, t3, t4, t5, t6);
    r1p_horner6(txb, xm, b1, b2, b3, b4, b5, b6);
    sc_0(zero);
    {   // i/o/s_blinding = phase 1 + u phase 2 (zero without phase-2 multipliers); e_blinding = x (i + x (o + x s))
        sc bi, bo, bs;
        r1p_blinding(bi, sh, rnd, um, 0, p);
        r1p_blinding(bo, sh, rnd, um, 1, p);
        r1p_blinding(bs, sh, rnd, um, 2, p);
        r1p_horner6(eb, xm, bi, bo, bs, zero, zero, zero);   // x (i + x (o + x s))
    }
    const uint8_t ltx[3] = {'t', '_', 'x'}, ltxb[12] = {'t', '_', 'x', '_', 'b', 'l', 'i', 'n', 'd', 'i', 'n', 'g'},
                  leb[10] = {'e', '_', 'b', 'l', 'i', 'n', 'd', 'i', 'n', 'g'};
    merlin_append_words8(t, ltx, 3, tx.v);
    merlin_append_words8(t, ltxb, 12, txb.v);
    merlin_append_words8(t, leb, 10, eb.v);
    rp_challenge_scalar(t, lw, 1, w_);
    {   // InnerProductProof::create's innerproduct_domain_sep(n) (transcript.rs:50-53)
        const uint8_t dsep[7] = {'d', 'o', 'm', '-', 's', 'e', 'p'}, ipp[6] = {'i', 'p', 'p', ' ', 'v', '1'}, ln[1] = {'n'};
        merlin_append_message(t, dsep, 7, ipp, 6);
        merlin_append_u64(t, ln, 1, sh.c.pn);
    }
    r1p_ts_save(t, ts, p);
    store_words8(rec + R1P_TX * 8, tx);
    store_words8(rec + R1P_TXB * 8, txb);
    store_words8(rec + R1P_EB * 8, eb);
    store_words8(wout + (uint64_t)p * 8, w_);
    r1_store28(fields, sh.c, R1P_X_M, p, xm);
    r1_store28(fields, sh.c, R1P_U_M, p, um);
}

// ---- the IPP's inputs: lane = (proof, i) over padded_n, [proof][i] 32-byte records -------------------------------------------
BP_HD void r1p_vecs_thread(uint32_t tid, const r1p_shape &sh, const uint32_t *fields, const uint32_t *vecs, uint32_t *lv, uint32_t *rv, uint32_t *gf,
                           uint32_t *hf) {
    const uint32_t pn = sh.c.pn, np = sh.c.nproofs, n = sh.c.n, p = tid / pn, i = tid - p * pn;
    sc28 xm, um, yinv;
    r1_load28(xm, fields, sh.c, R1P_X_M, p);
    r1_load28(um, fields, sh.c, R1P_U_M, p);
    r1_pow_from_tables(yinv, fields, sh.c, sh.c.f_ylo, sh.c.f_yhi, i, p);
    sc l, r;
    if (i < n) {
        sc l1, l2, l3, r0, r1, r3, s0;
        sc28 am;
        r1p_ld(l1, vecs, np, i, p);
        r1p_ld(l2, vecs, np, n + i, p);
        r1p_ld(l3, vecs, np, 2 * n + i, p);
        r1p_ld(r0, vecs, np, 3 * n + i, p);
        r1p_ld(r1, vecs, np, 4 * n + i, p);
        r1p_ld(r3, vecs, np, 5 * n + i, p);
        // l = x (l1 + x (l2 + x l3)); r = r0 + x (r1 + x (x r3))   (VecPoly3::eval, util.rs:117-125)
        sc_to_mont28(am, l3);
        r1_mulp(s0, xm, am);
        sc_add(s0, s0, l2);
        sc_to_mont28(am, s0);
        r1_mulp(s0, xm, am);
        sc_add(s0, s0, l1);
        sc_to_mont28(am, s0);
        r1_mulp(l, xm, am);
        sc_to_mont28(am, r3);
        r1_mulp(s0, xm, am);
        sc_to_mont28(am, s0);
        r1_mulp(s0, xm, am);
        sc_add(s0, s0, r1);
        sc_to_mont28(am, s0);
        r1_mulp(s0, xm, am);
        sc_add(r, s0, r0);
    } else {   // padding (prover.rs:628-631): l = 0, r = -y^i
        sc28 yp;
        sc_0(l);
        r1_pow_from_tables(yp, fields, sh.c, sh.f_yplo, sh.f_yphi, i, p);
        sc_from_mont28(r, yp);
        sc_neg(r, r);
    }
    // G_factors = 1^n1 || u^(n2 + pad); H_factors = y^-i G_factors (prover.rs:640-646)
    sc g, h;
    if (i < sh.c.n1) {
        sc_from_u32(g, 1);
        sc_from_mont28(h, yinv);
    } else {
        sc28 t;
        sc_from_mont28(g, um);
        sc28_montmul(t, um, yinv);
        sc_from_mont28(h, t);
    }
    const uint64_t o = (uint64_t)tid * 8;
    store_words8(lv + o, l);
    store_words8(rv + o, r);
    store_words8(gf + o, g);
    store_words8(hf + o, h);
}

}  // namespace bp
#endif
