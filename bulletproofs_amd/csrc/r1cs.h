// R1CS constraint-system proof verification on the device: r1cs::Verifier::verify (src/r1cs/verifier.rs:329-500 of the
// reference) for a circuit recorded once as data (bpgpu_r1cs_circuit, include/bpgpu.h), up to its multiscalar multiplication.
//   r1cs_front_thread   : lane = proof   R1CSProof::from_bytes (r1cs/proof.rs:129-204), the transcript script of Verifier::new,
//                                        commit and verify (verifier.rs:189-194, 235-243, 337-404), the IPP challenges, the
//                                        TranscriptRng draw of r (verifier.rs:448-449); the per-proof scalar tables below
//   r1cs_flatten_thread : lane = (column, proof)   flattened_constraints (verifier.rs:260-298) over the circuit's per-variable
//                                        (CSC) lists, the g / h scalars of multiplier i (verifier.rs:406-444), wV_j * r x^2
//   r1cs_finish_block   : 64 lanes = proof   delta = <y^-n o wR, wL> and the B / B_blinding coefficients (verifier.rs:416, 476-481)
// The mega-check itself is bpgpu_msm_batch_shared's chain: generator rows (B_blinding, B, G(padded_n), H(padded_n)) and
// 11 + m + 2k per-proof points (A_I1, A_O1, S1, A_I2, A_O2, S2, V_0.., T_1, T_3..T_6, L_0.., R_0..).
// Per-proof scalars live field-major ([field][proof][10 words], rangeproof.h's rp_store layout).
#ifndef BPGPU_R1CS_H
#define BPGPU_R1CS_H
#include "rangeproof.h"
#include <cstring>
#include <vector>

namespace bp {

// one term of a per-variable list: constraint q, coefficient (Montgomery form, the reference's sign for V / ONE folded in),
// challenge j with power e (chal = j | e << 16; R1_NO_CHAL: none)
#define R1_NO_CHAL 0xffffffffu
struct r1cs_ent {
    uint32_t q, chal;
    uint32_t coeff[10];
};

// scalar fields of the per-proof store; after the fixed ones: z^(0..63), (z^64)^(0..nzhi-1), y^-(0..63), (y^-64)^(0..nyhi-1),
// the phase-2 challenges, and per IPP round (u_i, u_i^-1) -- all Montgomery
enum {
    R1F_X = 0, R1F_XX, R1F_RXX, R1F_W, R1F_R, R1F_TX, R1F_TXB, R1F_EB, R1F_A, R1F_B,   // plain
    R1F_X_M, R1F_A_M, R1F_B_M, R1F_U_M,                                                  // Montgomery
    R1F_FIXED
};

struct r1cs_shape {
    uint32_t m, n1, n, pn, k;      // committed variables, phase-1 multipliers, all multipliers, padded_n, lg(padded_n)
    uint32_t two_phase, nch, Q;    // r1cs-2phase?, phase-2 challenges, constraints
    uint32_t nzhi, nyhi;           // lengths of the high power tables
    uint32_t f_zlo, f_zhi, f_ylo, f_yhi, f_ch, f_tab, nfields;
    uint32_t U;                    // per-proof points: 11 + m + 2k
    uint32_t proof_stride, nproofs;
    uint32_t one_chunks;           // lanes per proof over the ONE list (R1_ONE_CHUNK entries each, at least one)
    uint32_t gens_short;           // padded_n > gens_capacity: InvalidGeneratorsLength after the phase-2 challenges
    uint32_t seeded;               // rng32 not given: proof p's 32 bytes are ChaCha20(seed, block p, domain R1_RNG_DOMAIN)
    uint32_t seed[8];
};
#define R1_RNG_DOMAIN 0x72316373u   // "s1cr"
#define R1_ONE_CHUNK 32
#define R1_VERDICT_GENS 4            // BPGPU_VERDICT_INVALID_GENERATORS_LENGTH

BP_HD void r1_load_words8_u(uint32_t w[8], const uint8_t *src) {   // byte-aligned (proof elements sit behind the version byte)
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = (uint32_t)src[4 * i] | ((uint32_t)src[4 * i + 1] << 8) | ((uint32_t)src[4 * i + 2] << 16) | ((uint32_t)src[4 * i + 3] << 24);
}
BP_HD void r1_store(uint32_t *buf, const r1cs_shape &sh, uint32_t f, uint32_t p, const sc &s) { rp_store(buf, sh.nproofs, f, p, s); }
BP_HD void r1_store28(uint32_t *buf, const r1cs_shape &sh, uint32_t f, uint32_t p, const sc28 &s) { rp_store28(buf, sh.nproofs, f, p, s); }
BP_HD void r1_load(sc &s, const uint32_t *buf, const r1cs_shape &sh, uint32_t f, uint32_t p) { rp_load(s, buf, sh.nproofs, f, p); }
BP_HD void r1_load28(sc28 &s, const uint32_t *buf, const r1cs_shape &sh, uint32_t f, uint32_t p) { rp_load28(s, buf, sh.nproofs, f, p); }
BP_HD void r1_mulp(sc &r, const sc28 &am, const sc28 &bm) {   // plain a*b from two Montgomery forms
    sc28 t;
    sc28_montmul(t, am, bm);
    sc_from_mont28(r, t);
}

// STROBE-128 KEY (merlin's strobe.rs: begin_op(A | C), then the state bytes are overwritten)
BP_HD void strobe_key(strobe &t, const uint8_t *d, uint32_t n) {
    strobe_begin_op(t, BP_FLAG_A | BP_FLAG_C, false);
    for (uint32_t i = 0; i < n; i++) {
        ks_clear8(t.st, t.pos);
        ks_xor8(t.st, t.pos, d[i]);
        if (++t.pos == BP_STROBE_R) strobe_run_f(t);
    }
}
// transcript.build_rng().finalize(rng32) -> Scalar::random (merlin 2 TranscriptRngBuilder::finalize / TranscriptRng::fill_bytes):
// meta-AD "rng", KEY the 32 bytes, meta-AD u32le(64), PRF 64 bytes, wide reduction.  Consumes `t` (a clone in the reference).
BP_HD void r1_transcript_rng_scalar(strobe &t, const uint8_t key[32], sc &r) {
    const uint8_t lrng[3] = {'r', 'n', 'g'}, len64[4] = {64, 0, 0, 0};
    strobe_meta_ad(t, lrng, 3, false);
    strobe_key(t, key, 32);
    strobe_meta_ad(t, len64, 4, false);
    strobe_begin_op(t, BP_FLAG_I | BP_FLAG_A | BP_FLAG_C, false);
    uint32_t w[16];
    for (int i = 0; i < 16; i++) w[i] = strobe_squeeze_word(t);
    sc_from_wide(r, w);
}

BP_HD void r1_emit(uint32_t p, const strobe &t, uint32_t *ts_out) {
    if (ts_out) rp_ts_emit(p, t.st, rp_ts_meta(t.pos, t.pos_begin, t.cur_flags), ts_out);
}
// table[e] for e = lo + 64 hi: t[f_lo + (e & 63)] * t[f_hi + (e >> 6)]
BP_HD void r1_pow_from_tables(sc28 &r, const uint32_t *fields, const r1cs_shape &sh, uint32_t f_lo, uint32_t f_hi, uint32_t e, uint32_t p) {
    sc28 lo, hi;
    r1_load28(lo, fields, sh, f_lo + (e & 63u), p);
    r1_load28(hi, fields, sh, f_hi + (e >> 6), p);
    sc28_montmul(r, lo, hi);
}
BP_HD void r1_build_tables(uint32_t *fields, const r1cs_shape &sh, uint32_t f_lo, uint32_t f_hi, uint32_t nhi, const sc28 &base, uint32_t p) {
    sc28 acc;
    sc28_one_mont(acc);
    for (uint32_t e = 0; e < 64; e++) {
        r1_store28(fields, sh, f_lo + e, p, acc);
        sc28_montmul(acc, acc, base);
    }
    sc28 hi;                         // acc = base^64
    sc28_one_mont(hi);
    for (uint32_t j = 0; j < nhi; j++) {
        r1_store28(fields, sh, f_hi + j, p, hi);
        sc28_montmul(hi, hi, acc);
    }
}

// ---- launch 1: lane = proof ----------------------------------------------------------------------------------------------
// Outputs are pre-zeroed by the host.  status[p]: 0, or the BPGPU_VERDICT_* the reference returns before its MSM.
BP_HD void r1cs_front_thread(uint32_t p, const r1cs_shape &sh, const rp_strobe_init &init, kstate st, const uint8_t *proofs,
                             const uint32_t *proof_lens, const uint8_t *commitments, const uint32_t *ts_in, const uint8_t *rng32,
                             const uint32_t *lbl_off, const uint8_t *lbl, uint32_t *fields, uint32_t *uniq_sc, uint32_t *uniq_pt,
                             uint32_t *ts_out, uint32_t *status) {
    const uint8_t *pr = proofs + (uint64_t)p * sh.proof_stride;
    const uint32_t len = proof_lens[p];
    // R1CSProof::from_bytes (proof.rs:129-204), InnerProductProof::from_bytes (inner_product_proof.rs:373-407)
    bool fmt = len < 1 || len > sh.proof_stride;
    uint32_t ver = 0, k = 0, e0 = 0;
    if (!fmt) {
        ver = pr[0];
        const uint32_t rest = len - 1;
        const uint32_t nel = ver == 0 ? 11u : 14u;
        fmt = rest % 32 != 0 || ver > 1 || rest < nel * 32;
        if (!fmt) {
            const uint32_t ne = rest / 32 - nel;
            fmt = ne < 2 || (ne - 2) % 2 != 0 || (ne - 2) / 2 >= 32;
            k = fmt ? 0 : (ne - 2) / 2;
            e0 = nel;
        }
    }
    const uint32_t o_T = ver ? 6u : 3u;      // element index of T_1
    sc tx, txb, eb, a, b;
    if (!fmt) {
        r1_load_words8_u(tx.v, pr + 1 + 32 * (o_T + 5));
        r1_load_words8_u(txb.v, pr + 1 + 32 * (o_T + 6));
        r1_load_words8_u(eb.v, pr + 1 + 32 * (o_T + 7));
        r1_load_words8_u(a.v, pr + 1 + 32 * (e0 + 2 * k));
        r1_load_words8_u(b.v, pr + 1 + 32 * (e0 + 2 * k + 1));
        fmt = !sc_is_canonical_sc(tx) || !sc_is_canonical_sc(txb) || !sc_is_canonical_sc(eb) || !sc_is_canonical_sc(a) || !sc_is_canonical_sc(b);
    }
    if (fmt) {
        status[p] = BP_VERDICT_FORMAT;
        rp_ts_passthrough(p, init, ts_in, ts_out);
        return;
    }
    strobe t;
    t.st = st;
    if (ts_in) {
        const uint32_t *src = ts_in + (uint64_t)p * BP_TS_WORDS;
        for (uint32_t i = 0; i < 50; i++) ks_set32(st, i, src[i]);
        const uint32_t meta = src[50];
        t.pos = meta & 0xffu;
        t.pos_begin = (meta >> 8) & 0xffu;
        t.cur_flags = (meta >> 16) & 0xffu;
    } else {
        for (uint32_t i = 0; i < 50; i++) ks_set32(st, i, init.w[i]);
        t.pos = init.pos;
        t.pos_begin = init.pos_begin;
        t.cur_flags = init.cur_flags;
    }
    uint32_t *usc = uniq_sc + (uint64_t)p * sh.U * 8, *upt = uniq_pt + (uint64_t)p * sh.U * 8;
    const uint8_t dsep[7] = {'d', 'o', 'm', '-', 's', 'e', 'p'};
    // Verifier::new + commit (verifier.rs:189-194, 235-243)
    {
        const uint8_t v1[7] = {'r', '1', 'c', 's', ' ', 'v', '1'}, lV[1] = {'V'};
        merlin_append_message(t, dsep, 7, v1, 7);
        const uint8_t *cm = commitments + (uint64_t)p * sh.m * 32;
        for (uint32_t j = 0; j < sh.m; j++) {
            uint32_t w[8];
            r1_load_words8_u(w, cm + 32 * j);
            merlin_append_words8(t, lV, 1, w);
            for (int q = 0; q < 8; q++) upt[(6 + j) * 8 + q] = w[q];
        }
        const uint8_t lm[1] = {'m'};
        merlin_append_u64(t, lm, 1, sh.m);
    }
    // A_I1, A_O1, S1 (validated), A_I2, A_O2, S2 (not), T_1, T_3..T_6 (validated): the per-proof points
    const uint8_t lAI1[4] = {'A', '_', 'I', '1'}, lAO1[4] = {'A', '_', 'O', '1'}, lS1[2] = {'S', '1'};
    const uint8_t *l1[3] = {lAI1, lAO1, lS1};
    const uint32_t l1n[3] = {4, 4, 2};
    for (uint32_t e = 0; e < 3; e++) {
        uint32_t w[8];
        r1_load_words8_u(w, pr + 1 + 32 * e);
        if (words8_zero(w)) {   // validate_and_append_point (transcript.rs:75-87): Err before absorbing
            r1_emit(p, t, ts_out);
            status[p] = BP_VERDICT_VERIFICATION;
            return;
        }
        merlin_append_words8(t, l1[e], l1n[e], w);
        for (int q = 0; q < 8; q++) upt[e * 8 + q] = w[q];
    }
    // create_randomized_constraints (verifier.rs:300-321)
    sc28 ch_m;
    if (sh.two_phase) {
        const uint8_t ph[11] = {'r', '1', 'c', 's', '-', '2', 'p', 'h', 'a', 's', 'e'};
        merlin_append_message(t, dsep, 7, ph, 11);
        for (uint32_t j = 0; j < sh.nch; j++) {
            sc c;
            rp_challenge_scalar(t, lbl + lbl_off[j], lbl_off[j + 1] - lbl_off[j], c);
            sc_to_mont28(ch_m, c);
            r1_store28(fields, sh, sh.f_ch + j, p, ch_m);
        }
    } else {
        const uint8_t ph[11] = {'r', '1', 'c', 's', '-', '1', 'p', 'h', 'a', 's', 'e'};
        merlin_append_message(t, dsep, 7, ph, 11);
    }
    if (sh.gens_short) {   // verifier.rs:341-343
        r1_emit(p, t, ts_out);
        status[p] = R1_VERDICT_GENS;
        return;
    }
    {
        const uint8_t lAI2[4] = {'A', '_', 'I', '2'}, lAO2[4] = {'A', '_', 'O', '2'}, lS2[2] = {'S', '2'};
        const uint8_t *l2[3] = {lAI2, lAO2, lS2};
        for (uint32_t e = 0; e < 3; e++) {
            uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // one-phase serialization: the identity
            if (ver) r1_load_words8_u(w, pr + 1 + 32 * (3 + e));
            merlin_append_words8(t, l2[e], l1n[e], w);
            for (int q = 0; q < 8; q++) upt[(3 + e) * 8 + q] = w[q];
        }
    }
    sc y, z, u, x, w_;
    {
        const uint8_t ly[1] = {'y'}, lz[1] = {'z'};
        rp_challenge_scalar(t, ly, 1, y);
        rp_challenge_scalar(t, lz, 1, z);
    }
    {
        const uint8_t lT1[3] = {'T', '_', '1'}, lT3[3] = {'T', '_', '3'}, lT4[3] = {'T', '_', '4'}, lT5[3] = {'T', '_', '5'}, lT6[3] = {'T', '_', '6'};
        const uint8_t *lT[5] = {lT1, lT3, lT4, lT5, lT6};
        for (uint32_t e = 0; e < 5; e++) {
            uint32_t w[8];
            r1_load_words8_u(w, pr + 1 + 32 * (o_T + e));
            if (words8_zero(w)) {
                r1_emit(p, t, ts_out);
                status[p] = BP_VERDICT_VERIFICATION;
                return;
            }
            merlin_append_words8(t, lT[e], 3, w);
            for (int q = 0; q < 8; q++) upt[(6 + sh.m + e) * 8 + q] = w[q];
        }
    }
    {
        const uint8_t lu[1] = {'u'}, lx[1] = {'x'}, lw[1] = {'w'};
        const uint8_t ltx[3] = {'t', '_', 'x'}, ltxb[12] = {'t', '_', 'x', '_', 'b', 'l', 'i', 'n', 'd', 'i', 'n', 'g'},
                      leb[10] = {'e', '_', 'b', 'l', 'i', 'n', 'd', 'i', 'n', 'g'};
        rp_challenge_scalar(t, lu, 1, u);
        rp_challenge_scalar(t, lx, 1, x);
        merlin_append_words8(t, ltx, 3, tx.v);
        merlin_append_words8(t, ltxb, 12, txb.v);
        merlin_append_words8(t, leb, 10, eb.v);
        rp_challenge_scalar(t, lw, 1, w_);
    }
    // verification_scalars(padded_n) (inner_product_proof.rs:198-253): n != 2^lg_n returns before its domain separator
    if (k != sh.k) {
        r1_emit(p, t, ts_out);
        status[p] = BP_VERDICT_VERIFICATION;
        return;
    }
    {
        const uint8_t ipp[6] = {'i', 'p', 'p', ' ', 'v', '1'}, ln[1] = {'n'};
        merlin_append_message(t, dsep, 7, ipp, 6);
        merlin_append_u64(t, ln, 1, sh.pn);
    }
    const uint8_t lL[1] = {'L'}, lR[1] = {'R'}, lu[1] = {'u'};
    sc28 acc, um, ym;
    sc28_one_mont(acc);
    for (uint32_t i = 0; i < k; i++) {
        uint32_t wl[8], wr[8];
        r1_load_words8_u(wl, pr + 1 + 32 * (e0 + 2 * i));
        r1_load_words8_u(wr, pr + 1 + 32 * (e0 + 2 * i + 1));
        if (words8_zero(wl)) {
            r1_emit(p, t, ts_out);
            status[p] = BP_VERDICT_VERIFICATION;
            return;
        }
        merlin_append_words8(t, lL, 1, wl);
        if (words8_zero(wr)) {
            r1_emit(p, t, ts_out);
            status[p] = BP_VERDICT_VERIFICATION;
            return;
        }
        merlin_append_words8(t, lR, 1, wr);
        for (int q = 0; q < 8; q++) {
            upt[(11 + sh.m + i) * 8 + q] = wl[q];
            upt[(11 + sh.m + k + i) * 8 + q] = wr[q];
        }
        sc ui;
        rp_challenge_scalar(t, lu, 1, ui);
        sc_to_mont28(um, ui);
        r1_store28(fields, sh, sh.f_tab + 2 * i, p, um);
        r1_store28(fields, sh, sh.f_tab + 2 * i + 1, p, acc);   // prefix product before u_i
        sc28_montmul(acc, acc, um);
    }
    r1_emit(p, t, ts_out);   // the reference's transcript after the last IPP challenge (build_rng works on a clone)
    // one inversion for y and every u_i
    sc28 tot, inv, yinv_m;
    sc_to_mont28(ym, y);
    sc28_montmul(tot, acc, ym);
    sc28_invert_mont_safegcd(inv, tot);
    sc28_montmul(yinv_m, inv, acc);      // 1 / y
    sc28_montmul(inv, inv, ym);          // 1 / prod u_i
    for (uint32_t ii = k; ii-- > 0;) {
        sc28 pre, ui_inv, sq;
        sc s0;
        r1_load28(um, fields, sh, sh.f_tab + 2 * ii, p);
        r1_load28(pre, fields, sh, sh.f_tab + 2 * ii + 1, p);
        sc28_montmul(ui_inv, inv, pre);
        sc28_montmul(inv, inv, um);
        r1_store28(fields, sh, sh.f_tab + 2 * ii + 1, p, ui_inv);
        sc28_montsq(sq, um);
        sc_from_mont28(s0, sq);
        store_words8(usc + (11 + sh.m + ii) * 8, s0);   // u_i^2 on L_i
        sc28_montsq(sq, ui_inv);
        sc_from_mont28(s0, sq);
        store_words8(usc + (11 + sh.m + k + ii) * 8, s0);   // u_i^-2 on R_i
    }
    // r = Scalar::random(transcript.build_rng().finalize(thread_rng()))  (verifier.rs:446-449)
    sc r;
    {
        uint8_t key[32];
        if (rng32) {
            for (int i = 0; i < 32; i++) key[i] = rng32[(uint64_t)p * 32 + i];
        } else {
            uint32_t kw[16];
            chacha20_block(sh.seed, (uint64_t)p, R1_RNG_DOMAIN, 0u, kw);
            for (int i = 0; i < 32; i++) key[i] = (uint8_t)(kw[i >> 2] >> (8 * (i & 3)));
        }
        r1_transcript_rng_scalar(t, key, r);
    }
    // the per-proof scalars: tables of z^e and y^-e, the coefficients of the points (verifier.rs:451-491)
    sc28 zm, xm, um_, am, bm;
    sc_to_mont28(zm, z);
    sc_to_mont28(xm, x);
    sc_to_mont28(um_, u);
    sc_to_mont28(am, a);
    sc_to_mont28(bm, b);
    r1_build_tables(fields, sh, sh.f_zlo, sh.f_zhi, sh.nzhi, zm, p);
    r1_build_tables(fields, sh, sh.f_ylo, sh.f_yhi, sh.nyhi, yinv_m, p);
    sc xx, xxx, rxx, s0;
    sc28 xxm, rm, rxxm, t28;
    sc28_montsq(xxm, xm);
    sc_from_mont28(xx, xxm);
    sc28_montmul(t28, xxm, xm);
    sc_from_mont28(xxx, t28);
    sc_to_mont28(rm, r);
    sc28_montmul(rxxm, rm, xxm);
    sc_from_mont28(rxx, rxxm);
    store_words8(usc + 0 * 8, x);            // A_I1
    store_words8(usc + 1 * 8, xx);           // A_O1
    store_words8(usc + 2 * 8, xxx);          // S1
    r1_mulp(s0, um_, xm);
    store_words8(usc + 3 * 8, s0);           // A_I2
    r1_mulp(s0, um_, xxm);
    store_words8(usc + 4 * 8, s0);           // A_O2
    r1_mulp(s0, um_, t28);
    store_words8(usc + 5 * 8, s0);           // S2
    {
        const uint32_t tb = 6 + sh.m;        // T_scalars = [r x, r x^3, r x^4, r x^5, r x^6]
        sc28 q;
        r1_mulp(s0, rm, xm);
        store_words8(usc + tb * 8, s0);
        sc28_montmul(q, rxxm, xm);
        sc_from_mont28(s0, q);
        store_words8(usc + (tb + 1) * 8, s0);
        sc28_montmul(q, q, xm);
        sc_from_mont28(s0, q);
        store_words8(usc + (tb + 2) * 8, s0);
        sc28_montmul(q, q, xm);
        sc_from_mont28(s0, q);
        store_words8(usc + (tb + 3) * 8, s0);
        sc28_montmul(q, q, xm);
        sc_from_mont28(s0, q);
        store_words8(usc + (tb + 4) * 8, s0);
    }
    r1_store(fields, sh, R1F_X, p, x);
    r1_store(fields, sh, R1F_XX, p, xx);
    r1_store(fields, sh, R1F_RXX, p, rxx);
    r1_store(fields, sh, R1F_W, p, w_);
    r1_store(fields, sh, R1F_R, p, r);
    r1_store(fields, sh, R1F_TX, p, tx);
    r1_store(fields, sh, R1F_TXB, p, txb);
    r1_store(fields, sh, R1F_EB, p, eb);
    r1_store(fields, sh, R1F_A, p, a);
    r1_store(fields, sh, R1F_B, p, b);
    r1_store28(fields, sh, R1F_X_M, p, xm);
    r1_store28(fields, sh, R1F_A_M, p, am);
    r1_store28(fields, sh, R1F_B_M, p, bm);
    r1_store28(fields, sh, R1F_U_M, p, um_);
}

// ---- launch 2: lane = (column, proof), column-major so that a wavefront walks one list ------------------------------------
// weight of list entries [t0, t1): sum of coeff * ch_j^e * z^(q+1)
BP_HD void r1_weight_range(sc &acc, const r1cs_shape &sh, const r1cs_ent *ents, uint32_t t0, uint32_t t1, const uint32_t *fields, uint32_t p) {
    sc_0(acc);
    for (uint32_t t = t0; t < t1; t++) {
        const r1cs_ent &e = ents[t];
        sc28 c, zp, prod;
#pragma unroll
        for (int q = 0; q < 10; q++) c.v[q] = e.coeff[q];
        r1_pow_from_tables(zp, fields, sh, sh.f_zlo, sh.f_zhi, e.q + 1, p);
        sc28_montmul(prod, c, zp);
        if (e.chal != R1_NO_CHAL) {   // ch_j^e (1 <= e < 256), left-to-right from the top bit
            const uint32_t j = e.chal & 0xffffu, pw = e.chal >> 16;
            sc28 ch, cp;
            r1_load28(ch, fields, sh, sh.f_ch + j, p);
            cp = ch;
            for (int bit = 30 - __builtin_clz(pw); bit >= 0; bit--) {
                sc28_montsq(cp, cp);
                if ((pw >> bit) & 1u) sc28_montmul(cp, cp, ch);
            }
            sc28_montmul(prod, prod, cp);
        }
        sc s;
        sc_from_mont28(s, prod);
        sc_add(acc, acc, s);
    }
}
BP_HD void r1_weight(sc &acc, const r1cs_shape &sh, const uint32_t *col_ptr, const r1cs_ent *ents, uint32_t col, const uint32_t *fields, uint32_t p) {
    r1_weight_range(acc, sh, ents, col_ptr[col], col_ptr[col + 1], fields, p);
}

// columns [0, pn): multiplier i (wL, wR, wO lists 3i, 3i+1, 3i+2; none for the padding) -> g_i, h_i and the delta term;
// [pn, pn + m): V_j -> wV_j r x^2; [pn + m, pn + m + one_chunks): R1_ONE_CHUNK entries of the ONE list each (a gadget puts
// constants in most constraints: the shuffle's x_i - z) -> partial sums of wc in rows pn.. of dterm
BP_HD void r1cs_flatten_thread(uint32_t tid, const r1cs_shape &sh, const uint32_t *col_ptr, const r1cs_ent *ents, const uint32_t *status,
                               uint32_t *fields, uint32_t *gen_sc, uint32_t *uniq_sc, uint32_t *dterm) {
    const uint32_t i = tid / sh.nproofs, p = tid - i * sh.nproofs;
    if (status[p] != 0) return;
    const uint32_t pn = sh.pn, n = sh.n;
    if (i >= pn) {
        const uint32_t j = i - pn;
        sc wv;
        if (j >= sh.m) {
            const uint32_t c = j - sh.m, b0 = col_ptr[3 * n + sh.m], b1 = col_ptr[3 * n + sh.m + 1];
            const uint32_t t0 = b0 + c * R1_ONE_CHUNK, t1 = t0 + R1_ONE_CHUNK < b1 ? t0 + R1_ONE_CHUNK : b1;
            r1_weight_range(wv, sh, ents, t0 < b1 ? t0 : b1, t1, fields, p);
            store_words8(dterm + ((uint64_t)(pn + c) * sh.nproofs + p) * 8, wv);
            return;
        }
        r1_weight(wv, sh, col_ptr, ents, 3 * n + j, fields, p);
        sc rxx, s0;
        r1_load(rxx, fields, sh, R1F_RXX, p);
        sc_mul(s0, wv, rxx);
        store_words8(uniq_sc + ((uint64_t)p * sh.U + 6 + j) * 8, s0);
        return;
    }
    sc wl, wr, wo;
    if (i < n) {
        r1_weight(wl, sh, col_ptr, ents, 3 * i, fields, p);
        r1_weight(wr, sh, col_ptr, ents, 3 * i + 1, fields, p);
        r1_weight(wo, sh, col_ptr, ents, 3 * i + 2, fields, p);
    } else {
        sc_0(wl);
        sc_0(wr);
        sc_0(wo);
    }
    sc28 yinv, s, sinv;
    r1_pow_from_tables(yinv, fields, sh, sh.f_ylo, sh.f_yhi, i, p);
    // s_i = prod_b (bit_b(i) ? u : u^-1)[k-1-b]; s_i^-1 = s_{pn-1-i} has the factors swapped (inner_product_proof.rs:241-250)
    sc28_one_mont(s);
    sc28_one_mont(sinv);
    for (uint32_t bb = 0; bb < sh.k; bb++) {
        const uint32_t j = sh.k - 1 - bb, set = (i >> bb) & 1u;
        sc28 f, g;
        r1_load28(f, fields, sh, sh.f_tab + 2 * j + (set ? 0 : 1), p);
        r1_load28(g, fields, sh, sh.f_tab + 2 * j + (set ? 1 : 0), p);
        sc28_montmul(s, s, f);
        sc28_montmul(sinv, sinv, g);
    }
    sc28 xm, am, bm, um, t0, t1;
    r1_load28(xm, fields, sh, R1F_X_M, p);
    r1_load28(am, fields, sh, R1F_A_M, p);
    r1_load28(bm, fields, sh, R1F_B_M, p);
    sc ynwr, v, w2, g, h, one;
    sc28 wrm, wlm;
    sc_to_mont28(wrm, wr);
    sc28_montmul(t0, wrm, yinv);
    sc_from_mont28(ynwr, t0);                 // yneg_wR_i
    sc_to_mont28(wlm, wl);
    sc28_montmul(t1, t0, wlm);
    sc_from_mont28(v, t1);
    store_words8(dterm + ((uint64_t)i * sh.nproofs + p) * 8, v);   // yneg_wR_i * wL_i (delta)
    // g_i = u_or_1 (x yneg_wR_i - a s_i)
    r1_mulp(v, xm, t0);
    r1_mulp(w2, am, s);
    sc_sub(g, v, w2);
    // h_i = u_or_1 (y^-i (x wL_i + wO_i - b s_i^-1) - 1)
    r1_mulp(v, xm, wlm);
    sc_add(v, v, wo);
    r1_mulp(w2, bm, sinv);
    sc_sub(v, v, w2);
    sc28 vm;
    sc_to_mont28(vm, v);
    r1_mulp(h, yinv, vm);
    sc_from_u32(one, 1);
    sc_sub(h, h, one);
    if (i >= sh.n1) {
        sc28 um, gm, hm;
        r1_load28(um, fields, sh, R1F_U_M, p);
        sc_to_mont28(gm, g);
        sc_to_mont28(hm, h);
        r1_mulp(g, um, gm);
        r1_mulp(h, um, hm);
    }
    uint32_t *row = gen_sc + (uint64_t)p * (2 * pn + 2) * 8;
    store_words8(row + (2 + i) * 8, g);
    store_words8(row + (2 + pn + i) * 8, h);
}

// ---- launch 3: 64 lanes per proof: delta and wc (sums over dterm rows), then B = w (t_x - a b) + r (x^2 (wc + delta) - t_x), B_blinding = -e_blinding - r t_x_blinding
BP_HD void r1_finish_lead(uint32_t p, const r1cs_shape &sh, const sc &delta, const sc &wc, const uint32_t *fields, uint32_t *gen_sc) {
    sc w, tx, txb, eb, a, b, r, xx, t0, t1, t2;
    r1_load(w, fields, sh, R1F_W, p);
    r1_load(tx, fields, sh, R1F_TX, p);
    r1_load(txb, fields, sh, R1F_TXB, p);
    r1_load(eb, fields, sh, R1F_EB, p);
    r1_load(a, fields, sh, R1F_A, p);
    r1_load(b, fields, sh, R1F_B, p);
    r1_load(r, fields, sh, R1F_R, p);
    r1_load(xx, fields, sh, R1F_XX, p);
    sc_mul(t0, a, b);
    sc_sub(t0, tx, t0);
    sc_mul(t0, w, t0);                        // w (t_x - a b)
    sc_add(t1, wc, delta);
    sc_mul(t1, xx, t1);
    sc_sub(t1, t1, tx);
    sc_mul(t1, r, t1);                        // r (x^2 (wc + delta) - t_x)
    sc_add(t0, t0, t1);
    sc_mul(t2, r, txb);
    sc_add(t2, t2, eb);
    sc_neg(t2, t2);
    uint32_t *row = gen_sc + (uint64_t)p * (2 * sh.pn + 2) * 8;
    store_words8(row, t2);                    // B_blinding
    store_words8(row + 8, t0);                // B
}

// ---- host side: the circuit as the launches read it (bpgpu_r1cs_circuit_create and the launch set-up of libbpgpu.so; the host harness of
// tests/r1cs_harness runs the same two functions, so that it drives the product's data layout and not a copy of it) -------------------
// (plain host functions: a HIP translation unit parses them in its device pass too, and emits nothing for them there)
// the per-variable lists of VALIDATED term arrays (bpgpu_r1cs_circuit_create's arguments; kinds L, R, O, V, ONE = 0..4): col_ptr has
// 3n + m + 2 entries over the columns L_i, R_i, O_i (3i, 3i+1, 3i+2), V_j (3n + j), ONE (3n + m)
inline void r1cs_build_lists(size_t m, size_t n, size_t n_constraints, const uint32_t *row_ptr, size_t n_terms, const uint8_t *term_kind,
                             const uint32_t *term_index, const uint32_t *term_challenge, const uint32_t *term_power, const uint8_t *term_coeff,
                             std::vector<uint32_t> &col_ptr, std::vector<r1cs_ent> &ents) {
    const size_t ncols = 3 * n + m + 1;
    std::vector<uint32_t> cnt(ncols + 1, 0), col(n_terms);
    for (size_t t = 0; t < n_terms; t++) {
        const uint32_t kind = term_kind[t], idx = term_index[t];
        col[t] = (uint32_t)(kind <= 2 ? 3 * idx + kind : kind == 3 ? 3 * n + idx : 3 * n + m);
        cnt[col[t] + 1]++;
    }
    for (size_t i = 0; i < ncols; i++) cnt[i + 1] += cnt[i];
    col_ptr = cnt;
    ents.resize(n_terms);
    std::vector<uint32_t> fill(cnt.begin(), cnt.end() - 1);
    for (size_t q = 0; q < n_constraints; q++)   // constraint order within each list: the reference's summation order
        for (uint32_t t = row_ptr[q]; t < row_ptr[q + 1]; t++) {
            r1cs_ent &e = ents[fill[col[t]]++];
            e.q = (uint32_t)q;
            e.chal = term_challenge[t] == R1_NO_CHAL ? R1_NO_CHAL : (term_challenge[t] | (term_power[t] << 16));
            sc cf;
            memcpy(cf.v, term_coeff + (size_t)t * 32, 32);
            if (term_kind[t] == 3 || term_kind[t] == 4) sc_neg(cf, cf);   // wV -= .., wc -= .. (verifier.rs:286-292)
            sc28 cm;
            sc_to_mont28(cm, cf);
            memcpy(e.coeff, cm.v, 40);
        }
}

// the launch shape of `nbatch` proofs of a circuit (n_one: length of its ONE list) on generators of capacity gens_capacity; the rng
// fields (seeded, seed) are the caller's
inline void r1cs_shape_of(r1cs_shape &sh, uint32_t m, uint32_t n1, uint32_t n, uint32_t pn, uint32_t k, uint32_t two_phase, uint32_t nch, uint32_t Q,
                          uint32_t n_one, size_t proof_stride, size_t nbatch, size_t gens_capacity) {
    sh.m = m, sh.n1 = n1, sh.n = n, sh.pn = pn, sh.k = k;
    sh.two_phase = two_phase, sh.nch = nch, sh.Q = Q;
    sh.nzhi = (Q >> 6) + 1;
    sh.nyhi = ((pn - 1) >> 6) + 1;
    sh.f_zlo = R1F_FIXED;
    sh.f_zhi = sh.f_zlo + 64;
    sh.f_ylo = sh.f_zhi + sh.nzhi;
    sh.f_yhi = sh.f_ylo + 64;
    sh.f_ch = sh.f_yhi + sh.nyhi;
    sh.f_tab = sh.f_ch + sh.nch;
    sh.nfields = sh.f_tab + 2 * sh.k;
    sh.U = 11 + sh.m + 2 * sh.k;
    sh.proof_stride = (uint32_t)proof_stride;
    sh.nproofs = (uint32_t)nbatch;
    sh.one_chunks = n_one ? (n_one + R1_ONE_CHUNK - 1) / R1_ONE_CHUNK : 1;
    sh.gens_short = pn > gens_capacity ? 1u : 0u;   // verifier.rs:341-343 (a single-party proof: party 0)
}

}  // namespace bp
#endif
