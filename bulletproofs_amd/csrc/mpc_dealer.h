// The DEALER side of the multi-party aggregation protocol (src/range_proof/dealer.rs), batched and stateless: rows are sessions
// of one shape (n, m).
//     step 4  Dealer::new + receive_bit_commitments (dealer.rs:37-137):  V_j as given, A = sum A_j, S = sum S_j   -> y, z
//     step 5  receive_poly_commitments (dealer.rs:160-197):              T_1 = sum T_1_j, T_2 = sum T_2_j          -> x
//     step 6  assemble_shares / receive_shares (dealer.rs:226-380):      sums, w, the inner-product argument       -> proof
// The point sums are a decode-add-compress kernel of their own (mpc_ptsum_thread); the transcript steps between them absorb a
// handful of 32-byte messages per session and run on the host with the library's Merlin code (keccak.h, BP_HD); the
// inner-product argument is ippc_core's, over G(n, m), H(n, m) from the generator tables.
#ifndef BPGPU_MPC_DEALER_H
#define BPGPU_MPC_DEALER_H
#include "mpc_party.h"

namespace bp {

// lane = (session p, column c < ncol): out[p * ncol + c] = compress(sum_j decode(in[(p m + j) * rec + off + 32 c])).
// An encoding that does not decode marks the session (status pre-zeroed) and its sums are not used.
BP_HD void mpc_ptsum_thread(uint32_t tid, uint32_t m, uint32_t ncol, uint32_t rec, uint32_t off, const uint8_t *in, uint32_t *out, uint32_t *status) {
    const uint32_t p = tid / ncol, c = tid - p * ncol;
    ge_ext acc;
    ge_identity(acc);
    bool bad = false;
    for (uint32_t j = 0; j < m; j++) {
        uint32_t w[8];
        load_words8(w, in + ((uint64_t)p * m + j) * rec + off + 32 * c);
        ge_ext q;
        if (!ristretto_decompress(q, w)) {
            bad = true;
            continue;
        }
        if (j == 0) acc = q;
        else ge_add(acc, acc, q);
    }
    uint32_t o[8];
    ristretto_compress(o, acc);
#pragma unroll
    for (int i = 0; i < 8; i++) out[8 * (uint64_t)tid + i] = bad ? 0u : o[i];
    if (bad) status[p] = MPC_ST_BAD_POINT;
}

// session p: t_x, t_x_blinding, e_blinding summed over its m shares (dealer.rs:262-266) and which parties sent a non-canonical
// scalar (bad[j] = 1; upstream they are Scalars by type).  share_len = 32 (3 + 2n).  Returns true when every scalar is canonical.
BP_HD bool mpc_sum_shares(uint32_t n, uint32_t m, const uint8_t *shares /*this session's*/, sc &t_x, sc &t_x_bl, sc &e_bl, uint8_t *bad /*[m]*/) {
    sc_0(t_x);
    sc_0(t_x_bl);
    sc_0(e_bl);
    bool all = true;
    for (uint32_t j = 0; j < m; j++) {
        const uint8_t *sb = shares + (uint64_t)j * 32 * (3 + 2 * n);
        bool ok = true;
        for (uint32_t i = 0; i < 3 + 2 * n; i++) {
            sc x;
            load_words8(x.v, sb + 32 * i);
            ok = ok && sc_is_canonical_sc(x);
        }
        if (bad) bad[j] = ok ? 0 : 1;
        all = all && ok;
        if (!ok) continue;
        sc x;
        load_words8(x.v, sb);
        sc_add(t_x, t_x, x);
        load_words8(x.v, sb + 32);
        sc_add(t_x_bl, t_x_bl, x);
        load_words8(x.v, sb + 64);
        sc_add(e_bl, e_bl, x);
    }
    return all;
}

// lane = (session p, index q < nm): the inner-product argument's inputs (dealer.rs:281-293): a = l_vec, b = r_vec concatenated in
// party order, G_factors = 1, H_factors = y^-q.  yinv [nsessions][8].  skip[p] != 0: the session is void (zeros in, status later).
BP_HD void mpc_vectors_thread(uint32_t tid, uint32_t n, uint32_t m, const uint8_t *shares, const uint32_t *yinv, const uint8_t *skip, uint32_t *a_vec,
                              uint32_t *b_vec, uint32_t *Gf, uint32_t *Hf) {
    const uint32_t nm = n * m, p = tid / nm, q = tid - p * nm, j = q / n, i = q - j * n;
    sc a, b, one, r, base;
    sc_from_u32(one, 1);
    sc_0(a);
    sc_0(b);
    if (!skip[p]) {
        const uint8_t *sb = shares + ((uint64_t)p * m + j) * 32 * (3 + 2 * n);
        load_words8(a.v, sb + 96 + 32 * i);
        load_words8(b.v, sb + 96 + 32 * (n + i));
    }
    ippc_st(a_vec + 8 * (uint64_t)tid, a);
    ippc_st(b_vec + 8 * (uint64_t)tid, b);
    ippc_st(Gf + 8 * (uint64_t)tid, one);
    ippc_ld(base, yinv + 8 * (uint64_t)p);
    r = one;                                   // y^-q by square and multiply
    for (uint32_t e = q; e; e >>= 1) {
        if (e & 1) sc_mul(r, r, base);
        sc_mul(base, base, base);
    }
    ippc_st(Hf + 8 * (uint64_t)tid, r);
}

}  // namespace bp
#endif
