// Host harness for the inner-product / linear entry points on the callers' own transcripts: the front-end lanes that start from per-proof
// states and apply innerproduct_domain_sep themselves (ipp_prepare_lane<true>, ipp_vs_front_lane<true>, lin_prepare_lane<true>), the state
// fill in front of the inner-product prover (ipp_ts_fill_thread) and the linear prover's public lane under either draw source
// (linc_public_lane), compiled with g++ and driven lane by lane, the way k_ipp_prepare_ts / k_ipp_vs_front_ts / k_lin_prepare_ts /
// k_ipp_ts_fill / k_linc_public(_ts) run them.  TEST-ONLY: never part of libbpgpu.so, never a fallback.
#define BP_FE_CHECK 1
#include "../../bulletproofs_amd/csrc/ipp.h"
#include "../../bulletproofs_amd/csrc/linear.h"
#include "../../bulletproofs_amd/csrc/linear_prover.h"
using namespace bp;

// where the lanes start: ts_in with ts_in_stride words (0 or 52) between the states, or -- by_value != 0 -- the one state at ts_in handed
// over as the kernels' `init` argument (what the _dev forms do with a host-side shared_transcript)
struct start_of {
    rp_strobe_init init;
    const uint32_t *ts_in;
    start_of(const uint32_t *ts, int by_value) : init{}, ts_in(ts) {
        if (by_value) {
            for (int i = 0; i < 50; i++) init.w[i] = ts[i];
            init.pos = ts[50] & 0xffu;
            init.pos_begin = (ts[50] >> 8) & 0xffu;
            init.cur_flags = (ts[50] >> 16) & 0xffu;
            ts_in = nullptr;
        }
    }
};

// the shape as ipp_verify_dev_locked / ipp_rlc_dev_locked (bpgpu.hip) build it from (n, proof_len); -1: no InnerProductProof length
static int ipp_shape_of(ipp_shape &sh, uint32_t n, uint32_t nproofs, uint32_t proof_len, uint32_t bases_shared) {
    if (proof_len % 32 || proof_len / 32 < 2 || (proof_len / 32 - 2) % 2) return -1;
    const uint32_t k = (proof_len / 32 - 2) / 2;
    if (k > BP_RP_MAX_K) return -1;
    const bool bad = n != (1u << k);
    sh.n = bad ? 0 : n;
    sh.k = k;
    sh.N = bad ? 2 : 2 * n + 2 * k + 2;
    sh.proof_len = proof_len;
    sh.nproofs = nproofs;
    sh.shape_verdict = bad ? BP_VERDICT_VERIFICATION : 0;
    sh.bases_shared = bases_shared;
    return 0;
}

// scalars, points: [nproofs][N][8] words (pre-zeroed by the caller, as the host does), N = 2n + 2 lg n + 2 (2 when n != 2^k); returns N
extern "C" int iplts_ipp_prepare(uint32_t n, uint32_t nproofs, const uint8_t *proofs, uint32_t proof_len, const uint8_t *Gf, const uint8_t *Hf,
                                 const uint8_t *P, const uint8_t *Q, const uint8_t *G, const uint8_t *H, uint32_t bases_shared, const uint32_t *ts_in,
                                 uint32_t ts_in_stride, int by_value, uint32_t *scalars, uint32_t *points, uint32_t *status, uint32_t *ts_out) {
    ipp_shape sh;
    if (ipp_shape_of(sh, n, nproofs, proof_len, bases_shared)) return -1;
    const start_of from(ts_in, by_value);
    for (uint32_t p = 0; p < nproofs; p++) {
        uint32_t w[50];
        kstate st;
        st.w = w, st.stride = 1;
        ipp_prepare_lane<true>(p, sh, from.init, st, proofs, Gf, Hf, P, Q, G, H, scalars, points, status, from.ts_in, ts_in_stride, ts_out);
    }
    return (int)sh.N;
}

// u_sq, u_inv_sq: [nproofs][k][8] words; tab: [nproofs][2k][10]
extern "C" int iplts_ipp_vs_front(uint32_t n, uint32_t nproofs, const uint8_t *proofs, uint32_t proof_len, const uint32_t *ts_in, uint32_t ts_in_stride,
                                  int by_value, uint32_t *u_sq, uint32_t *u_inv_sq, uint32_t *tab, uint32_t *status, uint32_t *ts_out) {
    ipp_shape sh;
    if (ipp_shape_of(sh, n, nproofs, proof_len, 1)) return -1;
    const start_of from(ts_in, by_value);
    for (uint32_t p = 0; p < nproofs; p++) {
        uint32_t w[50];
        kstate st;
        st.w = w, st.stride = 1;
        ipp_vs_front_lane<true>(p, sh, from.init, st, proofs, from.ts_in, ts_in_stride, u_sq, u_inv_sq, tab, ts_out, status);
    }
    return (int)sh.k;
}

// ts: [nproofs][52] words out: every state behind the separator
extern "C" void iplts_ts_fill(uint32_t n, uint32_t nproofs, const uint32_t *ts_in, uint32_t ts_in_stride, uint32_t *ts) {
    for (uint32_t p = 0; p < nproofs; p++) {
        uint32_t w[50];
        kstate st;
        st.w = w, st.stride = 1;
        ipp_ts_fill_thread(p, n, st, ts_in, ts_in_stride, ts);
    }
}

// the shape as lin_front_dev_locked builds it, explicit bases (gen_sc == NULL) or generator-table mode; returns N (terms per proof in the lists)
extern "C" int iplts_lin_prepare(uint32_t n, uint32_t nproofs, const uint8_t *proofs, uint32_t proof_len, const uint8_t *C, const uint8_t *b,
                                 uint32_t b_shared, const uint8_t *G, const uint8_t *F, const uint8_t *B, const uint32_t *ts_in, uint32_t ts_in_stride,
                                 int by_value, uint32_t *scalars, uint32_t *points, uint32_t *status, uint32_t *ts_out, uint32_t *gen_sc) {
    if (proof_len % 32 || proof_len / 32 < 3 || (proof_len / 32 - 3) % 2) return -1;
    const uint32_t k = (proof_len / 32 - 3) / 2;
    if (k > BP_RP_MAX_K) return -1;
    const bool bad = n != (1u << k);
    lin_shape sh;
    sh.n = bad ? 0 : n;
    sh.k = k;
    sh.proof_len = proof_len;
    sh.nproofs = nproofs;
    sh.shape_verdict = bad ? BP_VERDICT_VERIFICATION : 0;
    sh.b_shared = b_shared;
    sh.fixed = gen_sc ? 1 : 0;
    sh.N = gen_sc ? 2 * k + 2 : bad ? 4 : n + 2 * k + 4;
    const start_of from(ts_in, by_value);
    for (uint32_t p = 0; p < nproofs; p++) {
        uint32_t w[50];
        kstate st;
        st.w = w, st.stride = 1;
        lin_prepare_lane<true>(p, sh, from.init, st, proofs, C, b, G, F, B, scalars, points, status, ts_out, gen_sc, from.ts_in, ts_in_stride, n);
    }
    return (int)sh.N;
}

// a draw source that counts the requests for an index at or past D = 2 lg n + 2
template <class Src>
struct counted {
    Src src;
    uint32_t D, nproofs;
    uint32_t *bad;
    void draw(sc &r, const rpp_shape &sh, uint32_t p, uint32_t d) const {
        if (d >= D || p >= nproofs) {
            ++*bad;
            sc_0(r);
            return;
        }
        src.draw(r, sh, p, d);
    }
};

// The linear prover's public lane for every proof.  seeded: `randomness` holds 32 bytes per proof, else 64 (2 lg n + 2) per proof.
// sep: the lanes start from ts_in (ts_in_stride words apart) and apply the separator; else ts holds the separated states on entry.
// legacy: the buffer-fed wrapper the existing kernel calls (linc_public_thread; seeded = sep = 0).
// Returns the number of draws a lane asked for at an index >= D.
extern "C" int iplts_linc_public(int seeded, int sep, int legacy, uint32_t n, uint32_t nproofs, const uint8_t *C, const uint8_t *b, uint32_t b_shared,
                                 const uint8_t *G, const uint8_t *F, const uint8_t *B, const uint8_t *r_in, const uint8_t *randomness,
                                 const uint32_t *ts_in, uint32_t ts_in_stride, uint32_t *ts, uint32_t *r_out, uint32_t *draws, uint32_t *status) {
    linc_shape sh;
    sh.n = n, sh.k = 0, sh.nproofs = nproofs, sh.b_shared = b_shared;
    while ((1u << sh.k) < n) sh.k++;
    uint32_t bad = 0;
    const uint32_t D = 2 * sh.k + 2;
    for (uint32_t p = 0; p < nproofs; p++) {
        uint32_t w[50];
        kstate st;
        st.w = w, st.stride = 1;
        const counted<rpp_from_seed> s_seed{rpp_from_seed{randomness}, D, nproofs, &bad};
        const counted<rpp_from_bytes> s_bytes{rpp_from_bytes{randomness}, D, nproofs, &bad};
        if (legacy) linc_public_thread(p, sh, st, C, b, G, F, B, r_in, randomness, ts, r_out, draws, status);
        else if (seeded && sep) linc_public_lane<true>(p, sh, st, C, b, G, F, B, r_in, s_seed, ts_in, ts_in_stride, ts, r_out, draws, status);
        else if (seeded) linc_public_lane<false>(p, sh, st, C, b, G, F, B, r_in, s_seed, nullptr, 0, ts, r_out, draws, status);
        else if (sep) linc_public_lane<true>(p, sh, st, C, b, G, F, B, r_in, s_bytes, ts_in, ts_in_stride, ts, r_out, draws, status);
        else linc_public_lane<false>(p, sh, st, C, b, G, F, B, r_in, s_bytes, nullptr, 0, ts, r_out, draws, status);
    }
    return (int)bad;
}
