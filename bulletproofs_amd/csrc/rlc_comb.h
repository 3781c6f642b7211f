// The lane bodies that the combined checks ending in ONE multiscalar multiplication share (r1cs_rlc.h, linear_rlc.h, rlc_mix.h):
//   rlc_draw_thread    : lane = proof   64 library-drawn bytes of a domain
//   rlc_rho_thread     : lane = proof   its weight rho_p, from the caller's 64 bytes or drawn
//   rlc_weigh_thread   : lane = (term, proof), proof fastest   unique terms times rho_p into the combined list, shared terms times rho_p
//                                       for rlc.h's limb sums; the family supplies where a term lies and which row it lands on
//   rlc_reduce_thread  : lane = row     the accumulated coefficient mod l
//   rlc_verdict_thread : lane = proof   its front-end code, else OK when R decoded and is the identity, else undecided
// The soundness of every such check rests on the weight derivation and the verdict rule: both live here only.  The weight domains stay
// with their families (two checks never share a ChaCha20 nonce).
#ifndef BPGPU_RLC_COMB_H
#define BPGPU_RLC_COMB_H
#include "rangeproof.h"
#include "rlc.h"
#include "chacha20.h"

namespace bp {

#define RLC_GSTATUS_DONE 0xffffffffu   // gstatus of a proof whose verdict is written already (no verdict code takes this value)

// the per-call ChaCha20 key of the randomness the caller did not bring
struct rlc_key {
    uint32_t w[8];
};

// the 64 bytes of the call's proof gp in domain `dom` (16 little-endian words: what a caller's rng64 / weights64 row would hold): block gp
// of ChaCha20(key, nonce = dom)
BP_HD void rlc_draw_thread(uint32_t gp, const rlc_key &key, uint32_t dom, uint32_t *out) {
    uint32_t w16[16];
    chacha20_block(key.w, (uint64_t)gp, dom, 0u, w16);
#pragma unroll
    for (int i = 0; i < 16; i++) out[16 * (uint64_t)gp + i] = w16[i];
}

// rho of the call's proof gp: from_bytes_mod_order_wide(weights64[gp]), or of block gp of ChaCha20(key, nonce = dom)
BP_HD void rlc_rho_thread(uint32_t gp, const uint8_t *weights64, const rlc_key &key, uint32_t dom, uint32_t *rho) {
    uint32_t w16[16];
    if (weights64) {
        const uint8_t *src = weights64 + 64 * (uint64_t)gp;
        for (int i = 0; i < 16; i++)
            w16[i] = (uint32_t)src[4 * i] | ((uint32_t)src[4 * i + 1] << 8) | ((uint32_t)src[4 * i + 2] << 16) | ((uint32_t)src[4 * i + 3] << 24);
    } else {
        chacha20_block(key.w, (uint64_t)gp, dom, 0u, w16);
    }
    sc r;
    sc_from_wide(r, w16);
    store_words8(rho + 8 * (uint64_t)gp, r);
}

// lane tid = term * nstride + proof, over U unique terms and then the family's shared terms; nstride: nproofs rounded up to 64 (the
// lanes of the padding add nothing), so that the 64 lanes of a wavefront share their term.  rho, comb_sc, comb_pt start at the first
// proof's weight and slot.  MAP is the family's index map:
//   map.uniq(p, t)    the slot in src_sc / src_pt of unique term t of proof p
//   map.shared(p, g)  the 8 words of proof p's coefficient of shared term g
//   map.row(g)        the combined row of shared term g
// A unique term goes to slot p U + t of the combined list (scalar 0 and the identity encoding for a proof that stopped); a shared term
// sets its combined row `row` (also in the padding lanes: it is the wavefront's row) and returns true with its weighted coefficient `v`
// for the caller's accumulation (false for a proof that stopped and for the padding).
template <class MAP>
BP_HD bool rlc_weigh_thread(uint32_t tid, uint32_t nproofs, uint32_t nstride, uint32_t U, const MAP &map, const uint32_t *status, const uint32_t *rho,
                            const uint32_t *src_sc, const uint32_t *src_pt, uint32_t *comb_sc, uint32_t *comb_pt, sc &v, uint32_t &row) {
    const uint32_t t = tid / nstride, p = tid - t * nstride;
    sc_0(v);
    row = t < U ? 0u : map.row(t - U);
    if (p >= nproofs) return false;
    const uint32_t st = status[p];
    sc x, r;
#pragma unroll
    for (int q = 0; q < 8; q++) r.v[q] = rho[8 * (uint64_t)p + q];
    if (t < U) {
        const uint64_t src = map.uniq(p, t) * 8, dst = ((uint64_t)p * U + t) * 8;
        if (st != 0) {
            sc_0(x);
#pragma unroll
            for (int q = 0; q < 8; q++) comb_pt[dst + q] = 0u;
        } else {
#pragma unroll
            for (int q = 0; q < 8; q++) {
                x.v[q] = src_sc[src + q];
                comb_pt[dst + q] = src_pt[src + q];
            }
            sc_mul(x, x, r);
        }
        store_words8(comb_sc + dst, x);
        return false;
    }
    if (st != 0) return false;
    const uint32_t *src = map.shared(p, t - U);
#pragma unroll
    for (int q = 0; q < 8; q++) x.v[q] = src[q];
    sc_mul(v, x, r);
    return true;
}

// lane = row of a combination: the accumulated coefficient mod l to out_sc[row]
BP_HD void rlc_reduce_thread(uint32_t row, const uint64_t *acc, uint32_t *out_sc) {
    uint64_t a[10];
#pragma unroll
    for (int i = 0; i < 10; i++) a[i] = acc[(uint64_t)row * 10 + i];
    sc s;
    rlc_acc_to_sc(s, a);
    store_words8(out_sc + (uint64_t)row * 8, s);
}

// verdict of the call's proof gp: nothing where gstatus says it is written already; else its front-end code; else 0 when R is the
// identity and every point decoded, else undecided (the host then re-verifies proof by proof).  res: the 8 words of compress(R),
// rst: its status byte (0 = every point decoded).  Lane 0 also writes the 33 batch bytes.
BP_HD void rlc_verdict_thread(uint32_t gp, const uint32_t *gstatus, const uint32_t *res, const uint8_t *rst, uint8_t *verdict, uint8_t *batch_out) {
    uint32_t nz = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) nz |= res[i];
    const bool dec = rst[0] == 0, pass = dec && nz == 0;
    const uint32_t st = gstatus[gp];
    if (st != RLC_GSTATUS_DONE) verdict[gp] = st ? (uint8_t)st : (pass ? (uint8_t)BP_VERDICT_OK : (uint8_t)BP_VERDICT_UNDECIDED);
    if (gp == 0) {
        batch_out[0] = pass ? 0 : 1;
        for (int i = 0; i < 32; i++) batch_out[1 + i] = dec ? (uint8_t)(res[i >> 2] >> (8 * (i & 3))) : 0;
    }
}

}  // namespace bp
#endif
