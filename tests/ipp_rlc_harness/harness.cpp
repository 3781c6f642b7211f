// Host harness for the batch-combined InnerProductProof check: ipp_rlc.h's per-lane bodies (and ipp.h's ipp_vs_front_thread, its front
// end) compiled with g++ and driven lane by lane, the way k_ipp_vs_front / k_rlc_comb_rho / k_ipp_rlc_uniq / k_ipp_rlc_weigh /
// k_rlc_comb_reduce (explicit bases: k_ipp_rlc_reduce) run them.  TEST-ONLY: never part of libbpgpu.so, never a fallback.
#define BP_FE_CHECK 1
#include "../../bulletproofs_amd/csrc/ipp_rlc.h"
#include <vector>
using namespace bp;

// rho of proof p: from the caller's 64 bytes (weights64 != NULL) or drawn under key32
extern "C" void ipprlc_rho(const uint8_t *weights64, const uint8_t *key32, uint32_t p, uint32_t *rho) {
    ipp_rlc_key key{};
    if (key32) memcpy(key.w, key32, 32);
    ipp_rlc_rho_thread(p, weights64, key, rho);
}
extern "C" uint32_t ipprlc_weight_domain() { return IPP_RLC_WEIGHT_DOMAIN; }

// the Montgomery table [2k][10] that ipp_vs_front_thread leaves for one proof, from k challenges and their inverses (canonical, 8 words each)
extern "C" void ipprlc_make_table(uint32_t k, const uint32_t *u, const uint32_t *uinv, uint32_t *tab) {
    for (uint32_t j = 0; j < k; j++) {
        sc a, b;
        sc28 am, bm;
        for (int q = 0; q < 8; q++) a.v[q] = u[8 * j + q], b.v[q] = uinv[8 * j + q];
        sc_to_mont28(am, a);
        sc_to_mont28(bm, b);
        for (int q = 0; q < 10; q++) tab[(2 * j) * 10 + q] = am.v[q], tab[(2 * j + 1) * 10 + q] = bm.v[q];
    }
}

// the front end of nproofs proofs on one start state (208 bytes; innerproduct_domain_sep(n) is applied here, as the runtime does on the host):
// status, u_sq / u_inv_sq ([proof][k][8], zeroed first) and tab ([proof][2k][10])
extern "C" int ipprlc_front(uint32_t n, uint32_t nproofs, const uint8_t *proofs, uint32_t proof_len, const uint8_t *state208, uint32_t *status,
                            uint32_t *u_sq, uint32_t *u_inv_sq, uint32_t *tab) {
    if (proof_len % 32 || proof_len < 64 || ((proof_len / 32 - 2) & 1)) return -1;
    const uint32_t k = (proof_len / 32 - 2) / 2;
    ipp_shape sh;
    sh.n = n, sh.k = k, sh.N = 0, sh.proof_len = proof_len, sh.nproofs = nproofs, sh.shape_verdict = (n != (1u << k)) ? BP_VERDICT_VERIFICATION : 0, sh.bases_shared = 1;
    rp_strobe_init init;
    memset(&init, 0, sizeof init);
    memcpy(init.w, state208, 200);
    kstate st0;
    st0.w = init.w, st0.stride = 1;
    strobe t;
    t.st = st0, t.pos = state208[200], t.pos_begin = state208[201], t.cur_flags = state208[202];
    const uint8_t dom[7] = {'d', 'o', 'm', '-', 's', 'e', 'p'}, ipp[6] = {'i', 'p', 'p', ' ', 'v', '1'}, ln[1] = {'n'};
    merlin_append_message(t, dom, 7, ipp, 6);
    merlin_append_u64(t, ln, 1, n);
    init.pos = t.pos, init.pos_begin = t.pos_begin, init.cur_flags = t.cur_flags;
    for (uint32_t p = 0; p < nproofs; p++) status[p] = 0;
    for (size_t i = 0; i < (size_t)nproofs * k * 8; i++) u_sq[i] = u_inv_sq[i] = 0;
    for (uint32_t p = 0; p < nproofs; p++) {
        uint32_t w[50];
        kstate st;
        st.w = w, st.stride = 1;
        ipp_vs_front_thread(p, sh, init, st, proofs, nullptr, u_sq, u_inv_sq, tab, nullptr, status);
    }
    return 0;
}

// every lane of the uniq launch, every lane of the weigh launch (nstride = nproofs rounded up to 64 proofs per row, whole wavefronts) with
// the coefficients summed as rlc.h's limb sums, then every lane of the reduce launch.  fixed: generator-table mode -- rows (B_blinding, B,
// G_0.., H_0..) to row_out ((2n + 2) x 8 words), the unique terms from slot 0 of comb_sc / comb_pt (nproofs U slots); else the 2n rows are
// the head of the combined list (2n + nproofs U slots) with the encodings of G, H beside them.  ab: [proof][2][10] scratch.  Every row a
// lane names, padding included, must lie inside the accumulators, and the blocks' Gray-code walks (B rows per lane: 1, or
// min(IPP_RLC_BLOCK, n) as the runtime picks it for large launches) must cover every row once.
extern "C" int ipprlc_run(uint32_t nproofs, uint32_t n, uint32_t k, int fixed, uint32_t B, const uint32_t *status, const uint32_t *rho, const uint8_t *proofs,
                          const uint8_t *P, const uint8_t *Q, const uint32_t *u_sq, const uint32_t *u_inv_sq, const uint32_t *tab, const uint8_t *Gf,
                          const uint8_t *Hf, const uint8_t *G, const uint8_t *H, uint32_t *ab, uint32_t *comb_sc, uint32_t *comb_pt, uint32_t *row_out) {
    const uint32_t nstride = (nproofs + 63) / 64 * 64, U = 2 * k + 2, nrows = 2 * n + (fixed ? 2u : 0u);
    if (B == 0 || n % B != 0) return -1;
    ipp_rlc_shape sh{nproofs, nstride, n, k, U, 32 * U, fixed ? 2u : 0u, fixed ? 0u : 2 * n, B};
    for (uint32_t p = 0; p < nproofs; p++) ipp_rlc_uniq_thread(p, sh, status, rho, proofs, P, Q, u_sq, u_inv_sq, ab, comb_sc, comb_pt);
    std::vector<uint64_t> acc((size_t)nrows * 10, 0);
    std::vector<uint8_t> seen(2 * n, 0);
    const uint32_t nt = nstride * (2 * n / B);
    for (uint32_t tid = 0; tid < nt; tid++) {
        ipp_rlc_lane ln;
        ipp_rlc_weigh_begin(tid, sh, status, ab, tab, Gf, Hf, ln);
        for (uint32_t g = 0; g < B; g++) {
            sc v;
            uint32_t row;
            const bool active = ipp_rlc_weigh_step(g, sh, ln, v, row);
            if (row >= nrows) return -2;          // the wavefront's atomic would land past the accumulators
            const uint32_t r = (tid / nstride) * B + (g ^ (g >> 1));
            if (row != (fixed ? 2u : 0u) + r) return -3;   // (every lane of a wavefront names the same row at step g)
            if (tid % nstride == 0) seen[r]++;
            if (!active) continue;
            uint64_t l[10];
            rlc_limbs(l, v);
            for (int i = 0; i < 10; i++) acc[(size_t)row * 10 + i] += l[i];
        }
    }
    for (uint32_t r = 0; r < 2 * n; r++)
        if (seen[r] != 1) return -4;              // every row is walked exactly once per proof
    for (uint32_t g = 0; g < nrows; g++) {
        if (fixed) rlc_reduce_thread(g, acc.data(), row_out);
        else ipp_rlc_reduce_thread(g, n, acc.data(), G, H, comb_sc, comb_pt);
    }
    return 0;
}

#ifdef IPPRLC_MAIN
// stand-alone sanitizer run: a synthetic batch of 65 proofs at n = 16 in both modes (two proofs stopped), checked only for memory
// and arithmetic faults and for the lanes' own return codes
#include <cstdio>
int main() {
    const uint32_t nproofs = 65, n = 16, k = 4, U = 2 * k + 2;
    uint32_t x = 12345;
    auto next = [&]() { return x = x * 1664525u + 1013904223u; };
    std::vector<uint32_t> status(nproofs, 0), rho(8 * nproofs), us(8 * k * nproofs), ui(8 * k * nproofs), tab(20 * k * nproofs), ab(20 * nproofs);
    std::vector<uint8_t> proofs(32 * U * nproofs), P(32 * nproofs), Q(32 * nproofs), Gf(32 * n * nproofs), Hf(32 * n * nproofs), G(32 * n), H(32 * n), w64(64 * nproofs);
    status[3] = 1, status[64] = 2;
    for (auto *v : {&proofs, &P, &Q, &Gf, &Hf, &G, &H, &w64})
        for (auto &b : *v) b = (uint8_t)(next() >> 24);
    for (auto *v : {&us, &ui})
        for (size_t i = 0; i < v->size(); i++) (*v)[i] = (i % 8 == 7) ? next() >> 5 : next();
    for (uint32_t p = 0; p < nproofs; p++) {
        ipprlc_rho(w64.data(), nullptr, p, rho.data());
        ipprlc_make_table(k, us.data() + 8 * k * p, ui.data() + 8 * k * p, tab.data() + 20 * k * p);
    }
    for (int fixed = 0; fixed < 4; fixed++) {
        const size_t slots = ((fixed & 1) ? 0 : 2 * n) + (size_t)nproofs * U;
        std::vector<uint32_t> csc(8 * slots), cpt(8 * slots), row(8 * (2 * n + 2));
        const int rc = ipprlc_run(nproofs, n, k, fixed & 1, (fixed & 2) ? IPP_RLC_BLOCK : 1u, status.data(), rho.data(), proofs.data(), P.data(), Q.data(), us.data(), ui.data(), tab.data(), Gf.data(),
                                  Hf.data(), G.data(), H.data(), ab.data(), csc.data(), cpt.data(), row.data());
        if (rc) {
            printf("ipprlc_run(fixed=%d) = %d\n", fixed, rc);
            return 1;
        }
    }
    printf("ok\n");
    return 0;
}
#endif
