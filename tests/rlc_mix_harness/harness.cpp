// Host harness for the batch-combined check over range proofs of mixed shapes: rlc_mix.h's per-lane bodies compiled with g++ and driven
// lane by lane, the way k_rlc_mix_draw / k_rlc_mix_weigh / k_rlc_comb_reduce run them.  TEST-ONLY: never part of libbpgpu.so, never a fallback.
#define BP_FE_CHECK 1
#include "../../bulletproofs_amd/csrc/rlc_mix.h"
#include <vector>
using namespace bp;

extern "C" uint32_t rlcmix_gen_row(uint32_t g, uint32_t n, uint32_t m, uint32_t N, uint32_t M) { return rm_gen_row(g, n, m, N, M); }

// the 64 library-drawn bytes of the call's proof gp: which = 0 the combination weight, 1 the batching challenge's rng bytes
extern "C" void rlcmix_draw(const uint8_t *key32, uint32_t gp, int which, uint8_t *out64) {
    rm_key key;
    memcpy(key.w, key32, 32);
    std::vector<uint32_t> buf(16 * ((size_t)gp + 1), 0);
    rm_draw_thread(gp, key, which ? RM_RNG_DOMAIN : RM_WEIGHT_DOMAIN, buf.data());
    memcpy(out64, buf.data() + 16 * (size_t)gp, 64);
}

// one group: every lane of the weigh launch (nstride = nproofs rounded up to 64 proofs per term, whole wavefronts).  row0 / row1: the
// weighted B_blinding / B coefficients launch 1 leaves in the RPF_ROW0 / RPF_ROW1 fields; coef: [proof][2 n m][8] the weighted G then H
// coefficients, standing in for rp_expand_b4_thread (zero for a stopped proof there too).  The limb sums go on top of acc
// ((2 N M + 2) x 10), which the groups of a call share.  Every row a lane names, padding included, must lie inside acc.
extern "C" int rlcmix_weigh_group(uint32_t nproofs, uint32_t n, uint32_t m, uint32_t k, uint32_t N, uint32_t M, uint32_t gp0, uint32_t u0,
                                  const uint8_t *proofs, const uint8_t *commitments, const uint32_t *status, const uint32_t *row0, const uint32_t *row1,
                                  const uint32_t *uniq_sc, const uint32_t *coef, uint32_t *comb_sc, uint32_t *comb_pt, uint32_t *gstatus, uint64_t *acc) {
    rp_shape sh;
    sh.n = n, sh.m = m, sh.nm = n * m, sh.k = k, sh.U = 4 + 2 * k + m, sh.proof_len = 32 * (9 + 2 * k), sh.nproofs = nproofs, sh.shape_verdict = 0;
    rm_group gr{nproofs, (nproofs + 63) / 64 * 64, n, m, N, M, gp0, u0};
    const rp_fields fl = rp_field_layout(k, m);
    std::vector<uint32_t> fields((size_t)fl.count * nproofs * BP_RP_REC, 0xdeadbeefu);
    for (uint32_t p = 0; p < nproofs; p++) {
        sc a, b;
        for (int i = 0; i < 8; i++) a.v[i] = row0[8 * p + i], b.v[i] = row1[8 * p + i];
        rp_store(fields.data(), nproofs, RPF_ROW0, p, a);
        rp_store(fields.data(), nproofs, RPF_ROW1, p, b);
    }
    const uint32_t nrows = 2 * N * M + 2, nt = gr.nstride * rm_terms(sh);
    auto add = [&](uint32_t row, const sc &v) {
        uint64_t l[10];
        rlc_limbs(l, v);
        for (int i = 0; i < 10; i++) acc[(size_t)row * 10 + i] += l[i];
    };
    for (uint32_t tid = 0; tid < nt; tid++) {
        uint32_t p, q;
        bool live;
        sc r0, r1;
        const uint32_t role = rm_weigh_thread(tid, gr, sh, proofs, commitments, status, fields.data(), uniq_sc, comb_sc, comb_pt, gstatus, p, q, live, r0, r1);
        if (role == 1 && live) {
            add(0, r0);
            add(1, r1);
        } else if (role == 2) {
            for (uint32_t j = 0; j < 4; j++) {
                uint32_t row_g, row_h;
                rm_quad_rows(gr, q, j, row_g, row_h);
                if (row_g >= nrows || row_h >= nrows) return -2;   // the wavefront's atomic would land past the accumulators
                if (!live) continue;
                sc g, h;
                for (int i = 0; i < 8; i++) {
                    g.v[i] = coef[((size_t)p * 2 * sh.nm + 4 * q + j) * 8 + i];
                    h.v[i] = coef[((size_t)p * 2 * sh.nm + sh.nm + 4 * q + j) * 8 + i];
                }
                add(row_g, g);
                add(row_h, h);
            }
        }
    }
    return 0;
}

extern "C" void rlcmix_reduce(uint32_t nrows, const uint64_t *acc, uint32_t *gen_row_out) {
    for (uint32_t g = 0; g < nrows; g++) rlc_reduce_thread(g, acc, gen_row_out);
}
