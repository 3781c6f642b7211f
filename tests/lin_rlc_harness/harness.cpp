// Host harness for the batch-combined LinearProof check: linear_rlc.h's per-lane bodies compiled with g++ and driven lane by lane, the
// way k_rlc_comb_rho / k_lin_rlc_weigh / k_rlc_comb_reduce (explicit bases: k_lin_rlc_reduce) run them.  TEST-ONLY: never part of libbpgpu.so, never a fallback.
#define BP_FE_CHECK 1
#include "../../bulletproofs_amd/csrc/linear_rlc.h"
#include <vector>
using namespace bp;

// rho of proof p: from the caller's 64 bytes (weights64 != NULL) or drawn under key32
extern "C" void linrlc_rho(const uint8_t *weights64, const uint8_t *key32, uint32_t p, uint32_t *rho) {
    lin_rlc_key key{};
    if (key32) memcpy(key.w, key32, 32);
    lin_rlc_rho_thread(p, weights64, key, rho);
}
extern "C" uint32_t linrlc_weight_domain() { return LIN_RLC_WEIGHT_DOMAIN; }

// every lane of the weigh launch (nstride = nproofs rounded up to 64 proofs per term, whole wavefronts), the base coefficients summed
// as rlc.h's limb sums, then every lane of the reduce launch.  fixed: generator-table staging (gen_sc: [proof][n + 2][8], lists of
// U = 2k + 2 terms) or the explicit-bases lists of n + 2k + 4 terms; comb_sc / comb_pt: (fixed ? 0 : n + 2) + nproofs U slots;
// row_out: (n + 2) x 8 words, the generator-table row (fixed only; with explicit bases the rows are the head of the combined list,
// with the encodings of B, F, G beside them).  Every row a lane names, padding included, must lie in [0, n + 2).
extern "C" int linrlc_weigh_reduce(uint32_t nproofs, uint32_t n, uint32_t k, int fixed, const uint32_t *status, const uint32_t *rho,
                                   const uint32_t *gen_sc, const uint32_t *list_sc, const uint32_t *list_pt, const uint8_t *B, const uint8_t *F,
                                   const uint8_t *G, uint32_t *comb_sc, uint32_t *comb_pt, uint32_t *row_out) {
    const uint32_t nstride = (nproofs + 63) / 64 * 64, U = 2 * k + 2, nrows = n + 2;
    lin_rlc_shape sh{nproofs, nstride, n, k, U, fixed ? 1u : 0u, fixed ? 0u : nrows};
    std::vector<uint64_t> acc((size_t)nrows * 10, 0);
    const uint32_t nt = nstride * (U + nrows);
    for (uint32_t tid = 0; tid < nt; tid++) {
        sc v;
        uint32_t row;
        const bool base = lin_rlc_weigh_thread(tid, sh, status, rho, gen_sc, list_sc, list_pt, comb_sc, comb_pt, v, row);
        if (tid / nstride < U) {                  // (the kernel's wavefronts of unique terms do not accumulate)
            if (base) return -1;
            continue;
        }
        if (row >= nrows) return -2;              // the wavefront's atomic would land past the accumulators
        if (!base) continue;
        uint64_t l[10];
        rlc_limbs(l, v);
        for (int i = 0; i < 10; i++) acc[(size_t)row * 10 + i] += l[i];
    }
    for (uint32_t g = 0; g < nrows; g++)
        lin_rlc_reduce_thread(g, acc.data(), B, F, G, fixed ? row_out : comb_sc, fixed ? nullptr : comb_pt);
    return 0;
}
