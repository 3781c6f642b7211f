// Host harness for the batch-combined R1CS check: r1cs_rlc.h's per-lane bodies, and the ones of rlc_comb.h under them, compiled with g++
// and driven lane by lane, the way k_r1cs_rlc_weigh / k_rlc_comb_reduce / k_r1cs_rlc_sum / k_rlc_comb_verdict run them.  TEST-ONLY: never part of libbpgpu.so, never a fallback.
#define BP_FE_CHECK 1
#include "../../bulletproofs_amd/csrc/r1cs_rlc.h"
#include <vector>
using namespace bp;

// one slice: every lane of the weigh launch (nstride = nproofs rounded up to 64 proofs per term, whole wavefronts), the generator
// coefficients summed as rlc.h's limb sums, then reduced per row.  gens_short: the slice stopped in launch 1 -- no generator lanes, and
// pn may exceed PN.  Every row a lane names, padding included, must lie in [0, 2 PN + 2).  gen_row_out: (2 PN + 2) x 8 words.
extern "C" int r1rlc_weigh_slice(uint32_t nproofs, uint32_t U, uint32_t pn, uint32_t PN, int gens_short, uint32_t gp0, uint32_t u0,
                                 const uint32_t *status, const uint32_t *rho, const uint32_t *gen_sc, const uint32_t *uniq_sc,
                                 const uint32_t *uniq_pt, uint32_t *comb_sc, uint32_t *comb_pt, uint32_t *gstatus, uint32_t *gen_row_out) {
    const uint32_t nstride = (nproofs + 63) / 64 * 64, ngen = gens_short ? 0u : 2 * pn + 2;
    if (ngen && pn > PN) return -1;   // (the host refuses this: PN is the largest padded_n of the slices with generator terms)
    r1_rlc_slice sl{nproofs, nstride, U, ngen, pn, PN, gp0, u0};
    const uint32_t nrows = 2 * PN + 2;
    std::vector<uint64_t> acc((size_t)nrows * 10, 0);
    const uint32_t nt = nstride * (U + ngen);
    for (uint32_t tid = 0; tid < nt; tid++) {
        sc v;
        uint32_t row;
        const bool gen = r1_rlc_weigh_thread(tid, sl, status, rho, gen_sc, uniq_sc, uniq_pt, comb_sc, comb_pt, gstatus, v, row);
        if (tid / nstride < U) continue;          // (the kernel's wavefronts of unique terms do not accumulate)
        if (row >= nrows) return -2;              // the wavefront's atomic would land past the accumulators
        if (!gen) continue;
        uint64_t l[10];
        rlc_limbs(l, v);
        for (int i = 0; i < 10; i++) acc[(size_t)row * 10 + i] += l[i];
    }
    for (uint32_t g = 0; g < nrows; g++) rlc_reduce_thread(g, acc.data(), gen_row_out);
    return 0;
}

extern "C" uint32_t r1rlc_gen_row(uint32_t g, uint32_t pn, uint32_t PN) { return r1_rlc_gen_row(g, pn, PN); }

extern "C" void r1rlc_rho(const uint8_t *weights64, uint32_t gp, uint32_t *rho) {
    r1_rlc_key key{};
    r1_rlc_rho_thread(gp, weights64, key, rho);
}

// the one lane of the sum launch: the combinations' encodings and status bytes -> compress(R) and its status byte
extern "C" void r1cs_rlc_sum_lane(uint32_t ncomb, const uint32_t *parts, const uint8_t *part_status, uint32_t *res, uint8_t *rst) {
    r1_rlc_sum_thread(ncomb, parts, part_status, res, rst);
}

// every lane of the verdict launch the combined checks share, in descending order (lane 0's batch bytes must not depend on it)
extern "C" void rlc_comb_verdict_lanes(uint32_t n, const uint32_t *gstatus, const uint32_t *res, const uint8_t *rst, uint8_t *verdict, uint8_t *batch_out) {
    for (uint32_t gp = n; gp-- > 0;) rlc_verdict_thread(gp, gstatus, res, rst, verdict, batch_out);
}
