// Host harness for the front end of the mixed-shape combined check on caller-supplied transcripts: rlc_mix.h's lane body rm_front_thread in
// its two forms -- the per-shape script from ts_in (all states at one STROBE position) and the byte-wise replay (any positions) -- compiled
// with g++ and driven lane by lane, the way k_rlc_mix_front / k_rlc_mix_front_replay run it.  TEST-ONLY: never part of libbpgpu.so, never a
// fallback.
#define BP_FE_CHECK 1
#include "../../bulletproofs_amd/csrc/rlc_mix.h"
#include <cstring>
#include <vector>
using namespace bp;

extern "C" uint32_t rlcts_field_words(uint32_t n, uint32_t m, uint32_t nbatch) {
    uint32_t k = 0;
    while ((1u << k) < n * m) k++;
    return rp_field_layout(k, m).count * nbatch * BP_RP_REC;
}

// One group of nbatch proofs of shape (n, m), proof p from states208[p] with weight rho64[p] and rng bytes rng64[p].
// form 0: the script compiled for the states' common position with the domain separator (returns -2 when the states do not share one);
// form 1: the byte-wise replay with BP_TS_DOMSEP.  The sponge states live word-major in one 50 x 64-word block, lane t at word w * 64 + t,
// as the kernels' LDS.  Outputs: status (one byte per proof), the advanced states (nbatch x 208), the field store (rlcts_field_words words)
// and the U weighted coefficients per proof as plain scalars (nbatch x U x 8 words).
extern "C" int rlcts_front(uint32_t n, uint32_t m, uint32_t nbatch, const uint8_t *proofs, uint32_t proof_len, const uint8_t *commitments, const uint8_t *rng64,
                           const uint8_t *rho64, const uint8_t *states208, int form, uint8_t *status_out, uint8_t *ts_out208, uint32_t *fields_out,
                           uint32_t *uniq_out) {
    uint32_t k = 0;
    while ((1u << k) < n * m) k++;
    if (proof_len != 32 * (9 + 2 * k) || nbatch == 0) return -1;
    rp_shape sh;
    sh.n = n, sh.m = m, sh.nm = n * m, sh.k = k, sh.U = 4 + 2 * k + m, sh.proof_len = proof_len, sh.nproofs = nbatch, sh.shape_verdict = 0;
    uint32_t lg_m = 0;
    while ((1u << lg_m) < m) lg_m++;
    std::vector<uint32_t> ts_in((size_t)nbatch * BP_TS_WORDS, 0), ts_out((size_t)nbatch * BP_TS_WORDS, 7);
    bool uniform = true;
    for (uint32_t p = 0; p < nbatch; p++) {
        const uint8_t *st = states208 + (size_t)p * 208;
        if (st[200] != states208[200] || st[201] != states208[201] || st[202] != states208[202]) uniform = false;
        memcpy(&ts_in[(size_t)p * BP_TS_WORDS], st, 200);
        ts_in[(size_t)p * BP_TS_WORDS + 50] = rp_ts_meta(st[200], st[201], st[202]);
    }
    rp_strobe_init init;
    memset(&init, 0, sizeof init);   // only the position is shared; the words come from ts_in
    std::vector<uint32_t> img;
    if (form == 0) {
        if (!uniform) return -2;
        init.pos = states208[200], init.pos_begin = states208[201], init.cur_flags = states208[202];
        img = rp_script_build(n, m, k, init.pos, init.pos_begin, init.cur_flags, true);
    }
    const uint32_t W = 8;
    fb_params prm;
    prm.W = W, prm.nwin = fb_nwin(W), prm.half = 1u << (W - 1), prm.n_gens = 0;
    const size_t nf = rlcts_field_words(n, m, nbatch);
    std::vector<uint32_t> fields(nf + 8, 0xababababu), status(nbatch + 1, 0), uniq((size_t)nbatch * sh.U * 8 + 8, 0xcdcdcdcdu), lds(50 * 64, 0);
    rp_seg_tab none;
    memset(&none, 0, sizeof none);
    for (uint32_t p = 0; p < nbatch; p++) {
        kstate st;
        st.w = lds.data() + (p & 63);
        st.stride = 64;
        const rp_inputs in = rp_resolve(p, sh, proofs, commitments, rng64, none);
        if (form == 0)
            rm_front_thread<true>(p, sh, init, st, in, (const rp_script_hdr *)img.data(), fields.data(), status.data(), prm, lg_m, uniq.data(), rho64, 0u, ts_in.data(),
                                  ts_out.data());
        else
            rm_front_thread<false>(p, sh, init, st, in, nullptr, fields.data(), status.data(), prm, lg_m, uniq.data(), rho64, BP_TS_DOMSEP, ts_in.data(), ts_out.data());
    }
    for (uint32_t p = 0; p < nbatch; p++) {
        status_out[p] = (uint8_t)status[p];
        uint8_t *o = ts_out208 + (size_t)p * 208;
        memset(o, 0, 208);
        memcpy(o, &ts_out[(size_t)p * BP_TS_WORDS], 200);
        const uint32_t meta = ts_out[(size_t)p * BP_TS_WORDS + 50];
        o[200] = meta & 0xff, o[201] = (meta >> 8) & 0xff, o[202] = (meta >> 16) & 0xff;
    }
    memcpy(fields_out, fields.data(), nf * 4);
    memcpy(uniq_out, uniq.data(), (size_t)nbatch * sh.U * 32);
    return 0;
}
