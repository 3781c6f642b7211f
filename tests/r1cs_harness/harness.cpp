// Host harness for the R1CS verifier: r1cs.h's per-lane bodies (r1cs_front_thread, r1cs_flatten_thread, r1_finish_lead) compiled with g++
// and driven the way the three launches of r1cs_front_dev_locked (bpgpu.hip) drive them: every proof through the front lane, every
// (column, proof) lane of the flatten launch, the dterm rows summed as k_r1cs_finish sums them (64 strided shares, then a tree), then
// the lead lane.  The circuit image and the launch shape come from r1cs.h's own r1cs_build_lists / r1cs_shape_of, the functions
// libbpgpu.so uses.  Every buffer has its logical size (never more than the library reserves for it) in a heap allocation of its own,
// so that an access past one is an error under -fsanitize=address and not a read of a neighbour.
// The prover's witness lane (r1p_witness_thread / r1p_eval_row of r1cs_prover.h, whose cooperative-STROBE section is device-only) runs
// from a second kind of case file: phase 1 before the challenge fields exist, phase 2 with them filled from the given values.
// Built twice by tests/test_r1cs_generated.py: a shared library (r1h_run_file), and with -DR1H_MAIN and the sanitizers a standalone
// executable `harness case.bin out.bin` run as a child process.  TEST-ONLY: never part of libbpgpu.so, never a fallback.
//
// case file (little-endian u32 words, byte arrays padded to 4): "R1H1", m, n1, n2, two_phase, nch, Q, n_terms, nbatch, proof_stride,
// per_proof_ts, gens_capacity, label bytes; label_lens[nch], labels, row_ptr[Q + 1], kind[n_terms] (bytes), index, challenge, power
// [n_terms each], coeff[n_terms x 32 bytes], proof_lens[nbatch], proofs[nbatch x proof_stride], commitments[nbatch x m x 32],
// transcripts[(per_proof_ts ? nbatch : 1) x 208], rng32[nbatch x 32]
// witness case file: "R1W1", m, n1, n2, nch, Q, n_free, n_rows, n_terms, nbatch; src_left[n], src_right[n], row_ptr[n_rows + 1], kind, index,
// challenge, power, coeff as above; v[nbatch x m x 32], free inputs[nbatch x n_free x 32], challenge values[nbatch x nch x 32]
// -> a_L, a_R, a_O [nbatch x 3 x n x 32]
// output file: pn, k, U, one_chunks; status[nbatch], ts_out[nbatch x 52], gen_sc[nbatch x (2 pn + 2) x 8], uniq_sc, uniq_pt[nbatch x U x 8]
#define BP_FE_CHECK 1
#include "../../bulletproofs_amd/csrc/r1cs_prover.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
using namespace bp;

namespace {

struct reader {
    const std::vector<uint8_t> &b;
    size_t off = 0;
    bool bad = false;
    const uint8_t *take(size_t n) {
        const size_t padded = (n + 3) & ~(size_t)3;
        if (off + padded > b.size()) {
            bad = true;
            return nullptr;
        }
        const uint8_t *p = b.data() + off;
        off += padded;
        return p;
    }
    uint32_t u32() {
        const uint8_t *p = take(4);
        uint32_t v = 0;
        if (p) memcpy(&v, p, 4);
        return v;
    }
};

// an allocation of exactly n elements, filled from src (or with `fill` bytes)
template <typename T>
std::unique_ptr<T[]> exact(size_t n, const void *src, int fill = 0) {
    std::unique_ptr<T[]> p(new T[n]);
    if (n && src) memcpy((void *)p.get(), src, n * sizeof(T));
    else if (n) memset((void *)p.get(), fill, n * sizeof(T));
    return p;
}

void put(std::vector<uint8_t> &out, const void *p, size_t n) {
    const uint8_t *s = (const uint8_t *)p;
    out.insert(out.end(), s, s + n);
}

// rows [r0, r1) of dterm for proof p, as r1_block_sum (k_r1cs.hip): lane l takes rows r0 + l, r0 + l + 64, ..; then the tree over 64 partial sums
void block_sum(sc &out, const r1cs_shape &sh, const uint32_t *dterm, uint32_t r0, uint32_t r1, uint32_t p) {
    sc part[64], t;
    for (uint32_t l = 0; l < 64; l++) {
        sc_0(part[l]);
        for (uint32_t i = r0 + l; i < r1; i += 64) {
            const uint32_t *src = dterm + ((uint64_t)i * sh.nproofs + p) * 8;
            for (int q = 0; q < 8; q++) t.v[q] = src[q];
            sc_add(part[l], part[l], t);
        }
    }
    for (uint32_t h = 32; h > 0; h >>= 1)
        for (uint32_t l = 0; l < h; l++) sc_add(part[l], part[l], part[l + h]);
    out = part[0];
}

// a_L, a_R, a_O of every proof from the witness program, as bpgpu_r1cs_prove_batch runs k_r1p_witness: multipliers [0, n1), then [n1, n)
int run_witness(reader &r, std::vector<uint8_t> &out) {
    const uint32_t m = r.u32(), n1 = r.u32(), n2 = r.u32(), nch = r.u32(), Q = r.u32(), nfree = r.u32(), nrows = r.u32(), n_terms = r.u32(), nbatch = r.u32();
    if (r.bad || nbatch == 0) return -1;
    const uint32_t n = n1 + n2;
    const uint8_t *srcl = r.take(4 * (size_t)n), *srcr = r.take(4 * (size_t)n), *row_ptr = r.take(4 * ((size_t)nrows + 1)), *kind = r.take(n_terms),
                  *index = r.take(4 * (size_t)n_terms), *chal = r.take(4 * (size_t)n_terms), *power = r.take(4 * (size_t)n_terms),
                  *coeff = r.take(32 * (size_t)n_terms), *v = r.take((size_t)nbatch * m * 32), *freev = r.take((size_t)nbatch * nfree * 32),
                  *chv = r.take((size_t)nbatch * nch * 32);
    if (r.bad || r.off != r.b.size()) return -1;
    auto terms = exact<r1p_term>(n_terms, nullptr);
    for (uint32_t t = 0; t < n_terms; t++) {   // as bpgpu_r1cs_witness_create fills them (no sign flip: Prover::eval sums plainly)
        r1p_term &e = terms[t];
        uint32_t ch, pw;
        memcpy(&e.index, index + 4 * (size_t)t, 4);
        memcpy(&ch, chal + 4 * (size_t)t, 4);
        memcpy(&pw, power + 4 * (size_t)t, 4);
        e.kind = kind[t];
        e.chal = ch == R1_NO_CHAL ? R1_NO_CHAL : (ch | (pw << 16));
        sc cf;
        sc28 cm;
        memcpy(cf.v, coeff + (size_t)t * 32, 32);
        sc_to_mont28(cm, cf);
        memcpy(e.coeff, cm.v, 40);
    }
    uint32_t pn = 1, k = 0;
    while (pn < n) pn <<= 1, k++;
    r1p_shape sh{};                          // the field layout of bpgpu_r1cs_prove_batch
    sh.c.m = m, sh.c.n1 = n1, sh.c.n = n, sh.c.pn = pn, sh.c.k = k, sh.c.two_phase = (n2 || nch) ? 1u : 0u, sh.c.nch = nch, sh.c.Q = Q;
    sh.c.nzhi = (Q >> 6) + 1;
    sh.c.nyhi = ((pn - 1) >> 6) + 1;
    sh.c.f_zlo = R1P_FIXED;
    sh.c.f_zhi = sh.c.f_zlo + 64;
    sh.c.f_ylo = sh.c.f_zhi + sh.c.nzhi;
    sh.c.f_yhi = sh.c.f_ylo + 64;
    sh.f_yplo = sh.c.f_yhi + sh.c.nyhi;
    sh.f_yphi = sh.f_yplo + 64;
    sh.c.f_ch = sh.f_yphi + sh.c.nyhi;
    sh.c.nfields = sh.c.f_ch + sh.c.nch;
    sh.c.nproofs = nbatch;
    sh.nfree = nfree;
    auto src_l = exact<uint32_t>(n, srcl), src_r = exact<uint32_t>(n, srcr), rows = exact<uint32_t>((size_t)nrows + 1, row_ptr);
    auto d_v = exact<uint8_t>((size_t)nbatch * m * 32, v), d_free = exact<uint8_t>((size_t)nbatch * nfree * 32, freev);
    auto fields = exact<uint32_t>((size_t)sh.c.nfields * nbatch * 10, nullptr, 0xa5);
    auto aw = exact<uint32_t>(3 * (size_t)n * nbatch * 10, nullptr, 0xa5);
    for (uint32_t ph = 0; ph < 2; ph++) {
        sh.i0 = ph ? n1 : 0, sh.i1 = ph ? n : n1;
        if (ph)                               // k_r1p_chal1 has stored the phase-2 challenges by now
            for (uint32_t p = 0; p < nbatch; p++)
                for (uint32_t j = 0; j < nch; j++) {
                    sc c;
                    sc28 cm;
                    memcpy(c.v, chv + ((size_t)p * nch + j) * 32, 32);
                    sc_to_mont28(cm, c);
                    r1_store28(fields.get(), sh.c, sh.c.f_ch + j, p, cm);
                }
        for (uint32_t p = 0; p < nbatch; p++)
            r1p_witness_thread(p, sh, src_l.get(), src_r.get(), rows.get(), terms.get(), d_v.get(), d_free.get(), fields.get(), aw.get());
    }
    for (uint32_t p = 0; p < nbatch; p++)
        for (uint32_t f = 0; f < 3 * n; f++) {
            sc s;
            uint32_t w[8];
            r1p_ld(s, aw.get(), nbatch, f, p);
            store_words8(w, s);
            put(out, w, 32);
        }
    return 0;
}

int run(const std::vector<uint8_t> &in, std::vector<uint8_t> &out) {
    reader r{in};
    const uint32_t magic = r.u32();
    if (magic == 0x31573152u) return run_witness(r, out);   // "R1W1"
    if (magic != 0x31483152u) return -1;                    // "R1H1"
    const uint32_t m = r.u32(), n1 = r.u32(), n2 = r.u32(), two_phase = r.u32(), nch = r.u32(), Q = r.u32(), n_terms = r.u32(), nbatch = r.u32(),
                   proof_stride = r.u32(), per_proof_ts = r.u32(), gens_capacity = r.u32(), lbl_bytes = r.u32();
    if (r.bad || nbatch == 0) return -1;
    const uint32_t n = n1 + n2;
    const uint8_t *label_lens = r.take(4 * (size_t)nch), *labels = r.take(lbl_bytes), *row_ptr = r.take(4 * ((size_t)Q + 1)), *kind = r.take(n_terms),
                  *index = r.take(4 * (size_t)n_terms), *chal = r.take(4 * (size_t)n_terms), *power = r.take(4 * (size_t)n_terms),
                  *coeff = r.take(32 * (size_t)n_terms), *lens = r.take(4 * (size_t)nbatch), *proofs = r.take((size_t)nbatch * proof_stride),
                  *coms = r.take((size_t)nbatch * m * 32), *ts = r.take((per_proof_ts ? nbatch : 1) * (size_t)208), *rng = r.take((size_t)nbatch * 32);
    if (r.bad || r.off != in.size()) return -1;
    // the circuit image: [col_ptr][ents][lbl_off][lbl], each on its own
    std::vector<uint32_t> col_v;
    std::vector<r1cs_ent> ent_v;
    {
        auto rp = exact<uint32_t>((size_t)Q + 1, row_ptr), ix = exact<uint32_t>(n_terms, index), ch = exact<uint32_t>(n_terms, chal), pw = exact<uint32_t>(n_terms, power);
        r1cs_build_lists(m, n, Q, rp.get(), n_terms, kind, ix.get(), ch.get(), pw.get(), coeff, col_v, ent_v);
    }
    if (col_v.size() != 3 * (size_t)n + m + 2 || ent_v.size() != n_terms) return -2;
    auto col_ptr = exact<uint32_t>(col_v.size(), col_v.data());
    auto ents = exact<r1cs_ent>(ent_v.size(), ent_v.data());
    auto lbl_off = exact<uint32_t>((size_t)nch + 1, nullptr);
    for (uint32_t j = 0; j < nch; j++) {
        uint32_t len;
        memcpy(&len, label_lens + 4 * j, 4);
        lbl_off[j + 1] = lbl_off[j] + len;
    }
    if (lbl_off[nch] != lbl_bytes) return -1;
    auto lbl = exact<uint8_t>((size_t)lbl_bytes + 1, nullptr);   // (the image keeps one byte behind the labels)
    if (lbl_bytes) memcpy(lbl.get(), labels, lbl_bytes);
    uint32_t pn = 1, k = 0;
    while (pn < n) pn <<= 1, k++;            // next_power_of_two (0 -> 1), as bpgpu_r1cs_circuit_create
    r1cs_shape sh{};
    r1cs_shape_of(sh, m, n1, n, pn, k, two_phase, nch, Q, col_ptr[3 * n + m + 1] - col_ptr[3 * n + m], proof_stride, nbatch, gens_capacity);
    // the inputs and the working set of r1cs_front_dev_locked: generator rows, per-proof rows and status zeroed, fields and dterm not
    auto d_proofs = exact<uint8_t>((size_t)nbatch * proof_stride, proofs);
    auto d_lens = exact<uint32_t>(nbatch, lens);
    auto d_coms = exact<uint8_t>((size_t)nbatch * m * 32, coms);
    auto d_ts = exact<uint32_t>(per_proof_ts ? (size_t)nbatch * BP_TS_WORDS : 0, per_proof_ts ? ts : nullptr);
    auto d_rng = exact<uint8_t>((size_t)nbatch * 32, rng);
    const size_t ngen = 2 * (size_t)pn + 2, nd = ((size_t)pn + sh.one_chunks) * nbatch * 8;
    auto fields = exact<uint32_t>((size_t)sh.nfields * nbatch * 10, nullptr, 0xa5);
    auto gen = exact<uint32_t>(nbatch * ngen * 8, nullptr);
    auto usc = exact<uint32_t>((size_t)nbatch * sh.U * 8, nullptr), upt = exact<uint32_t>((size_t)nbatch * sh.U * 8, nullptr);
    auto status = exact<uint32_t>(nbatch, nullptr);
    auto dterm = exact<uint32_t>(nd, nullptr, 0xa5);
    auto ts_out = exact<uint32_t>((size_t)nbatch * BP_TS_WORDS, nullptr);
    rp_strobe_init init;
    memset(&init, 0, sizeof init);
    if (!per_proof_ts) {                     // strobe_init_from_state (bpgpu.hip)
        memcpy(init.w, ts, 200);
        init.pos = ts[200], init.pos_begin = ts[201], init.cur_flags = ts[202];
    }
    // launch 1: lane = proof
    for (uint32_t p = 0; p < nbatch; p++) {
        uint32_t sponge[50];
        kstate st;
        st.w = sponge;
        st.stride = 1;
        r1cs_front_thread(p, sh, init, st, d_proofs.get(), d_lens.get(), d_coms.get(), per_proof_ts ? d_ts.get() : nullptr, d_rng.get(), lbl_off.get(),
                          lbl.get(), fields.get(), usc.get(), upt.get(), ts_out.get(), status.get());
    }
    if (!sh.gens_short) {
        // launch 2: lane = (column, proof), proof fastest
        const uint32_t nt = (uint32_t)(((uint64_t)pn + m + sh.one_chunks) * nbatch);
        for (uint32_t tid = 0; tid < nt; tid++)
            r1cs_flatten_thread(tid, sh, col_ptr.get(), ents.get(), status.get(), fields.get(), gen.get(), usc.get(), dterm.get());
        // launch 3: one workgroup per proof
        for (uint32_t p = 0; p < nbatch; p++) {
            if (status[p] != 0) continue;
            sc delta, wc;
            block_sum(delta, sh, dterm.get(), 0, pn, p);
            block_sum(wc, sh, dterm.get(), pn, pn + sh.one_chunks, p);
            r1_finish_lead(p, sh, delta, wc, fields.get(), gen.get());
        }
    }
    const uint32_t hdr[4] = {pn, k, sh.U, sh.one_chunks};
    put(out, hdr, sizeof hdr);
    put(out, status.get(), (size_t)nbatch * 4);
    put(out, ts_out.get(), (size_t)nbatch * BP_TS_WORDS * 4);
    put(out, gen.get(), nbatch * ngen * 32);
    put(out, usc.get(), (size_t)nbatch * sh.U * 32);
    put(out, upt.get(), (size_t)nbatch * sh.U * 32);
    return 0;
}

int run_file(const char *in_path, const char *out_path) {
    FILE *f = fopen(in_path, "rb");
    if (!f) return -3;
    std::vector<uint8_t> in, out;
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + got);
    fclose(f);
    const int rc = run(in, out);
    if (rc) return rc;
    f = fopen(out_path, "wb");
    if (!f) return -3;
    const bool ok = out.empty() || fwrite(out.data(), 1, out.size(), f) == out.size();
    return fclose(f) == 0 && ok ? 0 : -3;
}

}  // namespace

extern "C" int r1h_run_file(const char *in_path, const char *out_path) { return run_file(in_path, out_path); }

#ifdef R1H_MAIN
int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s case.bin out.bin\n", argv[0]);
        return 2;
    }
    const int rc = run_file(argv[1], argv[2]);
    if (rc) fprintf(stderr, "r1cs harness: error %d\n", rc);
    return rc ? 1 : 0;
}
#endif
