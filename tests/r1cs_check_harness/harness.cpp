// Host harness for the R1CS witness check: r1cs_check.h's per-lane bodies (r1c_chal_thread, r1c_unit_thread, r1c_long_thread) and the
// prover's input and witness lanes (r1cs_prover.h) compiled with g++ and driven lane by lane the way bpgpu_r1cs_witness_check
// (bpgpu.hip) launches them; atomics are plain operations here.  The per-variable lists, the row form, the units and the slice come
// from the functions libbpgpu.so uses (r1cs_build_lists, r1c_build_rows, r1c_slice).  Every buffer has its logical size in a heap
// allocation of its own, so that an access past one is an error under -fsanitize=address and not a read of a neighbour.
// Built twice by tests/test_r1cs_check.py: a shared library (r1ch_run_file, r1ch_chunk), and with -DR1CH_MAIN and the sanitizers a
// stand-alone executable `harness case.bin out.bin` (`harness --chunk` prints R1C_CHUNK).  TEST-ONLY: never part of libbpgpu.so.
//
// case file (little-endian u32 words, byte arrays padded to 4): "R1C1", m, n1, n2, nch, Q, n_cterms, n_free, n_rows, n_wterms, nbatch,
// want_map; the constraints: row_ptr[Q + 1], kind[n_cterms] (bytes), index, challenge, power [n_cterms each], coeff[n_cterms x 32];
// the witness program: src_left[n], src_right[n], row_ptr[n_rows + 1], kind, index, challenge, power, coeff likewise;
// v[nbatch x m x 32], free inputs[nbatch x n_free x 32], challenge values[nbatch x nch x 32]
// output file: R1C_CHUNK, mapw, units, long rows, slots, slice; status[nbatch], first[nbatch], count[nbatch], map[nbatch x mapw]
#define BP_FE_CHECK 1
#include "../../bulletproofs_amd/csrc/r1cs_check.h"
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

struct term_arrays {
    const uint8_t *kind, *index, *chal, *power, *coeff;
    void take(reader &r, size_t nt) {
        kind = r.take(nt), index = r.take(4 * nt), chal = r.take(4 * nt), power = r.take(4 * nt), coeff = r.take(32 * nt);
    }
};

int run(const std::vector<uint8_t> &in, std::vector<uint8_t> &out) {
    reader r{in};
    if (r.u32() != 0x31433152u) return -1;   // "R1C1"
    const uint32_t m = r.u32(), n1 = r.u32(), n2 = r.u32(), nch = r.u32(), Q = r.u32(), n_cterms = r.u32(), nfree = r.u32(), nrows = r.u32(),
                   n_wterms = r.u32(), nbatch = r.u32(), want_map = r.u32();
    if (r.bad || nbatch == 0) return -1;
    const uint32_t n = n1 + n2;
    const uint8_t *crow = r.take(4 * ((size_t)Q + 1));
    term_arrays ct, wt;
    ct.take(r, n_cterms);
    const uint8_t *srcl = r.take(4 * (size_t)n), *srcr = r.take(4 * (size_t)n), *wrow = r.take(4 * ((size_t)nrows + 1));
    wt.take(r, n_wterms);
    const uint8_t *v = r.take((size_t)nbatch * m * 32), *freev = r.take((size_t)nbatch * nfree * 32), *chv = r.take((size_t)nbatch * nch * 32);
    if (r.bad || r.off != in.size()) return -1;
    // the circuit as bpgpu_r1cs_circuit_create keeps it, then its row form as the first check builds it
    std::vector<uint32_t> col_v;
    std::vector<r1cs_ent> ent_v;
    {
        auto rp = exact<uint32_t>((size_t)Q + 1, crow), ix = exact<uint32_t>(n_cterms, ct.index), ch = exact<uint32_t>(n_cterms, ct.chal),
             pw = exact<uint32_t>(n_cterms, ct.power);
        r1cs_build_lists(m, n, Q, rp.get(), n_cterms, ct.kind, ix.get(), ch.get(), pw.get(), ct.coeff, col_v, ent_v);
    }
    r1c_rows rows;
    r1c_build_rows(m, n, Q, col_v, ent_v, rows);
    if (rows.terms.size() != n_cterms) return -2;
    auto units = exact<r1c_unit>(rows.units.size(), rows.units.data());
    auto rterms = exact<r1p_term>(rows.terms.size(), rows.terms.data());
    auto longs = exact<r1c_long>(rows.longs.size(), rows.longs.data());
    // the witness program as bpgpu_r1cs_witness_create keeps it
    auto wterms = exact<r1p_term>(n_wterms, nullptr);
    for (uint32_t t = 0; t < n_wterms; t++) {
        r1p_term &e = wterms[t];
        uint32_t ch, pw;
        memcpy(&e.index, wt.index + 4 * (size_t)t, 4);
        memcpy(&ch, wt.chal + 4 * (size_t)t, 4);
        memcpy(&pw, wt.power + 4 * (size_t)t, 4);
        e.kind = wt.kind[t];
        e.chal = ch == R1_NO_CHAL ? R1_NO_CHAL : (ch | (pw << 16));
        sc cf;
        sc28 cm;
        memcpy(cf.v, wt.coeff + (size_t)t * 32, 32);
        sc_to_mont28(cm, cf);
        memcpy(e.coeff, cm.v, 40);
    }
    auto src_l = exact<uint32_t>(n, srcl), src_r = exact<uint32_t>(n, srcr), wrows = exact<uint32_t>((size_t)nrows + 1, wrow);
    uint32_t pn = 1, k = 0;
    while (pn < n) pn <<= 1, k++;
    r1p_shape sh{};                          // the field layout of bpgpu_r1cs_witness_check: the challenges only
    sh.c.m = m, sh.c.n1 = n1, sh.c.n = n, sh.c.pn = pn, sh.c.k = k, sh.c.two_phase = (n2 || nch) ? 1u : 0u, sh.c.nch = nch, sh.c.Q = Q;
    sh.c.f_ch = 0;
    sh.c.nfields = nch;
    sh.c.nproofs = nbatch;
    sh.nfree = nfree;
    sh.i0 = 0, sh.i1 = n;
    const uint32_t mapw = want_map ? (Q + 31) / 32 : 0;
    const size_t per = r1c_slice(rows, nbatch);
    auto d_v = exact<uint8_t>((size_t)nbatch * m * 32, v), d_free = exact<uint8_t>((size_t)nbatch * nfree * 32, freev),
         d_ch = exact<uint8_t>((size_t)nbatch * nch * 32, chv);
    auto fields = exact<uint32_t>((size_t)nch * nbatch * 10, nullptr, 0xa5);
    auto aw = exact<uint32_t>(3 * (size_t)n * nbatch * 10, nullptr, 0xa5);
    auto part = exact<uint32_t>((size_t)rows.nslots * per * 8, nullptr, 0xa5);
    auto status = exact<uint32_t>(nbatch, nullptr), first = exact<uint32_t>(nbatch, nullptr, 0xff), count = exact<uint32_t>(nbatch, nullptr);
    auto map = exact<uint32_t>((size_t)nbatch * mapw, nullptr);
    for (uint32_t tid = 0; tid < nbatch * nch; tid++) r1c_chal_thread(tid, sh, d_ch.get(), fields.get(), status.get());
    for (uint32_t tid = 0; tid < nbatch * (m + nfree); tid++) r1p_inputs_thread(tid, sh, d_v.get(), nullptr, d_free.get(), nullptr, status.get());
    if (n)
        for (uint32_t p = 0; p < nbatch; p++)
            r1p_witness_thread(p, sh, src_l.get(), src_r.get(), wrows.get(), wterms.get(), d_v.get(), d_free.get(), fields.get(), aw.get());
    for (size_t p0 = 0; p0 < nbatch; p0 += per) {
        const uint32_t cnt = (uint32_t)std::min(per, (size_t)nbatch - p0);
        for (uint32_t tid = 0; tid < rows.units.size() * cnt; tid++)
            r1c_unit_thread(tid, sh, (uint32_t)p0, cnt, units.get(), rterms.get(), aw.get(), d_v.get(), fields.get(), status.get(), mapw, part.get(), first.get(),
                            count.get(), want_map ? map.get() : nullptr);
        for (uint32_t tid = 0; tid < rows.longs.size() * cnt; tid++)
            r1c_long_thread(tid, (uint32_t)p0, cnt, longs.get(), part.get(), status.get(), mapw, first.get(), count.get(), want_map ? map.get() : nullptr);
    }
    const uint32_t hdr[6] = {R1C_CHUNK, mapw, (uint32_t)rows.units.size(), (uint32_t)rows.longs.size(), rows.nslots, (uint32_t)per};
    put(out, hdr, sizeof hdr);
    put(out, status.get(), (size_t)nbatch * 4);
    put(out, first.get(), (size_t)nbatch * 4);
    put(out, count.get(), (size_t)nbatch * 4);
    put(out, map.get(), (size_t)nbatch * mapw * 4);
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

extern "C" int r1ch_run_file(const char *in_path, const char *out_path) { return run_file(in_path, out_path); }
extern "C" int r1ch_chunk(void) { return R1C_CHUNK; }

#ifdef R1CH_MAIN
int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "--chunk")) {
        printf("CHUNK %d\n", R1C_CHUNK);
        return 0;
    }
    if (argc != 3) {
        fprintf(stderr, "usage: %s case.bin out.bin | --chunk\n", argv[0]);
        return 2;
    }
    const int rc = run_file(argv[1], argv[2]);
    if (rc) fprintf(stderr, "r1cs check harness: error %d\n", rc);
    return rc ? 1 : 0;
}
#endif
