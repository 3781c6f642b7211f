// Host harness for the transcript-batch interpreter (csrc/ts_batch.h): the lane body of k_ts_batch compiled with g++ and driven the
// way the kernel drives it -- a wavefront of W lanes whose sponge words sit strided in one block, every lane run forward to its own
// next rate boundary (tsb_advance), the lanes that stopped permuted together (tsb_permute), until no lane has stopped.
// TEST-ONLY: never part of libbpgpu.so, never a fallback.
//
// As a shared object (tests/test_ts_batch_on_cpu.py) it exports tsb_run.  With -DTSB_HARNESS_MAIN it is a stand-alone program for
// -fsanitize=address,undefined: every buffer is allocated at its exact size (a per-row `lens` case among them: a row's message buffer
// ends at its own length) and the results are compared with keccak.h's plain one-transcript functions.
#define BP_FE_CHECK 1
#include "../../bulletproofs_amd/csrc/ts_batch.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace bp;

// rows [0, nrows) in wavefronts of W lanes (1 .. 64); ts_in_stride in words (0: one start state); returns the number of permutation
// rounds the wavefronts took in all (what the kernel pays), rounds_serial the number a lane-by-lane loop would have paid
extern "C" uint64_t tsb_run(uint32_t W, uint32_t nrows, const uint32_t *ts_in, uint32_t ts_in_stride, uint32_t *ts_out, const tsb_op *ops, uint32_t nops,
                            const uint8_t *labels, uint64_t *rounds_serial) {
    if (W == 0 || W > 64) return ~0ull;
    std::vector<uint32_t> lds((size_t)TSB_LDS_WORDS * W);
    uint64_t rounds = 0, serial = 0;
    for (uint32_t r0 = 0; r0 < nrows; r0 += W) {
        const uint32_t nl = nrows - r0 < W ? nrows - r0 : W;
        tsb_lane L[64];
        kstate st[64], sq[64];
        for (uint32_t l = 0; l < nl; l++) {
            st[l].w = lds.data() + l;
            st[l].stride = W;
            sq[l].w = lds.data() + (size_t)50 * W + l;
            sq[l].stride = W;
            tsb_load(L[l], st[l], ts_in + (uint64_t)(r0 + l) * ts_in_stride);
        }
        for (uint32_t o = 0; o < nops; o++) {
            for (uint32_t l = 0; l < nl; l++) tsb_begin(L[l], sq[l], ops[o], r0 + l);
            for (;;) {
                bool stopped[64], any = false;
                for (uint32_t l = 0; l < nl; l++) {
                    stopped[l] = tsb_advance(L[l], st[l], sq[l], ops[o], labels, r0 + l);
                    any = any || stopped[l];
                }
                if (!any) break;
                rounds++;
                for (uint32_t l = 0; l < nl; l++)
                    if (stopped[l]) {
                        tsb_permute(L[l], st[l]);
                        serial++;
                    }
            }
            for (uint32_t l = 0; l < nl; l++) tsb_end(sq[l], ops[o], r0 + l);
        }
        for (uint32_t l = 0; l < nl; l++) tsb_store(L[l], st[l], ts_out + (uint64_t)(r0 + l) * BP_TS_WORDS);
    }
    if (rounds_serial) *rounds_serial = serial;
    return rounds;
}

#ifdef TSB_HARNESS_MAIN
namespace {
struct lone {   // one transcript through keccak.h's own functions
    uint32_t w[50];
    strobe t;
    explicit lone(const char *label) {
        kstate st;
        st.w = w;
        st.stride = 1;
        merlin_strobe_init(t, st);
        const uint8_t dsep[7] = {'d', 'o', 'm', '-', 's', 'e', 'p'};
        merlin_append_message(t, dsep, 7, (const uint8_t *)label, (uint32_t)strlen(label));
    }
    void state(uint32_t out[BP_TS_WORDS]) const {
        memcpy(out, w, 200);
        out[50] = rp_ts_meta(t.pos, t.pos_begin, t.cur_flags);
        out[51] = 0;
    }
};
int failures = 0;
void check(bool ok, const char *what) {
    if (!ok) {
        failures++;
        fprintf(stderr, "FAIL: %s\n", what);
    }
}
uint8_t *exact(size_t n) { return (uint8_t *)malloc(n); }
}  // namespace

int main() {
    const uint32_t nrows = 70, W = 64;
    // start states at 70 differing positions: row r has absorbed r + 90 bytes of a session id
    std::vector<lone> ref;
    ref.reserve(nrows);   // (a lone's strobe points into itself)
    uint32_t *ts_in = (uint32_t *)malloc((size_t)nrows * BP_TS_WORDS * 4), *ts_out = (uint32_t *)malloc((size_t)nrows * BP_TS_WORDS * 4);
    for (uint32_t r = 0; r < nrows; r++) {
        ref.emplace_back("payment-protocol v3");
        std::vector<uint8_t> sid(r + 90);
        for (size_t i = 0; i < sid.size(); i++) sid[i] = (uint8_t)(i * 7 + r);
        merlin_append_message(ref[r].t, (const uint8_t *)"session", 7, sid.data(), (uint32_t)sid.size());
        ref[r].state(ts_in + (size_t)r * BP_TS_WORDS);
    }
    // the script: a per-row append with lens (0 and len in neighbouring rows, lengths that wrap zero, one and two times), a shared
    // append, a u64, a challenge of 167 bytes, a challenge scalar, an append of nothing
    const uint32_t LEN = 400, CH = 167;
    uint32_t *lens = (uint32_t *)malloc(nrows * 4);
    for (uint32_t r = 0; r < nrows; r++) lens[r] = r % 4 == 0 ? 0 : r % 4 == 1 ? LEN : r % 4 == 2 ? 1 + r : 170 + r;
    // the rows' messages at the stride LEN; the allocation ends where the LAST row's own length ends, not at its LEN
    size_t packed = (size_t)(nrows - 1) * LEN + lens[nrows - 1];
    uint8_t *msgs = exact(packed);
    for (size_t i = 0; i < packed; i++) msgs[i] = (uint8_t)(i * 13 + 5);
    uint8_t *shared = exact(40);
    for (int i = 0; i < 40; i++) shared[i] = (uint8_t)(200 - i);
    uint64_t *xs = (uint64_t *)malloc(nrows * 8);
    for (uint32_t r = 0; r < nrows; r++) xs[r] = 0x0123456789abcdefull * (r + 1);
    uint8_t *chal = exact((size_t)nrows * CH), *scal = exact((size_t)nrows * 32), *nothing = nullptr;
    const char *lbl[6] = {"context", "shared", "n", "binding", "x", ""};
    uint32_t off[6], total = 0;
    for (int i = 0; i < 6; i++) {
        off[i] = total;
        total += (uint32_t)strlen(lbl[i]);
    }
    uint8_t *labels = exact(total);
    for (int i = 0; i < 6; i++) memcpy(labels + off[i], lbl[i], strlen(lbl[i]));
    tsb_op ops[6] = {
        {TSB_APPEND, off[0], 7, LEN, LEN, msgs, lens},
        {TSB_APPEND, off[1], 6, 40, 0, shared, nullptr},
        {TSB_APPEND, off[2], 1, 8, 8, (uint8_t *)xs, nullptr},
        {TSB_CHALLENGE, off[3], 7, CH, CH, chal, nullptr},
        {TSB_CHALLENGE_SCALAR, off[4], 1, 64, 32, scal, nullptr},
        {TSB_APPEND, off[5], 0, 0, 0, nothing, nullptr},
    };
    uint64_t serial = 0;
    const uint64_t rounds = tsb_run(W, nrows, ts_in, BP_TS_WORDS, ts_out, ops, 6, labels, &serial);
    check(rounds < serial, "the wavefront permutes its stopped lanes together");
    for (uint32_t r = 0; r < nrows; r++) {
        strobe &t = ref[r].t;
        merlin_append_message(t, (const uint8_t *)"context", 7, msgs + (size_t)r * LEN, lens[r]);
        merlin_append_message(t, (const uint8_t *)"shared", 6, shared, 40);
        merlin_append_u64(t, (const uint8_t *)"n", 1, xs[r]);
        uint8_t c[CH];
        merlin_challenge_bytes(t, (const uint8_t *)"binding", 7, c, CH);
        check(memcmp(c, chal + (size_t)r * CH, CH) == 0, "challenge bytes");
        sc x;
        rp_challenge_scalar(t, (const uint8_t *)"x", 1, x);
        check(memcmp(x.v, scal + (size_t)r * 32, 32) == 0, "challenge scalar");
        merlin_append_message(t, (const uint8_t *)"", 0, nullptr, 0);
        uint32_t want[BP_TS_WORDS];
        ref[r].state(want);
        check(memcmp(want, ts_out + (size_t)r * BP_TS_WORDS, BP_TS_WORDS * 4) == 0, "state");
    }
    // one shared start state (stride 0), out in place of nothing else; W = 7: a last wavefront of fewer lanes
    const uint64_t rounds2 = tsb_run(7, nrows, ts_in + 3 * BP_TS_WORDS, 0, ts_out, ops + 1, 2, labels, nullptr);
    check(rounds2 != ~0ull, "shared start state");
    for (uint32_t r = 0; r < nrows; r++) {
        lone a("payment-protocol v3");
        memcpy(a.w, ts_in + 3 * BP_TS_WORDS, 200);
        a.t = ref[3].t;
        a.t.st.w = a.w;
        const uint32_t meta = ts_in[3 * BP_TS_WORDS + 50];
        a.t.pos = meta & 0xff, a.t.pos_begin = (meta >> 8) & 0xff, a.t.cur_flags = (meta >> 16) & 0xff;
        merlin_append_message(a.t, (const uint8_t *)"shared", 6, shared, 40);
        merlin_append_u64(a.t, (const uint8_t *)"n", 1, xs[r]);
        uint32_t want[BP_TS_WORDS];
        a.state(want);
        check(memcmp(want, ts_out + (size_t)r * BP_TS_WORDS, BP_TS_WORDS * 4) == 0, "state from a shared start");
    }
    free(ts_in), free(ts_out), free(lens), free(msgs), free(shared), free(xs), free(chal), free(scal), free(labels);
    if (failures) return 1;
    printf("ts_batch harness ok: %u rows, %llu permutation rounds instead of %llu\n", nrows, (unsigned long long)rounds, (unsigned long long)serial);
    return 0;
}
#endif
