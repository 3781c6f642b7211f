// Batches of Merlin transcripts: one SCRIPT of transcript operations applied to many transcripts (rows), lane = row.
//
// The public form of what every front-end kernel does with keccak.h's primitives (bpgpu_transcript_batch, include/bpgpu.h): the
// callers' start states -- one, or one per row, at any STROBE position -- take a list of append_message / challenge_bytes operations
// whose labels are shared and whose messages are per row, of per-row lengths.
//
// The op list is uniform across the wavefront, so the op loop does not diverge.  The ROWS differ: they start at differing positions
// and append differing lengths, so they reach the 166-byte rate boundary at differing bytes.  A lane that ran strobe_absorb1 byte by
// byte would meet the permutation inside a divergent loop, and a wavefront whose 64 rows wrap at 64 different bytes would run
// Keccak-f[1600] 64 times, one lane each.  Here an operation is a small per-lane state machine (tsb_advance) over its five segments
//     framing (meta-AD)  |  label  |  4 length bytes  |  framing (AD or PRF)  |  body (message bytes in, or challenge bytes out)
// that runs forward to the lane's OWN next boundary, applies run_f's three XORs there and stops; the wavefront then permutes every
// lane that stopped TOGETHER, at the one call site of the permutation (tsb_permute), and goes round again until no lane has stopped.
// An operation costs max over the rows of their wrap counts, not the sum.  The byte-wise segment loops between two boundaries do
// diverge, by at most 166 XORs into the lane's own LDS column.
//
// Everything here compiles for the host as well: tests/ts_batch_harness drives the same lane body over a simulated wavefront.
#ifndef BPGPU_TS_BATCH_H
#define BPGPU_TS_BATCH_H
#include "rangeproof.h"

namespace bp {

#define TSB_BLOCK 64          // one wavefront per workgroup: 64 x (50 sponge + 16 challenge) words = 16.5 KiB of LDS
#define TSB_SQ_WORDS 16       // the 64 bytes of a challenge_scalar, parked per lane until the operation ends
#define TSB_LDS_WORDS (50 + TSB_SQ_WORDS)

// kinds as the device sees them (the ABI's APPEND_U64 arrives as an APPEND of 8 bytes)
#define TSB_APPEND 0u
#define TSB_CHALLENGE 1u
#define TSB_CHALLENGE_SCALAR 2u

struct tsb_op {
    uint32_t kind, label_off, label_len, len;   // label bytes at labels[label_off ..); len: message / challenge bytes (64 for a scalar)
    uint64_t stride;                            // bytes between rows of `data`; 0: one message for every row (appends only)
    uint8_t *data;                              // appends read it, challenges write it (32 bytes per row for a scalar)
    const uint32_t *lens;                       // optional: row r appends min(lens[r], len) bytes
};

struct tsb_lane {
    uint32_t pos, pos_begin, cur_flags;
    uint32_t seg, off, mlen;                    // where in the operation the lane is; its own body length
};

BP_HD void tsb_load(tsb_lane &L, const kstate &st, const uint32_t *src) {
    for (uint32_t i = 0; i < 50; i++) ks_set32(st, i, src[i]);
    const uint32_t meta = src[50];
    L.pos = meta & 0xffu;
    L.pos_begin = (meta >> 8) & 0xffu;
    L.cur_flags = (meta >> 16) & 0xffu;
    if (L.pos >= BP_STROBE_R || L.pos_begin > BP_STROBE_R) L.pos = L.pos_begin = 0;   // (the host form refuses such a state)
    L.seg = 5;
    L.off = L.mlen = 0;
}
BP_HD void tsb_store(const tsb_lane &L, const kstate &st, uint32_t *dst) {
    for (uint32_t i = 0; i < 50; i++) dst[i] = ks_get32(st, i);
    dst[50] = rp_ts_meta(L.pos, L.pos_begin, L.cur_flags);
    dst[51] = 0;
}

BP_HD void tsb_begin(tsb_lane &L, const kstate &sq, const tsb_op &op, uint64_t r) {
    L.seg = 0;
    L.off = 0;
    L.mlen = op.len;
    if (op.kind == TSB_APPEND && op.lens) {
        const uint32_t n = op.lens[r];
        L.mlen = n < op.len ? n : op.len;
    }
    if (op.kind == TSB_CHALLENGE_SCALAR)
        for (uint32_t i = 0; i < TSB_SQ_WORDS; i++) ks_set32(sq, i, 0);
}

// the lane is at a boundary (pos == R), or a PRF begins in mid-block: strobe_run_f up to the permutation itself
BP_HD bool tsb_stop(const tsb_lane &L, const kstate &st) {
    ks_xor8(st, L.pos, L.pos_begin);
    ks_xor8(st, L.pos + 1, 0x04);
    ks_xor8(st, BP_STROBE_R + 1, 0x80);
    return true;
}
// ... and the permutation, for every lane of the wavefront that stopped
BP_HD void tsb_permute(tsb_lane &L, const kstate &st) {
    keccak_f1600(st);
    L.pos = 0;
    L.pos_begin = 0;
}

// Run the lane forward through its operation.  true: it stopped in front of a permutation (tsb_permute, then call again);
// false: the operation is done.
BP_HD bool tsb_advance(tsb_lane &L, const kstate &st, const kstate &sq, const tsb_op &op, const uint8_t *labels, uint64_t r) {
    while (L.seg < 5) {
        if (L.seg == 0 || L.seg == 3) {   // strobe_begin_op: meta-AD in front of the label, AD / PRF in front of the body
            const uint32_t flags = L.seg == 0 ? (BP_FLAG_M | BP_FLAG_A) : op.kind == TSB_APPEND ? BP_FLAG_A : (BP_FLAG_I | BP_FLAG_A | BP_FLAG_C);
            if (L.off == 0) {
                const uint32_t old_begin = L.pos_begin;
                L.pos_begin = L.pos + 1;
                L.cur_flags = flags;
                ks_xor8(st, L.pos++, old_begin);
                L.off = 1;
                if (L.pos == BP_STROBE_R) return tsb_stop(L, st);
            }
            if (L.off == 1) {
                ks_xor8(st, L.pos++, flags);
                L.off = 2;
                if (L.pos == BP_STROBE_R) return tsb_stop(L, st);
            }
            L.off = 0;
            L.seg++;
            if ((flags & BP_FLAG_C) && L.pos != 0) return tsb_stop(L, st);
            continue;
        }
        const uint32_t total = L.seg == 1 ? op.label_len : L.seg == 2 ? 4u : L.mlen;
        uint32_t take = total - L.off;
        if (take > BP_STROBE_R - L.pos) take = BP_STROBE_R - L.pos;
        if (L.seg == 1) {
            const uint8_t *src = labels + op.label_off + L.off;
            for (uint32_t i = 0; i < take; i++) ks_xor8(st, L.pos + i, src[i]);
        } else if (L.seg == 2) {          // strobe_meta_len: the length a lone Transcript would announce
            const uint32_t n = op.kind == TSB_APPEND ? L.mlen : op.len;
            for (uint32_t i = 0; i < take; i++) ks_xor8(st, L.pos + i, (n >> (8 * (L.off + i))) & 0xffu);
        } else if (op.kind == TSB_APPEND) {
            const uint8_t *src = op.data + r * op.stride + L.off;
            for (uint32_t i = 0; i < take; i++) ks_xor8(st, L.pos + i, src[i]);
        } else {                          // STROBE's PRF: read, then zero what was read
            uint8_t *dst = op.data + r * op.stride + L.off;
            for (uint32_t i = 0; i < take; i++) {
                const uint32_t b = ks_get8(st, L.pos + i);
                ks_clear8(st, L.pos + i);
                if (op.kind == TSB_CHALLENGE) dst[i] = (uint8_t)b;
                else ks_xor8(sq, L.off + i, b);
            }
        }
        L.pos += take;
        L.off += take;
        if (L.off == total) {
            L.off = 0;
            L.seg++;
        }
        if (L.pos == BP_STROBE_R) return tsb_stop(L, st);
    }
    return false;
}

// the crate's challenge_scalar: the 64 parked bytes through Scalar::from_bytes_mod_order_wide, 32 canonical bytes out
BP_HD void tsb_end(const kstate &sq, const tsb_op &op, uint64_t r) {
    if (op.kind != TSB_CHALLENGE_SCALAR) return;
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = ks_get32(sq, i);
    sc s;
    sc_from_wide(s, w);
    uint8_t *dst = op.data + r * op.stride;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        dst[4 * i] = (uint8_t)s.v[i];
        dst[4 * i + 1] = (uint8_t)(s.v[i] >> 8);
        dst[4 * i + 2] = (uint8_t)(s.v[i] >> 16);
        dst[4 * i + 3] = (uint8_t)(s.v[i] >> 24);
    }
}

#if defined(__HIPCC__)
// lane = row; lds: TSB_LDS_WORDS x TSB_BLOCK words.  Lanes past the batch run along with nothing to do: the wavefront-wide vote needs them.
__device__ __forceinline__ void tsb_thread(uint32_t lane, uint64_t r, bool active, uint32_t *lds, const uint32_t *ts_in, uint32_t ts_in_stride, uint32_t *ts_out,
                                           const tsb_op *ops, uint32_t nops, const uint8_t *labels) {
    kstate st, sq;
    st.w = lds + lane;
    st.stride = TSB_BLOCK;
    sq.w = lds + 50 * TSB_BLOCK + lane;
    sq.stride = TSB_BLOCK;
    tsb_lane L;
    L.pos = L.pos_begin = L.cur_flags = L.off = L.mlen = 0;
    L.seg = 5;
    if (active) tsb_load(L, st, ts_in + r * ts_in_stride);
    for (uint32_t o = 0; o < nops; o++) {
        const tsb_op op = ops[o];
        if (active) tsb_begin(L, sq, op, r);
        for (;;) {
            const bool stopped = active && tsb_advance(L, st, sq, op, labels, r);
            if (!__any(stopped)) break;
            if (stopped) tsb_permute(L, st);
        }
        if (active) tsb_end(sq, op, r);
    }
    if (active) tsb_store(L, st, ts_out + r * BP_TS_WORDS);
}
#endif

}  // namespace bp
#endif
