// libbpgpu.so: host runtime + C ABI (include/bpgpu.h).  The kernels (gfx950) live in k_*.hip, thin __global__
// wrappers around the per-lane bodies in msm_vb.h / msm_fixed.h / rangeproof.h; the bodies are shared with the
// CPU test harness.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <sys/random.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <new>
#include <vector>

#include "../../include/bpgpu.h"
#include "kernels.h"
#include "hostrng.h"
#include "host_io.h"

using namespace bp;

// ============================================================================
// host runtime
// ============================================================================
struct kstat {
    uint64_t launches = 0;
    double ms = 0;
};

// Generator tables are read-only and depend only on (device, generator encodings, W): contexts of
// one process share them (a service runs one context per host thread / stream).
struct shared_table {
    int device;
    uint32_t W;
    std::vector<uint8_t> gens;
    fb_entry *d_table;
    int refs;
};
static std::mutex g_tab_mu;                 // the list below
static std::mutex g_tab_build_mu[64];       // one table under construction per DEVICE (two contexts of a device asking for the same table: the second
                                            // one waits and finds it); tables of different devices are built at the same time (pool over N devices)
static std::vector<shared_table *> g_tables;

static std::atomic<uint64_t> g_ctx_serial{1};
struct bpgpu_ctx {
    const uint64_t serial = g_ctx_serial.fetch_add(1);   // never reused, unlike the address: what a recorded relation remembers of its context
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    std::string err;
    // bump arena for per-call scratch
    char *arena = nullptr;
    size_t arena_cap = 0, arena_off = 0;
    // options
    uint32_t W = 0;                          // fixed-base window bits; 0 = largest that fits table_budget
    uint64_t table_budget = 160ull << 30;    // bytes of HBM the generator tables may take: 160 GiB of the MI355X's 288 GB (W = 20 / 16 / 15 for m = 1 / 16 / 32:
                                             // +3 / +5 / +8 % over the 96 GiB of rounds 1-2, profiles/r03/window_sweep.txt); halved automatically when the allocation fails
    uint32_t splits = 0;
    uint32_t splits_hint = 0;                // per-call suggestion of the pool (pick_splits), used when `splits` is 0
    int busy_hint = -1;                      // set by the pool per chain: 1 = other chains run beside this one (throughput forms), 0 = it is alone (latency), -1 = unknown
    uint32_t vb_radix = 0;                   // radix of the proofs' own points in the range-proof path: 16, 32 (wide chains only), 0 = default (16)
    int a_outside = 1;                       // wide chains: A (coefficient 1) added after the Horner chain instead of carried through the window sums
    uint32_t horner_lanes = 0;               // lanes per Horner chain in the range-proof path: 1, 4, 64, 0 = auto (1 on wide chains, 64 up to 256 proofs, else 4)
    struct shared_table *tab_ref = nullptr;  // refcounted, shared by the contexts of one device
    // generators
    size_t gens_capacity = 0, party_capacity = 0;
    uint32_t *d_gens = nullptr;       // [B_blinding, B, G..., H...] compressed, n_gens x 8 words
    fb_entry *d_table = nullptr;
    fb_params prm{};
    std::vector<uint8_t> h_gens;      // host copy of the encodings
    // A second, larger-window table for a SMALLER shape (n2 <= gens_capacity, m2 <= party_capacity) that the context also serves
    // (bpgpu_gens_add_shape): its generators are a subset of the primary set's, re-listed compactly [B~, B, G(n2, m2), H(n2, m2)].
    // Range proofs with n <= n2 and m <= m2 walk this table; the window pair is chosen under ONE budget (pick_window_pair).
    struct sec_table {
        size_t n = 0, m = 0;
        std::vector<uint8_t> h_gens;
        uint32_t *d_gens = nullptr;
        fb_params prm{};
        fb_entry *d_table = nullptr;
        struct shared_table *ref = nullptr;
        std::map<std::pair<size_t, size_t>, uint32_t *> ids_cache;
    } sec;
    std::map<std::pair<size_t, size_t>, uint32_t *> gen_ids_cache;  // (n,m) -> device id list
    struct script_ent {
        uint32_t *mem = nullptr;
        size_t cap = 0;
        uint64_t last_use = 0;
    };
    std::map<std::vector<uint32_t>, script_ent> script_cache;       // (n, m, k, pos, pos_begin, flags, domsep) -> transcript script (rp_script.h), LRU-bounded (script_for)
    std::vector<uint32_t *> script_retired;
    uint64_t script_tick = 0;
    int coop_defer_emit = 1;                                        // narrow chains: the scalar role's U coefficient recodings on U lanes at once (rangeproof.h rp_defer): one blocking call
                                                                    // 0.528 / 0.528 / 0.533 -> 0.521 / 0.526 / 0.518 ms, 16 threads p50 0.64 -> 0.62 ms, 16 x 128 tickets 801 -> 819 k/s
                                                                    // (profiles/r05/coop_defer_emit_ab.txt; the kernel's duration for ONE proof is unchanged, 238 us: the gain is at several
                                                                    // groups per launch); 0: the leader recodes them one after the other
    int narrow_chunk = 0;                                           // narrow chains: per-proof points per (chunk, window) lane of launch 3; 0 = 8 (the Horner wavefront adds the chunks' rows), 32 = one chunk
    int exp_single = 1;                                             // narrow chains: the generator-exponent role with one index per lane (rp_expand_b1_thread); 0: as wide chains
    int narrow_walk = 1;                                            // narrow chains: the table walk with lane = split and the partial sums folded in launch 4 (k_rp34.hip rp_walk_narrow); 0: thread = proof
    int narrow_hi_max = 32;                                         // chains of up to this many proofs give every per-proof point a second table (2^128 P) and run a 32-window Horner chain; 0: never
    int narrow_fused_finish = 1;                                    // narrow chains, verdicts only: the last workgroup of a proof in launch 4 finishes it (no finish launch)
    int msm_narrow = 1;                                             // bpgpu_msm_batch with <= 16 MSMs of <= 768 terms in all: second tables, ~sqrt(N) chunks, one tail launch (k_vb_*_hi / k_vb_tail_narrow)
    int narrow_hi4_max = 4;                                         // chains of up to this many proofs: tables of the 2^64, 2^128 and 2^192 multiples, 16-window chain (0: never).  Same-box A/B
                                                                    // (profiles/r06/narrow_hi4_ab.txt): one call 0.315 -> 0.29 ms; at <= 8 the 16 / 64 / 256-thread rows are unchanged, at 32 they lose 5 - 15 %
    int exp_w3_min_nm = 1024;                                       // wide chains of shapes with at least this many generator pairs run the exponent launch at three wavefronts per SIMD (k_rp_exponents_w3)
    int coop_split = 1;                                             // narrow chains, per-proof check: the k + 1 inversions on k + 1 lanes of the group at once, the basepoint coefficients as a
                                                                    // role of launch 3 (rangeproof.h rp_split_invert_lane / rp_rows_thread); 0: the leader does it all (A/B: profiles/r06/coop_split_ab.txt)
    int transcript_coop = 1;                                        // chains of up to 256 proofs replay their transcripts 32 lanes per proof (keccak.h): one call of 1 / 8 / 64 / 256 proofs 0.62 -> 0.53 / 0.56 / 0.57 / 0.58 ms; 0: lane = proof everywhere
    int msm_fork = 1;                                               // bpgpu_msm_batch_shared: the generator-table half on the second stream beside the per-MSM points (0: one stream -- with
                                                                    // many contexts in flight two streams each outnumber the hardware queues: config 5 on 16 / 24 / 32 contexts +1.6 / +1.7 /
                                                                    // +3.2 % MSMs/s, but one MSM alone 0.77 -> 0.98 ms: stays on; profiles/r05/msm_queue_ab.txt)
    int split_stage3 = -1;                                          // window sums and generator exponents as two launches: 1 yes, 0 no, -1 auto (chains of >= 2048 proofs)
    bool no_script = false;                                         // option "transcript_script" = 0: byte-wise replay everywhere (A/B)
    // device-resident work decomposition of the uniform (nbatch, terms-per-MSM) variable-base plans
    // One decomposition per terms-per-MSM value, built for a CAPACITY of MSMs: entry b of every array depends on b only, so the plan
    // of `cap` MSMs serves any batch of up to `cap` as a prefix (the pool's combining queue issues chains of every width; keyed by
    // (nbatch, per) the cache missed on almost every chain -- a host-side build, a hipMalloc and three blocking copies each).
    struct plan_dev {
        char *mem = nullptr;
        size_t cap = 0, o1 = 0, o2 = 0;      // MSMs it was built for; offsets of chunk_first / term_chunk inside mem
        uint64_t last_use = 0;
    };
    struct plan_view {                       // what a call of `nbatch` MSMs sees of it
        char *mem = nullptr;
        size_t o1 = 0, o2 = 0, n_chunks = 0;
        uint32_t total = 0;
    };
    uint64_t plan_tick = 0;                  // plan_cache is bounded: least-recently-used entries are retired
    std::map<size_t, plan_dev> plan_cache;   // terms per MSM (| chunk size << 40) -> plan
    std::vector<char *> plan_retired;        // outgrown / evicted blocks that launches in flight may still read: freed with the context
    // per-proof status words of the range-proof path: zero between calls (the last kernel of a call resets the
    // entries it used), so no memset launch is needed per call; `dirty` forces one after an aborted enqueue
    uint32_t *rp_status = nullptr;
    size_t rp_status_cap = 0;
    uint32_t *fin_cnt = nullptr;             // [256] arrival counters of the narrow chain's fused finish (k_rp_stage4<64>: the last workgroup of a proof finishes it and
                                             // hands its counter back zeroed)
    bool rp_status_dirty = false;
    bool test_seed_set = false;   // bpgpu_internal_set_chain_seed (tests): the per-chain key of the device-expanded randomness
    uint8_t test_seed[32];
    // A context has ONE arena / status buffer / plan cache, so the work of consecutive calls must not overlap on the
    // device: every call records order_ev at its end, and a call that arrives on a different stream than its
    // predecessor makes its stream wait for that event first (ctx_enter / ctx_leave).
    hipEvent_t order_ev = nullptr;
    hipStream_t last_stream = nullptr;
    bool have_last = false;
    host_staging io;                         // pinned staging block + persistent device IO buffer of the host-pointer entry points (host_io.h)
    char *ipp_buf = nullptr;                 // term lists of the stand-alone inner-product verifier
    size_t ipp_cap = 0;
    char *rpp_buf = nullptr;                 // working set of the batched range-proof prover
    size_t rpp_cap = 0;
    char *comb_buf = nullptr;                // combined term list, accumulators and weights of the combined checks (R1CS, linear, mixed range proofs)
    size_t comb_cap = 0;
    uint32_t r1cs_rlc_max_terms = 0;         // option "r1cs_rlc_max_terms": unique terms per combination (0 = R1_RLC_MAX_TERMS)
    uint32_t bucket_min = 0;                 // terms per MSM from which the bucket path is taken (0 = BK_MIN_TERMS; huge = never)
    int bucket_chain = 0;                    // option "bucket_chain": 0 = the fused chain (bucket2.h) where it applies, 1 = bucket.h's chain everywhere (A/B)
    int bucket_lanes = 0;                    // option "bucket_lanes": lanes of a (MSM, window) workgroup of the fused chain (0 = by batch width; 64, 128, 256)
    int exp_pairs = 1;                       // option "exponent_pairs": the generator-exponent role handles mirrored pairs of indices (0: four consecutive indices per lane, for A/B)
    int fast_tail = -1;                      // option "bucket_fast_tail" (A/B): -1 = by batch width, 0 / 1 = never / always the short-chain tail
    int walk_waves = 0;                      // option "fb_walk_waves": wavefronts the generator half of a fused chain is cut into (0 = 1024)
    // constant-time generator-table MSMs for the prover's secret-dependent commitments (msm_fixed.h fb_accum_ct_thread): their own
    // small-window table, built on first use
    bool prover_ct = false;
    fb_entry *d_table_ct = nullptr;
    fb_params prm_ct{};
    // second stream for the generator-table half of a shared-generator MSM: it is independent of the per-MSM points'
    // half until the finish, so the two halves run side by side (fork after the status memset, join before the finish)
    hipStream_t stream2 = nullptr;
    hipEvent_t fork_ev = nullptr, join_ev = nullptr;
    // result of a submitted (not yet collected) host-pointer call: where its outputs sit in the pinned buffer and where the
    // caller wants them (bpgpu_rangeproof_verify_batch_submit / bpgpu_ctx_collect)
    struct pending_result {
        bool active = false;
        const char *h_out = nullptr;
        size_t nbatch = 0, off_msm = 0, off_ts = 0;
        uint8_t *verdict = nullptr, *msm_out = nullptr, *ts_out = nullptr;
    } pend;
    bool sync_blocking = false;              // host entry points: sleep on a blocking event instead of spinning
    hipEvent_t done_ev = nullptr;
    // profiling
    bool prof = false;
    std::map<std::string, kstat> stats;
    std::vector<std::tuple<std::string, hipEvent_t, hipEvent_t>> pending;
    std::vector<hipEvent_t> ev_pool;
};

static void release_ref(shared_table *&ref, fb_entry *&tab) {
    std::lock_guard<std::mutex> lk(g_tab_mu);
    if (ref && --ref->refs == 0) {
        hipFree(ref->d_table);
        for (size_t i = 0; i < g_tables.size(); i++)
            if (g_tables[i] == ref) {
                g_tables.erase(g_tables.begin() + i);
                break;
            }
        delete ref;
    }
    ref = nullptr;
    tab = nullptr;
}
static void release_table(bpgpu_ctx *c) { release_ref(c->tab_ref, c->d_table); }
static void release_secondary(bpgpu_ctx *c) {
    release_ref(c->sec.ref, c->sec.d_table);
    if (c->sec.d_gens) hipFree(c->sec.d_gens);
    c->sec.d_gens = nullptr;
    for (auto &kv : c->sec.ids_cache) hipFree(kv.second);
    c->sec.ids_cache.clear();
    c->sec.h_gens.clear();
    c->sec.n = c->sec.m = 0;
}

static int fail(bpgpu_ctx *c, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}
#define HIPCHK(c, call)                                                                                    \
    do {                                                                                                   \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess) return fail(c, BPGPU_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

static hipEvent_t get_event(bpgpu_ctx *c) {
    if (!c->ev_pool.empty()) {
        hipEvent_t e = c->ev_pool.back();
        c->ev_pool.pop_back();
        return e;
    }
    hipEvent_t e;
    hipEventCreate(&e);
    return e;
}

// Kernel launch; with profiling on, a start/stop event pair is attached to the dispatch itself
// (hipExtLaunchKernelGGL), so the elapsed time is the kernel's own begin..end -- the timestamps rocprofv3's
// kernel trace reports -- and excludes time spent queued behind other streams' kernels.
#define LAUNCH(c, s, name, kern, grid, block, ...)                                                          \
    do {                                                                                                    \
        if ((c)->prof) {                                                                                    \
            hipEvent_t a_ = get_event(c), b_ = get_event(c);                                                \
            hipExtLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, s, a_, b_, 0, __VA_ARGS__);             \
            (c)->pending.emplace_back(name, a_, b_);                                                        \
        } else {                                                                                            \
            hipLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, s, __VA_ARGS__);                           \
        }                                                                                                   \
    } while (0)

// the same with `shm` bytes of dynamic LDS
#define LAUNCH_SHM(c, s, name, kern, grid, block, shm, ...)                                                 \
    do {                                                                                                    \
        if ((c)->prof) {                                                                                    \
            hipEvent_t a_ = get_event(c), b_ = get_event(c);                                                \
            hipExtLaunchKernelGGL(kern, dim3(grid), dim3(block), shm, s, a_, b_, 0, __VA_ARGS__);           \
            (c)->pending.emplace_back(name, a_, b_);                                                        \
        } else {                                                                                            \
            hipLaunchKernelGGL(kern, dim3(grid), dim3(block), shm, s, __VA_ARGS__);                         \
        }                                                                                                   \
    } while (0)

// a kernel template with a constant-time form: kern<true> under the name `name "_ct"`, kern<false> under `name`, the same arguments
#define LAUNCH_CT(c, s, ct, name, kern, grid, block, ...)                          \
    do {                                                                           \
        if (ct) LAUNCH(c, s, name "_ct", kern<true>, grid, block, __VA_ARGS__);    \
        else LAUNCH(c, s, name, kern<false>, grid, block, __VA_ARGS__);            \
    } while (0)
// a kernel template with two / three forms under ONE name: kern<true> or kern<false>; kern<v0>, kern<v1> or kern<v2> by sel = 0, 1, 2 -- the same arguments
#define LAUNCH_TF(c, s, flag, name, kern, grid, block, ...)                        \
    do {                                                                           \
        if (flag) LAUNCH(c, s, name, kern<true>, grid, block, __VA_ARGS__);        \
        else LAUNCH(c, s, name, kern<false>, grid, block, __VA_ARGS__);            \
    } while (0)
#define LAUNCH_SEL3(c, s, sel, v0, v1, v2, name, kern, grid, block, ...)           \
    do {                                                                           \
        if ((sel) == 0) LAUNCH(c, s, name, kern<v0>, grid, block, __VA_ARGS__);    \
        else if ((sel) == 1) LAUNCH(c, s, name, kern<v1>, grid, block, __VA_ARGS__); \
        else LAUNCH(c, s, name, kern<v2>, grid, block, __VA_ARGS__);               \
    } while (0)

static void drain_profile(bpgpu_ctx *c) {
    for (auto &t : c->pending) {
        hipEventSynchronize(std::get<2>(t));
        float ms = 0;
        hipEventElapsedTime(&ms, std::get<1>(t), std::get<2>(t));
        auto &st = c->stats[std::get<0>(t)];
        st.launches++;
        st.ms += ms;
        c->ev_pool.push_back(std::get<1>(t));
        c->ev_pool.push_back(std::get<2>(t));
    }
    c->pending.clear();
}

// arena: reset at the start of each API call; grows (with a device sync) when too small
static int arena_reserve(bpgpu_ctx *c, size_t bytes) {
    if (bytes <= c->arena_cap) return BPGPU_OK;
    HIPCHK(c, hipDeviceSynchronize());
    if (c->arena) HIPCHK(c, hipFree(c->arena));
    c->arena = nullptr;
    c->arena_cap = 0;
    size_t cap = bytes + bytes / 4 + (1 << 20);
    HIPCHK(c, hipMalloc((void **)&c->arena, cap));
    c->arena_cap = cap;
    return BPGPU_OK;
}
struct arena_plan {
    size_t total = 0;
    size_t add(size_t bytes) {
        size_t off = total;
        total += align_up(bytes);
        return off;
    }
};

static uint64_t table_bytes(uint32_t n_gens, uint32_t W);

static int collect_locked(bpgpu_ctx *c);
// ---- ordering of calls on one context (see bpgpu_ctx::order_ev) ----
// keep_staging: the call continues an earlier one of the same entry point and still holds pointers into the pinned staging
// buffers (the per-proof fallback of the batch-combined check): nothing retired is freed
static int ctx_enter(bpgpu_ctx *c, hipStream_t s, bool keep_staging = false) {
    if (c->pend.active) {   // a submitted call's results still sit in the staging buffers: deliver them first
        int rcp = collect_locked(c);
        if (rcp) return rcp;
    }
    int rc = c->io.begin(keep_staging);
    if (rc) return rc;
    if (c->have_last && c->last_stream != s) HIPCHK(c, hipStreamWaitEvent(s, c->order_ev, 0));
    return BPGPU_OK;
}
static int ctx_leave(bpgpu_ctx *c, hipStream_t s) {
    HIPCHK(c, hipEventRecord(c->order_ev, s));
    c->last_stream = s;
    c->have_last = true;
    return c->io.left(s);
}
// wait for everything enqueued on s (host-pointer entry points): spin, or sleep on a blocking event
static int host_wait(bpgpu_ctx *c, hipStream_t s) {
    if (c->sync_blocking) {
        HIPCHK(c, hipEventRecord(c->done_ev, s));
        HIPCHK(c, hipEventSynchronize(c->done_ev));
    } else {
        HIPCHK(c, hipStreamSynchronize(s));
    }
    c->io.waited();
    return BPGPU_OK;
}
// the device working sets a prover call clears on its way out, besides the IO buffer (host_call::finish)
static void secret_spans(bpgpu_ctx *c, dev_span b[3]) {
    b[0] = {c->rpp_buf, c->rpp_cap};
    b[1] = {c->ipp_buf, c->ipp_cap};
    b[2] = {c->arena, c->arena_cap};
}
static int os_random(bpgpu_ctx *c, char *dst, size_t bytes);
// finish a submitted call: wait for its stream work and hand the results to the caller's buffers
static int collect_locked(bpgpu_ctx *c) {
    if (!c->pend.active) return BPGPU_OK;
    bpgpu_ctx::pending_result p = c->pend;
    c->pend.active = false;
    int rc = host_wait(c, c->stream);
    if (rc) return rc;
    memcpy(p.verdict, p.h_out, p.nbatch);
    if (p.msm_out) memcpy(p.msm_out, p.h_out + p.off_msm, p.nbatch * 32);
    if (p.ts_out) memcpy(p.ts_out, p.h_out + p.off_ts, p.nbatch * BPGPU_TRANSCRIPT_BYTES);
    return BPGPU_OK;
}

extern "C" {

int bpgpu_version(void) { return 100; }

int bpgpu_ctx_create(int device, bpgpu_ctx **out) {
    if (!out) return BPGPU_ERR_INVALID_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return BPGPU_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return BPGPU_ERR_NO_DEVICE;
    bpgpu_ctx *c = new bpgpu_ctx();
    c->device = device;
    c->io.err = &c->err;
    c->io.hip_err_code = BPGPU_ERR_HIP;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->order_ev, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->io.pin_ev, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->done_ev, hipEventDisableTiming | hipEventBlockingSync) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->join_ev, hipEventDisableTiming) != hipSuccess) {
        delete c;
        return BPGPU_ERR_HIP;
    }
    if (const char *e = getenv("BPGPU_COOP_SPLIT")) c->coop_split = atoi(e) != 0;
    if (const char *e = getenv("BPGPU_EXP_W3_MIN_NM")) c->exp_w3_min_nm = atoi(e);   // (A/B only)
    if (const char *e = getenv("BPGPU_NARROW_WALK")) c->narrow_walk = atoi(e) != 0;
    if (const char *e = getenv("BPGPU_NARROW_FUSED_FINISH")) c->narrow_fused_finish = atoi(e) != 0;
    if (const char *e = getenv("BPGPU_NARROW_HI_MAX")) c->narrow_hi_max = atoi(e);
    if (const char *e = getenv("BPGPU_NARROW_HI4_MAX")) c->narrow_hi4_max = atoi(e);
    if (const char *e = getenv("BPGPU_EXP_SINGLE")) c->exp_single = atoi(e) != 0;
    if (const char *e = getenv("BPGPU_NARROW_CHUNK")) c->narrow_chunk = atoi(e);
    if (const char *e = getenv("BPGPU_COOP_DEFER_EMIT")) c->coop_defer_emit = atoi(e) != 0;   // (A/B of whole test suites: the option's default for every context of the process)
    *out = c;
    return BPGPU_OK;
}

void bpgpu_ctx_destroy(bpgpu_ctx *c) {
    if (!c) return;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    c->pend.active = false;   // results of a submitted call nobody collected are dropped
    drain_profile(c);
    for (auto e : c->ev_pool) hipEventDestroy(e);
    for (auto &kv : c->gen_ids_cache) hipFree(kv.second);
    for (auto &kv : c->script_cache) hipFree(kv.second.mem);
    for (uint32_t *q : c->script_retired) hipFree(q);
    for (auto &kv : c->plan_cache) hipFree(kv.second.mem);
    for (char *q : c->plan_retired) hipFree(q);
    if (c->arena) hipFree(c->arena);
    c->io.release();
    if (c->ipp_buf) hipFree(c->ipp_buf);
    if (c->rpp_buf) hipFree(c->rpp_buf);
    if (c->comb_buf) hipFree(c->comb_buf);
    if (c->order_ev) hipEventDestroy(c->order_ev);
    if (c->done_ev) hipEventDestroy(c->done_ev);
    if (c->fork_ev) hipEventDestroy(c->fork_ev);
    if (c->join_ev) hipEventDestroy(c->join_ev);
    if (c->stream2) hipStreamDestroy(c->stream2);
    if (c->rp_status) hipFree(c->rp_status);
    if (c->fin_cnt) hipFree(c->fin_cnt);
    if (c->d_table_ct) hipFree(c->d_table_ct);
    if (c->d_gens) hipFree(c->d_gens);
    release_secondary(c);
    release_table(c);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

const char *bpgpu_last_error(bpgpu_ctx *c) { return c ? c->err.c_str() : "null context"; }

int bpgpu_ctx_set_option(bpgpu_ctx *c, const char *key, int64_t value) {
    if (!c || !key) return BPGPU_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!strcmp(key, "fixed_window_bits")) {
        if (value != 0 && (value < 2 || value > 20)) return fail(c, BPGPU_ERR_INVALID_ARG, "fixed_window_bits must be 0 (auto) or 2..20");
        if (c->d_table) return fail(c, BPGPU_ERR_INVALID_ARG, "set fixed_window_bits before loading generators");
        c->W = (uint32_t)value;
        return BPGPU_OK;
    }
    if (!strcmp(key, "fixed_table_max_bytes")) {
        if (value < (1 << 20)) return fail(c, BPGPU_ERR_INVALID_ARG, "fixed_table_max_bytes too small");
        if (c->d_table) return fail(c, BPGPU_ERR_INVALID_ARG, "set fixed_table_max_bytes before loading generators");
        c->table_budget = (uint64_t)value;
        return BPGPU_OK;
    }
    if (!strcmp(key, "fixed_splits")) {
        if (value < 0 || value > 4096) return fail(c, BPGPU_ERR_INVALID_ARG, "fixed_splits out of range");
        c->splits = (uint32_t)value;
        return BPGPU_OK;
    }
    if (!strcmp(key, "per_proof_radix")) {
        if (value != 0 && value != 16 && value != 32) return fail(c, BPGPU_ERR_INVALID_ARG, "per_proof_radix must be 0 (auto), 16 or 32");
        c->vb_radix = (uint32_t)value;
        return BPGPU_OK;
    }
    if (!strcmp(key, "a_outside")) {
        c->a_outside = value != 0;
        return BPGPU_OK;
    }
    if (!strcmp(key, "horner_lanes")) {
        if (value != 0 && value != 1 && value != 4 && value != 64) return fail(c, BPGPU_ERR_INVALID_ARG, "horner_lanes must be 0 (auto), 1, 4 or 64");
        c->horner_lanes = (uint32_t)value;
        return BPGPU_OK;
    }
    if (!strcmp(key, "host_sync_blocking")) {
        c->sync_blocking = value != 0;
        return BPGPU_OK;
    }
    if (!strcmp(key, "transcript_script")) {
        c->no_script = value == 0;
        return BPGPU_OK;
    }
    if (!strcmp(key, "exp_single")) {
        c->exp_single = value != 0;
        return BPGPU_OK;
    }
    if (!strcmp(key, "narrow_hi4_max")) {
        if (value < 0 || value > 256) return fail(c, BPGPU_ERR_INVALID_ARG, "narrow_hi4_max must be 0 .. 256");
        c->narrow_hi4_max = (int)value;
        return BPGPU_OK;
    }
    if (!strcmp(key, "narrow_hi_max")) {
        if (value < 0 || value > 256) return fail(c, BPGPU_ERR_INVALID_ARG, "narrow_hi_max must be 0 .. 256");
        c->narrow_hi_max = (int)value;
        return BPGPU_OK;
    }
    if (!strcmp(key, "narrow_fused_finish")) {
        c->narrow_fused_finish = value != 0;
        return BPGPU_OK;
    }
    if (!strcmp(key, "msm_narrow")) {
        c->msm_narrow = value != 0;
        return BPGPU_OK;
    }
    if (!strcmp(key, "narrow_walk")) {
        c->narrow_walk = value != 0;
        return BPGPU_OK;
    }
    if (!strcmp(key, "coop_split")) {
        c->coop_split = value != 0;
        return BPGPU_OK;
    }
    if (!strcmp(key, "narrow_chunk")) {
        if (value < 0 || value > BP_VB_CHUNK) return fail(c, BPGPU_ERR_INVALID_ARG, "narrow_chunk must be 0 (automatic) or 2 .. 32");
        c->narrow_chunk = (int)value;
        return BPGPU_OK;
    }
    if (!strcmp(key, "coop_defer_emit")) {
        c->coop_defer_emit = value != 0;
        return BPGPU_OK;
    }
    if (!strcmp(key, "transcript_coop")) {
        if (value < 0 || value > 1) return fail(c, BPGPU_ERR_INVALID_ARG, "transcript_coop must be 0 or 1");
        c->transcript_coop = (int)value;
        return BPGPU_OK;
    }
    if (!strcmp(key, "msm_fork")) {
        c->msm_fork = value != 0;
        return BPGPU_OK;
    }
    if (!strcmp(key, "split_stage3")) {
        c->split_stage3 = value < 0 ? -1 : (value != 0);
        return BPGPU_OK;
    }
    if (!strcmp(key, "prover_constant_time")) {
        c->prover_ct = value != 0;
        return BPGPU_OK;
    }
    if (!strcmp(key, "bucket_min_terms")) {
        if (value < 0 || value > 0x7fffffff) return fail(c, BPGPU_ERR_INVALID_ARG, "bucket_min_terms out of range");
        c->bucket_min = (uint32_t)value;
        return BPGPU_OK;
    }
    if (!strcmp(key, "bucket_chain")) {
        if (value < 0 || value > 1) return fail(c, BPGPU_ERR_INVALID_ARG, "bucket_chain must be 0 (fused chain where it applies) or 1 (bucket.h's chain)");
        c->bucket_chain = (int)value;
        return BPGPU_OK;
    }
    if (!strcmp(key, "exponent_pairs")) {
        c->exp_pairs = value != 0;
        return BPGPU_OK;
    }
    if (!strcmp(key, "bucket_fast_tail")) {
        c->fast_tail = value < 0 ? -1 : (value != 0);
        return BPGPU_OK;
    }
    if (!strcmp(key, "fb_walk_waves")) {
        if (value < 0 || value > 65536) return fail(c, BPGPU_ERR_INVALID_ARG, "fb_walk_waves out of range");
        c->walk_waves = (int)value;
        return BPGPU_OK;
    }
    if (!strcmp(key, "bucket_lanes")) {
        if (value != 0 && value != 64 && value != 128 && value != 256) return fail(c, BPGPU_ERR_INVALID_ARG, "bucket_lanes must be 0 (auto), 64, 128 or 256");
        c->bucket_lanes = (int)value;
        return BPGPU_OK;
    }
    if (!strcmp(key, "r1cs_rlc_max_terms")) {
        if (value < 0 || value > R1_RLC_MAX_TERMS) return fail(c, BPGPU_ERR_INVALID_ARG, "r1cs_rlc_max_terms must be 0 (default) .. 2^24");
        c->r1cs_rlc_max_terms = (uint32_t)value;
        return BPGPU_OK;
    }
    return fail(c, BPGPU_ERR_INVALID_ARG, "unknown option %s", key);
}

int bpgpu_ctx_get_option(bpgpu_ctx *c, const char *key, int64_t *value) {
    if (!c || !key || !value) return BPGPU_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!strcmp(key, "fixed_window_bits")) *value = c->d_table ? c->prm.W : c->W;          // effective once tables exist
    else if (!strcmp(key, "fixed_table_bytes")) *value = c->d_table ? (int64_t)table_bytes(c->prm.n_gens, c->prm.W) : 0;
    else if (!strcmp(key, "fixed_table_max_bytes")) *value = (int64_t)c->table_budget;
    else if (!strcmp(key, "secondary_window_bits")) *value = c->sec.d_table ? c->sec.prm.W : 0;
    else if (!strcmp(key, "secondary_table_bytes")) *value = c->sec.d_table ? (int64_t)table_bytes(c->sec.prm.n_gens, c->sec.prm.W) : 0;
    else if (!strcmp(key, "secondary_shape_n")) *value = (int64_t)c->sec.n;
    else if (!strcmp(key, "secondary_shape_m")) *value = (int64_t)c->sec.m;
    else if (!strcmp(key, "fixed_splits")) *value = c->splits;
    else if (!strcmp(key, "horner_lanes")) *value = c->horner_lanes;
    else if (!strcmp(key, "per_proof_radix")) *value = c->vb_radix;
    else if (!strcmp(key, "a_outside")) *value = c->a_outside;
    else if (!strcmp(key, "host_sync_blocking")) *value = c->sync_blocking ? 1 : 0;
    else if (!strcmp(key, "transcript_script")) *value = c->no_script ? 0 : 1;
    else if (!strcmp(key, "prover_constant_time")) *value = c->prover_ct ? 1 : 0;
    else if (!strcmp(key, "bucket_min_terms")) *value = c->bucket_min ? c->bucket_min : BK_MIN_TERMS;
    else if (!strcmp(key, "bucket_chain")) *value = c->bucket_chain;
    else if (!strcmp(key, "bucket_lanes")) *value = c->bucket_lanes;
    else if (!strcmp(key, "bucket_fast_tail")) *value = c->fast_tail;
    else if (!strcmp(key, "exponent_pairs")) *value = c->exp_pairs;
    else if (!strcmp(key, "split_stage3")) *value = c->split_stage3;
    else if (!strcmp(key, "transcript_coop")) *value = c->transcript_coop;
    else if (!strcmp(key, "coop_split")) *value = c->coop_split;
    else if (!strcmp(key, "coop_defer_emit")) *value = c->coop_defer_emit;
    else if (!strcmp(key, "narrow_hi_max")) *value = c->narrow_hi_max;
    else if (!strcmp(key, "narrow_hi4_max")) *value = c->narrow_hi4_max;
    else if (!strcmp(key, "narrow_fused_finish")) *value = c->narrow_fused_finish;
    else if (!strcmp(key, "fb_walk_waves")) *value = c->walk_waves ? c->walk_waves : 2048;
    else if (!strcmp(key, "r1cs_rlc_max_terms")) *value = c->r1cs_rlc_max_terms ? c->r1cs_rlc_max_terms : R1_RLC_MAX_TERMS;
    else if (!strcmp(key, "staging_residue")) {
        // test hook: non-zero bytes left in the persistent staging buffers (pinned block, device IO buffer, prover working sets,
        // arena) -- 0 after a prover entry point has returned (host_call::finish)
        if (hipSetDevice(c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(c, BPGPU_ERR_HIP, "synchronize failed");
        int64_t nz = 0;
        for (size_t i = 0; i < c->io.pin_cap && i < c->io.last_secret_bytes; i++) nz += c->io.pin[i] != 0;   // (behind the secrets: public outputs)
        std::vector<char> tmp;
        const std::pair<const char *, size_t> bufs[4] = {{c->io.io_dev, c->io.io_cap}, {c->rpp_buf, c->rpp_cap}, {c->ipp_buf, c->ipp_cap}, {c->arena, c->arena_cap}};
        for (const auto &b : bufs) {
            if (!b.first || !b.second) continue;
            tmp.resize(b.second);
            if (hipMemcpy(tmp.data(), b.first, b.second, hipMemcpyDeviceToHost) != hipSuccess) return fail(c, BPGPU_ERR_HIP, "read-back failed");
            for (char ch : tmp) nz += ch != 0;
        }
        *value = nz;
    }
    else return fail(c, BPGPU_ERR_INVALID_ARG, "unknown option %s", key);
    return BPGPU_OK;
}

int bpgpu_synchronize(bpgpu_ctx *c) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BPGPU_OK;
}

int bpgpu_profile_enable(bpgpu_ctx *c, int on) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    c->prof = on != 0;
    return BPGPU_OK;
}
int bpgpu_profile_reset(bpgpu_ctx *c) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    drain_profile(c);
    c->stats.clear();
    return BPGPU_OK;
}
int bpgpu_profile_report(bpgpu_ctx *c, char *buf, size_t cap) {
    if (!c || !buf || cap == 0) return BPGPU_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    drain_profile(c);
    std::string s;
    for (auto &kv : c->stats) {
        char line[256];
        snprintf(line, sizeof line, "%s %llu %.6f\n", kv.first.c_str(), (unsigned long long)kv.second.launches, kv.second.ms);
        s += line;
    }
    snprintf(buf, cap, "%s", s.c_str());
    return BPGPU_OK;
}

}  // extern "C"

// ============================================================================
// generators
// ============================================================================
static uint64_t table_bytes(uint32_t n_gens, uint32_t W) { return (uint64_t)n_gens * fb_nwin(W) * (1ull << (W - 1)) * sizeof(fb_entry); }

// One window table for the generator list (h_gens on the host, d_gens on the device: n_gens compressed points): found among the tables
// the process already holds on this device, or built.  W_fixed = 0: the fewest windows (= additions per generator term) whose table
// fits `budget`; ties: the smaller table.
static int build_table_set(bpgpu_ctx *c, const std::vector<uint8_t> &h_gens, const uint32_t *d_gens, uint32_t W_fixed, uint64_t budget0, fb_params *prm_out,
                           shared_table **ref_out, fb_entry **tab_out) {
    fb_params prm;
    prm.n_gens = (uint32_t)(h_gens.size() / 32);
    std::lock_guard<std::mutex> lk_build(g_tab_build_mu[(unsigned)c->device & 63u]);
    uint32_t W = W_fixed;
    fb_entry *d_table = nullptr;
    size_t entries = 0;
    for (uint64_t budget = budget0;; budget /= 2) {
        if (W_fixed == 0) {
            W = 4;
            for (uint32_t w = 5; w <= 20; w++)
                if (table_bytes(prm.n_gens, w) <= budget && fb_nwin(w) < fb_nwin(W)) W = w;
        }
        prm.W = W;
        prm.nwin = fb_nwin(W);
        prm.half = 1u << (W - 1);
        *prm_out = prm;
        {
            std::lock_guard<std::mutex> lk(g_tab_mu);
            for (shared_table *t : g_tables)
                if (t->device == c->device && t->W == W && t->gens == h_gens) {
                    t->refs++;
                    *ref_out = t;
                    *tab_out = t->d_table;
                    return BPGPU_OK;
                }
        }
        entries = (size_t)prm.n_gens * prm.nwin * prm.half;
        if (hipMalloc((void **)&d_table, entries * sizeof(fb_entry)) == hipSuccess) break;
        (void)hipGetLastError();
        d_table = nullptr;
        // automatic window: the HBM may be shared with other tenants -- settle for a smaller table
        if (W_fixed != 0 || W <= 8) return fail(c, BPGPU_ERR_HIP, "hipMalloc of %zu table bytes (W = %u) failed", entries * sizeof(fb_entry), W);
    }
    ge_ext *d_base = nullptr;
    uint32_t *d_bad = nullptr;
    if (hipMalloc((void **)&d_base, (size_t)prm.n_gens * prm.nwin * sizeof(ge_ext)) != hipSuccess ||
        hipMalloc((void **)&d_bad, 4) != hipSuccess) {
        hipFree(d_table);
        return fail(c, BPGPU_ERR_HIP, "hipMalloc of table scratch failed");
    }
    hipMemsetAsync(d_bad, 0, 4, c->stream);
    LAUNCH(c, c->stream, "fb_base", k_fb_base, (prm.n_gens + 63) / 64, 64, prm, d_gens, d_base, d_bad);
    LAUNCH(c, c->stream, "fb_fill", k_fb_fill, (prm.n_gens * prm.nwin + 63) / 64, 64, prm, d_base, d_table);
    const uint64_t n_groups = (entries + BP_FB_NORM_GROUP - 1) / BP_FB_NORM_GROUP;
    LAUNCH(c, c->stream, "fb_norm", k_fb_norm, (uint32_t)((n_groups + 63) / 64), 64, n_groups, (uint64_t)entries, d_table);
    uint32_t bad = 0;
    hipError_t e1 = hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, c->stream);
    hipError_t e2 = hipStreamSynchronize(c->stream);
    hipError_t e3 = hipGetLastError();
    hipFree(d_base);
    hipFree(d_bad);
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) {
        hipFree(d_table);
        return fail(c, BPGPU_ERR_HIP, "table construction failed: %s", hipGetErrorString(e2 != hipSuccess ? e2 : (e1 != hipSuccess ? e1 : e3)));
    }
    if (bad) {
        hipFree(d_table);
        return fail(c, BPGPU_ERR_BAD_GENERATOR, "a generator encoding does not decode");
    }
    shared_table *t = new shared_table{c->device, W, h_gens, d_table, 1};
    {
        std::lock_guard<std::mutex> lk(g_tab_mu);
        g_tables.push_back(t);
    }
    *ref_out = t;
    *tab_out = d_table;
    return BPGPU_OK;
}

static int build_tables(bpgpu_ctx *c, uint32_t W_override = 0) {
    // c->d_gens / c->h_gens hold n_gens compressed points
    release_secondary(c);   // (belongs to the previous generator set)
    release_table(c);
    if (c->d_table_ct) {   // belongs to the previous generator set
        hipFree(c->d_table_ct);
        c->d_table_ct = nullptr;
    }
    for (auto &kv : c->gen_ids_cache) hipFree(kv.second);
    c->gen_ids_cache.clear();
    return build_table_set(c, c->h_gens, c->d_gens, W_override ? W_override : c->W, c->table_budget, &c->prm, &c->tab_ref, &c->d_table);
}

// Windows for TWO shapes under one budget (bpgpu_gens_add_shape): the pair (W1 for the primary set of n1 generators, W2 for the secondary
// set of n2) that minimises the sum of the two walks' lengths RELATIVE to what each would get alone with the whole budget --
// nwin(W1) / nwin(W1*) + nwin(W2) / nwin(W2*) -- among the pairs whose tables fit together; ties: fewer bytes.  W1_fixed != 0 pins W1.
static void pick_window_pair(uint32_t n1, uint32_t n2, uint64_t budget, uint32_t W1_fixed, uint32_t *W1, uint32_t *W2) {
    auto best_alone = [&](uint32_t ng) {
        uint32_t W = 4;
        for (uint32_t w = 5; w <= 20; w++)
            if (table_bytes(ng, w) <= budget && fb_nwin(w) < fb_nwin(W)) W = w;
        return W;
    };
    const double a1 = fb_nwin(best_alone(n1)), a2 = fb_nwin(best_alone(n2));
    double best = 1e30;
    uint64_t best_bytes = ~0ull;
    *W1 = W1_fixed ? W1_fixed : 4;
    *W2 = 4;
    for (uint32_t w1 = W1_fixed ? W1_fixed : 4; w1 <= (W1_fixed ? W1_fixed : 20); w1++)
        for (uint32_t w2 = 4; w2 <= 20; w2++) {
            const uint64_t bytes = table_bytes(n1, w1) + table_bytes(n2, w2);
            if (bytes > budget && !(w1 == (W1_fixed ? W1_fixed : 4) && w2 == 4)) continue;
            const double f = fb_nwin(w1) / a1 + fb_nwin(w2) / a2;
            if (f < best - 1e-12 || (f < best + 1e-12 && bytes < best_bytes)) {
                best = f;
                best_bytes = bytes;
                *W1 = w1;
                *W2 = w2;
            }
        }
}
// (tests/test_abi_and_host.py: the choice is plain host logic)
extern "C" void bpgpu_internal_window_pair(uint32_t n_gens_primary, uint32_t n_gens_secondary, uint64_t budget, uint32_t W1_fixed, uint32_t *W1, uint32_t *W2) {
    pick_window_pair(n_gens_primary, n_gens_secondary, budget, W1_fixed, W1, W2);
}

// BulletproofGens::new(gens_capacity, party_capacity) serves every (n <= gens_capacity, m <= party_capacity) (generators.rs:157-259); the
// window table that replaces the doublings is sized for the whole set, so a service that verifies m = 16 AND m = 1 proofs walked the
// m = 1 ones through 16-bit windows (-9 %).  This adds a second table over the sub-set (n2, m2) and re-balances both windows under the
// context's one budget (fixed_table_max_bytes).  Called again, it replaces the secondary shape.
extern "C" int bpgpu_gens_add_shape(bpgpu_ctx *c, size_t n2, size_t m2) {
    if (!c || n2 == 0 || m2 == 0) return BPGPU_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (c->h_gens.empty()) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    if (n2 > c->gens_capacity || m2 > c->party_capacity) return fail(c, BPGPU_ERR_NO_GENS, "the secondary shape exceeds the generator set");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream2));
    const uint32_t n1 = (uint32_t)(2 + 2 * c->gens_capacity * c->party_capacity), ng2 = (uint32_t)(2 + 2 * n2 * m2);
    uint32_t W1 = 0, W2 = 0;
    pick_window_pair(n1, ng2, c->table_budget, c->W, &W1, &W2);
    release_secondary(c);
    if (!c->d_table || c->prm.W != W1) {   // the primary table makes room (or was dropped by the pool before the re-balancing)
        const int rc = build_tables(c, W1);
        if (rc) return rc;
    }
    const size_t tot = c->gens_capacity * c->party_capacity;
    std::vector<uint8_t> &h2 = c->sec.h_gens;
    h2.assign((size_t)ng2 * 32, 0);
    memcpy(&h2[0], &c->h_gens[0], 64);   // B~, B
    for (size_t j = 0; j < m2; j++) {
        memcpy(&h2[64 + j * n2 * 32], &c->h_gens[64 + j * c->gens_capacity * 32], n2 * 32);
        memcpy(&h2[64 + (m2 * n2 + j * n2) * 32], &c->h_gens[64 + (tot + j * c->gens_capacity) * 32], n2 * 32);
    }
    HIPCHK(c, hipMalloc((void **)&c->sec.d_gens, h2.size()));
    HIPCHK(c, hipMemcpy(c->sec.d_gens, h2.data(), h2.size(), hipMemcpyHostToDevice));
    const int rc = build_table_set(c, h2, c->sec.d_gens, W2, c->table_budget, &c->sec.prm, &c->sec.ref, &c->sec.d_table);
    if (rc) {
        release_secondary(c);
        return rc;
    }
    c->sec.n = n2;
    c->sec.m = m2;
    return BPGPU_OK;
}
// the pool re-balances a whole device: every lane lets go of its tables first, so that the old and the new pair never coexist in HBM
extern "C" int bpgpu_internal_release_tables(bpgpu_ctx *c) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream2));
    release_secondary(c);
    release_table(c);
    return BPGPU_OK;
}

// the small-window table of the constant-time path (W = 4: 64 KiB per generator), built on first use
static int build_ct_table(bpgpu_ctx *c) {
    if (c->d_table_ct) return BPGPU_OK;
    fb_params prm;
    prm.n_gens = c->prm.n_gens;
    prm.W = BP_FB_CT_W;
    prm.nwin = fb_nwin(prm.W);
    prm.half = 1u << (prm.W - 1);
    const size_t entries = (size_t)prm.n_gens * prm.nwin * prm.half;
    fb_entry *d_table = nullptr;
    ge_ext *d_base = nullptr;
    uint32_t *d_bad = nullptr;
    if (hipMalloc((void **)&d_table, entries * sizeof(fb_entry)) != hipSuccess || hipMalloc((void **)&d_base, (size_t)prm.n_gens * prm.nwin * sizeof(ge_ext)) != hipSuccess ||
        hipMalloc((void **)&d_bad, 4) != hipSuccess) {
        if (d_table) hipFree(d_table);
        if (d_base) hipFree(d_base);
        return fail(c, BPGPU_ERR_HIP, "hipMalloc of the constant-time table failed");
    }
    hipMemsetAsync(d_bad, 0, 4, c->stream);
    LAUNCH(c, c->stream, "fb_base", k_fb_base, (prm.n_gens + 63) / 64, 64, prm, c->d_gens, d_base, d_bad);
    LAUNCH(c, c->stream, "fb_fill", k_fb_fill, (prm.n_gens * prm.nwin + 63) / 64, 64, prm, d_base, d_table);
    const uint64_t n_groups = (entries + BP_FB_NORM_GROUP - 1) / BP_FB_NORM_GROUP;
    LAUNCH(c, c->stream, "fb_norm", k_fb_norm, (uint32_t)((n_groups + 63) / 64), 64, n_groups, (uint64_t)entries, d_table);
    const hipError_t e = hipStreamSynchronize(c->stream);
    hipFree(d_base);
    hipFree(d_bad);
    if (e != hipSuccess) {
        hipFree(d_table);
        return fail(c, BPGPU_ERR_HIP, "constant-time table construction failed: %s", hipGetErrorString(e));
    }
    c->d_table_ct = d_table;
    c->prm_ct = prm;
    return BPGPU_OK;
}
// the window tables a launch walks and their parameters: the context's, or -- ct -- the constant-time path's, built on first use
struct fb_walk {
    fb_params prm;
    const fb_entry *table;
};
static int fb_walk_for(bpgpu_ctx *c, bool ct, fb_walk &w) {
    if (ct) {
        const int rc = build_ct_table(c);
        if (rc) return rc;
    }
    w.prm = ct ? c->prm_ct : c->prm;
    w.table = ct ? c->d_table_ct : c->d_table;
    return BPGPU_OK;
}

static int load_gens_locked(bpgpu_ctx *c, size_t gens_capacity, size_t party_capacity, const uint8_t *G, const uint8_t *H,
                            const uint8_t *B, const uint8_t *Bb) {
    const size_t tot = gens_capacity * party_capacity;
    c->gens_capacity = gens_capacity;
    c->party_capacity = party_capacity;
    c->h_gens.assign((2 + 2 * tot) * 32, 0);
    memcpy(&c->h_gens[0], Bb, 32);
    memcpy(&c->h_gens[32], B, 32);
    memcpy(&c->h_gens[64], G, tot * 32);
    memcpy(&c->h_gens[64 + tot * 32], H, tot * 32);
    if (c->d_gens) HIPCHK(c, hipFree(c->d_gens));
    c->d_gens = nullptr;
    HIPCHK(c, hipMalloc((void **)&c->d_gens, c->h_gens.size()));
    HIPCHK(c, hipMemcpy(c->d_gens, c->h_gens.data(), c->h_gens.size(), hipMemcpyHostToDevice));
    return build_tables(c);
}

extern "C" int bpgpu_gens_load(bpgpu_ctx *c, size_t gens_capacity, size_t party_capacity, const uint8_t *G, const uint8_t *H,
                               const uint8_t B[32], const uint8_t Bb[32]) {
    if (!c || !G || !H || !B || !Bb || gens_capacity == 0 || party_capacity == 0) return BPGPU_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return load_gens_locked(c, gens_capacity, party_capacity, G, H, B, Bb);
}

extern "C" int bpgpu_gens_export(bpgpu_ctx *c, uint8_t *G, uint8_t *H, uint8_t B[32], uint8_t Bb[32]) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->h_gens.empty()) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    const size_t tot = c->gens_capacity * c->party_capacity;
    if (Bb) memcpy(Bb, &c->h_gens[0], 32);
    if (B) memcpy(B, &c->h_gens[32], 32);
    if (G) memcpy(G, &c->h_gens[64], tot * 32);
    if (H) memcpy(H, &c->h_gens[64 + tot * 32], tot * 32);
    return BPGPU_OK;
}

// id list of the generator terms of an (n, m) proof in the reference's order
// (B_blinding, B, G(n,m), H(n,m)); ids index the loaded table.  g_only: (B_blinding, B, G(n,m)) -- the bases of a
// LinearProof over bp_gens.share(j).G(n) (linear_proof.rs:405-411)
static int gen_ids_for(bpgpu_ctx *c, size_t n, size_t m, uint32_t **out, bool g_only = false) {
    auto key = std::make_pair(n, g_only ? m + ((size_t)1 << 40) : m);
    auto it = c->gen_ids_cache.find(key);
    if (it != c->gen_ids_cache.end()) {
        *out = it->second;
        return BPGPU_OK;
    }
    std::vector<uint32_t> ids;
    const size_t tot = c->gens_capacity * c->party_capacity;
    ids.push_back(0);
    ids.push_back(1);
    for (size_t j = 0; j < m; j++)
        for (size_t i = 0; i < n; i++) ids.push_back((uint32_t)(2 + j * c->gens_capacity + i));
    for (size_t j = 0; j < m && !g_only; j++)
        for (size_t i = 0; i < n; i++) ids.push_back((uint32_t)(2 + tot + j * c->gens_capacity + i));
    uint32_t *d = nullptr;
    HIPCHK(c, hipMalloc((void **)&d, ids.size() * 4));
    HIPCHK(c, hipMemcpy(d, ids.data(), ids.size() * 4, hipMemcpyHostToDevice));
    c->gen_ids_cache[key] = d;
    *out = d;
    return BPGPU_OK;
}

// the same list relative to the secondary table's compact layout [B~, B, G(n2, m2), H(n2, m2)]
static int gen_ids_for_secondary(bpgpu_ctx *c, size_t n, size_t m, uint32_t **out) {
    auto key = std::make_pair(n, m);
    auto it = c->sec.ids_cache.find(key);
    if (it != c->sec.ids_cache.end()) {
        *out = it->second;
        return BPGPU_OK;
    }
    std::vector<uint32_t> ids = {0, 1};
    for (size_t j = 0; j < m; j++)
        for (size_t i = 0; i < n; i++) ids.push_back((uint32_t)(2 + j * c->sec.n + i));
    for (size_t j = 0; j < m; j++)
        for (size_t i = 0; i < n; i++) ids.push_back((uint32_t)(2 + c->sec.n * c->sec.m + j * c->sec.n + i));
    uint32_t *d = nullptr;
    HIPCHK(c, hipMalloc((void **)&d, ids.size() * 4));
    HIPCHK(c, hipMemcpy(d, ids.data(), ids.size() * 4, hipMemcpyHostToDevice));
    c->sec.ids_cache[key] = d;
    *out = d;
    return BPGPU_OK;
}

// ============================================================================
// variable-base MSM
// ============================================================================
struct vb_plan {
    std::vector<vb_chunk> chunks;
    std::vector<uint32_t> chunk_first, term_chunk;
    uint32_t total = 0;
};
static void make_vb_plan(vb_plan &pl, size_t nbatch, const uint32_t *n_terms, uint32_t chunk = BP_VB_CHUNK) {
    pl.chunk_first.resize(nbatch + 1);
    uint32_t t0 = 0;
    for (size_t b = 0; b < nbatch; b++) {
        pl.chunk_first[b] = (uint32_t)pl.chunks.size();
        for (uint32_t k = 0; k < n_terms[b]; k += chunk) {
            vb_chunk ch;
            ch.msm = (uint32_t)b;
            ch.first = t0 + k;
            ch.count = n_terms[b] - k < chunk ? n_terms[b] - k : chunk;
            ch.pad = 0;
            for (uint32_t i = 0; i < ch.count; i++) pl.term_chunk.push_back((uint32_t)pl.chunks.size());
            pl.chunks.push_back(ch);
        }
        t0 += n_terms[b];
    }
    pl.chunk_first[nbatch] = (uint32_t)pl.chunks.size();
    pl.total = t0;
}

// Enqueue the variable-base stages up to the per-MSM column sums.  Scratch comes from the
// arena at [base + offsets].  Returns device pointers through the struct.
struct vb_dev {
    vb_chunk *chunks;
    uint32_t *chunk_first, *term_chunk, *recoded;
    ge_cached *tab;
    ge_ext *part;
    uint32_t *colq16;   // [msm][64][4][8 words]: column sums as 16-bit limbs for the wavefront Horner
    ge_ext *hq;         // [msm] Horner results
};
static void plan_vb(arena_plan &ap, const vb_plan &pl, size_t nbatch, size_t off[7], size_t tab_entries = 8) {
    off[0] = ap.add(pl.chunks.size() * sizeof(vb_chunk) + 16);
    off[1] = ap.add((nbatch + 1) * 4);
    off[2] = ap.add((size_t)pl.total * 4 + 16);
    off[3] = ap.add((size_t)pl.total * 32 + 16);
    off[4] = ap.add((size_t)pl.total * tab_entries * sizeof(ge_cached) + 16);
    off[5] = ap.add(pl.chunks.size() * 64 * sizeof(ge_ext) + 16);
    off[6] = ap.add(nbatch * 64 * sizeof(ge_cached) + nbatch * sizeof(ge_ext) + 64);   // colq16 (128 B) or colc (160 B) per column, then hq
}
static void vb_bind(bpgpu_ctx *c, const size_t off[7], vb_dev &d) {
    char *a = c->arena;
    d.chunks = (vb_chunk *)(a + off[0]);
    d.chunk_first = (uint32_t *)(a + off[1]);
    d.term_chunk = (uint32_t *)(a + off[2]);
    d.recoded = (uint32_t *)(a + off[3]);
    d.tab = (ge_cached *)(a + off[4]);
    d.part = (ge_ext *)(a + off[5]);
    d.colq16 = (uint32_t *)(a + off[6]);
    d.hq = nullptr;   // set by vb_launch (behind colq16)
}
static int vb_launch(bpgpu_ctx *c, hipStream_t s, uint32_t total, uint32_t n_chunks, size_t nbatch, const uint32_t *d_scalars,
                     const uint32_t *d_points, uint32_t *d_status, vb_dev &d) {
    if (total) {
        LAUNCH(c, s, "vb_prepare", k_vb_prepare, (total + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, total, d.chunks, d.term_chunk, d_scalars,
               d_points, d.tab, d.recoded, d_status);
        const uint32_t nt = n_chunks * 64;
        LAUNCH(c, s, "vb_window", k_vb_window, (nt + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, nt, d.chunks, d.tab, d.recoded, d.part);
    }
    const uint32_t nc = (uint32_t)nbatch * 64;
    d.hq = (ge_ext *)(d.colq16 + (size_t)nbatch * 64 * 32);
    LAUNCH(c, s, "vb_colsum", k_vb_colsum, (nc + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, nc, d.chunk_first, d.part, d.colq16, (ge_cached *)nullptr);
    LAUNCH(c, s, "horner_wave", k_horner_wave, (uint32_t)nbatch, 64, d.colq16, d.hq);
    return BPGPU_OK;
}
// ragged plans: upload the decomposition into the arena every call
static int enqueue_vb(bpgpu_ctx *c, hipStream_t s, const vb_plan &pl, size_t nbatch, const size_t off[7],
                      const uint32_t *d_scalars, const uint32_t *d_points, uint32_t *d_status, vb_dev &d, bool upload_only = false) {
    vb_bind(c, off, d);
    // the plan is a local of the caller: stage it in pinned memory, which outlives the asynchronous copies
    const size_t b0 = pl.chunks.size() * sizeof(vb_chunk), b1 = (size_t)pl.total * 4, b2 = (nbatch + 1) * 4;
    char *h = nullptr;
    int rc = c->io.pin_alloc(align_up(b0) + align_up(b1) + align_up(b2), &h);
    if (rc) return rc;
    char *h0 = h, *h1 = h0 + align_up(b0), *h2 = h1 + align_up(b1);
    if (!pl.chunks.empty()) {
        memcpy(h0, pl.chunks.data(), b0);
        memcpy(h1, pl.term_chunk.data(), b1);
        HIPCHK(c, hipMemcpyAsync(d.chunks, h0, b0, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(d.term_chunk, h1, b1, hipMemcpyHostToDevice, s));
    }
    memcpy(h2, pl.chunk_first.data(), b2);
    HIPCHK(c, hipMemcpyAsync(d.chunk_first, h2, b2, hipMemcpyHostToDevice, s));
    if (upload_only) return BPGPU_OK;
    return vb_launch(c, s, pl.total, (uint32_t)pl.chunks.size(), nbatch, d_scalars, d_points, d_status, d);
}
// uniform plans (every MSM of the batch has `per` variable-base terms): decomposition cached on the device
// chunk: terms per (chunk, window) lane -- BP_VB_CHUNK, or fewer for narrow chains (rp_narrow_chunk): part of the cache key
static int uniform_plan(bpgpu_ctx *c, size_t nbatch, size_t per, bpgpu_ctx::plan_view *out, uint32_t chunk = BP_VB_CHUNK) {
    const size_t key = per | ((size_t)chunk << 40);
    auto it = c->plan_cache.find(key);
    if (it == c->plan_cache.end() || it->second.cap < nbatch) {
        if (it != c->plan_cache.end()) {   // outgrown: launches in flight may still read the old block
            c->plan_retired.push_back(it->second.mem);
            c->plan_cache.erase(it);
        } else if (c->plan_cache.size() >= 32) {   // bounded: retire the least recently used decomposition
            auto victim = c->plan_cache.begin();
            for (auto jt = c->plan_cache.begin(); jt != c->plan_cache.end(); ++jt)
                if (jt->second.last_use < victim->second.last_use) victim = jt;
            c->plan_retired.push_back(victim->second.mem);
            c->plan_cache.erase(victim);
        }
        if (c->plan_retired.size() > 64) {   // (only a caller that keeps changing its MSM sizes gets here)
            HIPCHK(c, hipDeviceSynchronize());
            for (char *q : c->plan_retired) hipFree(q);
            c->plan_retired.clear();
        }
        // capacity: a power of two >= nbatch; small per-MSM term counts (the range-proof path: 17 .. 60 points per proof) start at 1024
        // MSMs, large ones at what ~256 k terms allow (a lone 6 179-term MSM must not build the plan of a thousand of them)
        size_t cap = 1, floor_cap = per ? (size_t)262144 / per : 1024;
        if (floor_cap > 1024) floor_cap = 1024;
        while (cap < nbatch || cap < floor_cap) cap *= 2;
        std::vector<uint32_t> nt(cap, (uint32_t)per);
        vb_plan pl;
        make_vb_plan(pl, cap, nt.data(), chunk);
        bpgpu_ctx::plan_dev pd;
        pd.cap = cap;
        pd.o1 = align_up(pl.chunks.size() * sizeof(vb_chunk) + 16);
        pd.o2 = pd.o1 + align_up((cap + 1) * 4);
        const size_t tot = pd.o2 + align_up((size_t)pl.total * 4 + 16);
        HIPCHK(c, hipMalloc((void **)&pd.mem, tot));
        if (!pl.chunks.empty()) {
            HIPCHK(c, hipMemcpy(pd.mem, pl.chunks.data(), pl.chunks.size() * sizeof(vb_chunk), hipMemcpyHostToDevice));
            HIPCHK(c, hipMemcpy(pd.mem + pd.o2, pl.term_chunk.data(), (size_t)pl.total * 4, hipMemcpyHostToDevice));
        }
        HIPCHK(c, hipMemcpy(pd.mem + pd.o1, pl.chunk_first.data(), (cap + 1) * 4, hipMemcpyHostToDevice));
        it = c->plan_cache.emplace(key, pd).first;
    }
    it->second.last_use = ++c->plan_tick;
    out->mem = it->second.mem;
    out->o1 = it->second.o1;
    out->o2 = it->second.o2;
    out->n_chunks = nbatch * ((per + chunk - 1) / chunk);
    out->total = (uint32_t)(nbatch * per);
    return BPGPU_OK;
}
static void plan_vb_uniform(arena_plan &ap, size_t nbatch, size_t per, size_t off[7], size_t tab_entries = 8, size_t chunk = BP_VB_CHUNK) {
    const size_t n_chunks = nbatch * ((per + chunk - 1) / chunk), total = nbatch * per;
    off[0] = off[1] = off[2] = 0;   // decomposition lives in the plan cache
    off[3] = ap.add(total * 32 + 16);
    off[4] = ap.add(total * tab_entries * sizeof(ge_cached) + 16);
    off[5] = ap.add(n_chunks * 64 * sizeof(ge_ext) + 16);
    off[6] = ap.add(nbatch * 64 * sizeof(ge_cached) + nbatch * sizeof(ge_ext) + 64);   // colq16 (128 B) or colc (160 B) per column, then hq
}
static int enqueue_vb_uniform(bpgpu_ctx *c, hipStream_t s, size_t nbatch, size_t per, const size_t off[7], const uint32_t *d_scalars,
                              const uint32_t *d_points, uint32_t *d_status, vb_dev &d) {
    bpgpu_ctx::plan_view pv;
    int rc = uniform_plan(c, nbatch, per, &pv);
    if (rc) return rc;
    vb_bind(c, off, d);
    d.chunks = (vb_chunk *)pv.mem;
    d.chunk_first = (uint32_t *)(pv.mem + pv.o1);
    d.term_chunk = (uint32_t *)(pv.mem + pv.o2);
    return vb_launch(c, s, pv.total, (uint32_t)pv.n_chunks, nbatch, d_scalars, d_points, d_status, d);
}

// ============================================================================
// bucket (Pippenger) path for MSMs with many variable-base terms (bucket.h)
// ============================================================================
struct bk_dev {
    uint32_t *msm_first;   // [nmsm + 1]
    fb_entry *pts;         // [total] affine Niels records
    uint32_t *rwords;      // [total][BK_RWORDS]
    uint32_t *idx;         // [nwin][total]
    bk_desc *desc;         // [nmsm * nwin][half]
    ge_ext *bsum;          // [nmsm * nwin][half]
    ge_ext *gS, *gA;       // [nmsm * nwin][leaves]: bottom level of the running-sum tree
    uint32_t *gcnt, *gcur; // [nmsm * nwin][half]: global histogram / scatter cursors of the split sort (large MSMs)
    uint32_t *colq16;      // [nmsm][64][32 words]
    ge_ext *hq;            // [nmsm]
};
static uint32_t pick_bucket_c(size_t terms_per_msm) { return terms_per_msm >= 6000 ? 12u : 8u; }
static void plan_bucket(arena_plan &ap, size_t nmsm, size_t total, bk_params prm, size_t off[12]) {
    off[0] = ap.add((nmsm + 1) * 4);
    off[1] = ap.add(total * sizeof(fb_entry) + 16);
    off[2] = ap.add(total * BK_RWORDS * 4 + 16);
    off[3] = ap.add((size_t)prm.nwin * total * 4 + 16);
    off[4] = ap.add(nmsm * prm.nwin * prm.half * sizeof(bk_desc));
    off[5] = ap.add(nmsm * prm.nwin * prm.half * sizeof(ge_ext));
    off[6] = ap.add(nmsm * 64 * 128);
    off[7] = ap.add(nmsm * sizeof(ge_ext));
    off[8] = ap.add(nmsm * prm.nwin * bk_leaves(prm) * sizeof(ge_ext));
    off[9] = ap.add(nmsm * prm.nwin * bk_leaves(prm) * sizeof(ge_ext));
    off[10] = ap.add(nmsm * prm.nwin * prm.half * 4);
    off[11] = ap.add(nmsm * prm.nwin * prm.half * 4);
}
static void bucket_bind(bpgpu_ctx *c, const size_t off[12], bk_dev &d) {
    char *a = c->arena;
    d.msm_first = (uint32_t *)(a + off[0]);
    d.pts = (fb_entry *)(a + off[1]);
    d.rwords = (uint32_t *)(a + off[2]);
    d.idx = (uint32_t *)(a + off[3]);
    d.desc = (bk_desc *)(a + off[4]);
    d.bsum = (ge_ext *)(a + off[5]);
    d.colq16 = (uint32_t *)(a + off[6]);
    d.hq = (ge_ext *)(a + off[7]);
    d.gS = (ge_ext *)(a + off[8]);
    d.gA = (ge_ext *)(a + off[9]);
    d.gcnt = (uint32_t *)(a + off[10]);
    d.gcur = (uint32_t *)(a + off[11]);
}
// counting sort of the terms of every (MSM, window) by digit + population sort of the buckets.  Few thousand terms per
// MSM: one workgroup per (MSM, window), everything in LDS; more: the terms are shared by nsub workgroups (global
// histogram, one scan workgroup, scatter through global cursors).  per_msm: the largest term count of one MSM.
static int enqueue_bucket_sort(bpgpu_ctx *c, hipStream_t s, bk_params prm, uint32_t nmsm, uint32_t total, size_t per_msm, int single, bk_dev &d,
                               const uint32_t *skip_status, uint32_t skip_div) {
    const uint32_t nbw = nmsm * prm.nwin;
    if (per_msm < 32768) {
        if (prm.lanes == 64) LAUNCH(c, s, "bk_sort", k_bk_sort<64>, nbw, 64, prm, d.msm_first, total, single, d.rwords, d.idx, d.desc, skip_status, skip_div);
        else LAUNCH(c, s, "bk_sort", k_bk_sort<256>, nbw, 256, prm, d.msm_first, total, single, d.rwords, d.idx, d.desc, skip_status, skip_div);
        return BPGPU_OK;
    }
    uint32_t nsub = (uint32_t)((per_msm + 4095) / 4096);
    if (nsub > 128) nsub = 128;
    HIPCHK(c, hipMemsetAsync(d.gcnt, 0, (size_t)nbw * prm.half * 4, s));
    for (int phase = 0; phase < 3; phase++) {
        const uint32_t grid = phase == 1 ? nbw : nbw * nsub;
        if (prm.lanes == 64)
            LAUNCH(c, s, "bk_sort", k_bk_sort_big<64>, grid, 64, phase, nsub, prm, d.msm_first, total, single, d.rwords, d.idx, d.desc, d.gcnt, d.gcur, skip_status, skip_div);
        else
            LAUNCH(c, s, "bk_sort", k_bk_sort_big<256>, grid, 256, phase, nsub, prm, d.msm_first, total, single, d.rwords, d.idx, d.desc, d.gcnt, d.gcur, skip_status, skip_div);
    }
    return BPGPU_OK;
}
// bucket sums -> window sums (running-sum tree: wide leaf level, packed upper levels) -> column sums for the Horner chain
static void enqueue_bucket_reduce(bpgpu_ctx *c, hipStream_t s, bk_params prm, uint32_t nbw, bk_dev &d) {
    const uint32_t nl = nbw * bk_leaves(prm);
    LAUNCH(c, s, "bk_leaf", k_bk_leaf, (nl + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, nl, prm, d.bsum, d.gS, d.gA);
    if (prm.c == 8) LAUNCH(c, s, "bk_tree", k_bk_tree<8>, (nbw + 63) / 64, 64, prm, nbw, d.gS, d.gA, d.colq16);
    else LAUNCH(c, s, "bk_tree", k_bk_tree<12>, (nbw + 1) / 2, 64, prm, nbw, d.gS, d.gA, d.colq16);
}
// first-term offsets of the MSMs -> device (through pinned staging)
static int bucket_upload_first(bpgpu_ctx *c, hipStream_t s, size_t nmsm, const uint32_t *n_terms, size_t uniform_per, bk_dev &d) {
    char *h = nullptr;
    int rc = c->io.pin_alloc((nmsm + 1) * 4, &h);
    if (rc) return rc;
    uint32_t *f = (uint32_t *)h;
    uint32_t t0 = 0;
    for (size_t b = 0; b < nmsm; b++) {
        f[b] = t0;
        t0 += n_terms ? n_terms[b] : (uint32_t)uniform_per;
    }
    f[nmsm] = t0;
    HIPCHK(c, hipMemcpyAsync(d.msm_first, h, (nmsm + 1) * 4, hipMemcpyHostToDevice, s));
    return BPGPU_OK;
}
// sort -> bucket sums -> window sums -> Horner chain; leaves the MSM sums in d.hq
static int enqueue_bucket_tail(bpgpu_ctx *c, hipStream_t s, bk_params prm, size_t nmsm, size_t total, size_t per_msm, bk_dev &d) {
    const uint32_t nbw = (uint32_t)(nmsm * prm.nwin), tot32 = (uint32_t)total;
    int rcs = enqueue_bucket_sort(c, s, prm, (uint32_t)nmsm, tot32, per_msm, 0, d, nullptr, 0u);
    if (rcs) return rcs;
    const uint32_t nt = nbw * prm.half;
    const uint32_t lim = bk_chain_lim(per_msm, prm);
    LAUNCH(c, s, "bk_accum", k_bk_accum, (nt + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, nt, prm, tot32, d.desc, d.idx, d.pts, d.bsum, lim);
    const uint32_t hg = bk_heavy_groups(prm, nmsm);
    LAUNCH(c, s, "bk_heavy", k_bk_heavy, nbw * hg, 64, prm, tot32, (const bk_desc *)d.desc, (const uint32_t *)d.idx, (const fb_entry *)d.pts, d.bsum, lim, hg);
    enqueue_bucket_reduce(c, s, prm, nbw, d);
    LAUNCH(c, s, "horner_wave", k_horner_wave, (uint32_t)nmsm, 64, d.colq16, d.hq);
    return BPGPU_OK;
}
// ---- the fused chain (bucket2.h): c = 8, every MSM of the batch <= BK2_MAX_TERMS terms ----------------------------------------
static bool bucket2_applies(bpgpu_ctx *c, bk_params prm, size_t per_msm_max) { return c->bucket_chain == 0 && prm.c == BK2_C && per_msm_max <= BK2_MAX_TERMS; }
static void plan_bucket2(arena_plan &ap, size_t nmsm, size_t total, size_t off[12]) {
    const bk_params prm = bk_make(BK2_C);
    off[0] = ap.add((nmsm + 1) * 4);
    off[1] = ap.add(total * sizeof(fb_entry) + 16);
    off[2] = ap.add((size_t)BK2_NWIN * total + 16);   // digits, window-major (bk_dev::rwords)
    off[3] = off[4] = off[10] = off[11] = 0;          // no index lists, descriptors or global histograms
    off[5] = ap.add(nmsm * prm.nwin * prm.half * sizeof(ge_ext));
    off[6] = ap.add(nmsm * 64 * 128);
    off[7] = ap.add(nmsm * sizeof(ge_ext));
    off[8] = ap.add(nmsm * prm.nwin * BK2_FAST_LEAVES * sizeof(ge_ext));   // (8 leaves per window in a wide batch, 32 in a narrow one)
    off[9] = ap.add(nmsm * prm.nwin * BK2_FAST_LEAVES * sizeof(ge_ext));
}
// narrow chains end with the short-chain tail (bucket2.h: bk2_fast_v), wide batches with the one that executes fewer instructions
static bool bucket2_fast_tail(bpgpu_ctx *c, size_t nmsm) { return c->fast_tail < 0 ? nmsm < BK2_FAST_MAX_MSMS : c->fast_tail != 0; }
static uint32_t bucket2_lanes(bpgpu_ctx *c, size_t nmsm) {
    if (c->bucket_lanes) return (uint32_t)c->bucket_lanes;
    // a wide batch fills the device with one wavefront per (MSM, window) and keeps the runs long (2 081 terms: 33 additions per
    // lane, one head piece per lane); a lone MSM (32 workgroups in all) wants the shortest chain
    return nmsm >= 8 ? 64u : (nmsm >= 2 ? 128u : 256u);
}
// decode + digits -> window workgroups (sort in LDS + bucket sums) -> window sums -> Horner chain; leaves the MSM sums in d.hq
static int enqueue_bucket2(bpgpu_ctx *c, hipStream_t s, size_t nmsm, size_t total, size_t per_msm, const uint32_t *d_scalars, const uint32_t *d_points,
                           uint32_t *d_status, bk_dev &d) {
    const bk_params prm = bk_make(BK2_C);
    const uint32_t nbw = (uint32_t)(nmsm * prm.nwin), tot32 = (uint32_t)total;
    uint8_t *dig = (uint8_t *)d.rwords;
    LAUNCH(c, s, "bk_prepare", k_bk2_prepare, (tot32 + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, tot32, (uint32_t)nmsm, d.msm_first, d_scalars, d_points, d.pts, dig, d_status);
    const uint32_t lanes = bucket2_lanes(c, nmsm);
    const size_t shm = ((per_msm * 2 + 15) / 16) * 16;
    const int xcd_map = (nmsm % 8) == 0 ? 1 : 0;
    if (lanes == 64) LAUNCH_SHM(c, s, "bk_window", k_bk2_window<64>, nbw, 64, shm, (uint32_t)nmsm, xcd_map, d.msm_first, tot32, (const uint8_t *)dig, (const fb_entry *)d.pts, d.bsum);
    else if (lanes == 128) LAUNCH_SHM(c, s, "bk_window", k_bk2_window<128>, nbw, 128, shm, (uint32_t)nmsm, xcd_map, d.msm_first, tot32, (const uint8_t *)dig, (const fb_entry *)d.pts, d.bsum);
    else LAUNCH_SHM(c, s, "bk_window", k_bk2_window<256>, nbw, 256, shm, (uint32_t)nmsm, xcd_map, d.msm_first, tot32, (const uint8_t *)dig, (const fb_entry *)d.pts, d.bsum);
    if (bucket2_fast_tail(c, nmsm)) {
        const uint32_t nl = nbw * BK2_FAST_LEAVES;
        LAUNCH(c, s, "bk_leaf", k_bk2_leafv, (nl + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, nl, (const ge_ext *)d.bsum, d.gA);
    } else {
        const uint32_t nl = nbw * bk_leaves(prm);
        LAUNCH(c, s, "bk_leaf", k_bk_leaf, (nl + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, nl, prm, d.bsum, d.gS, d.gA);   // (the tree's upper level is the tail's first phase)
    }
    return BPGPU_OK;
}
// the generator half of a fused chain as ONE launch (msm_fixed.h: fb_walk_thread): partial sums -> partial[npart][nbatch]
static uint32_t fb_walk_parts(bpgpu_ctx *c, size_t nbatch, uint32_t n_gen_terms) {
    const uint32_t target = c->walk_waves ? (uint32_t)c->walk_waves : 2048u;   // (512 / 1024 / 2048 / 4096: 109 / 111 / 113 / 113 k MSMs/s, profiles/r06/cfg5_two_buffers_uncapped_and_walk_waves_ab.txt)
    if (nbatch < 32) {   // lane = slice of one MSM's generator terms: workgroups of one wavefront
        uint32_t nwg = (uint32_t)((target + nbatch - 1) / nbatch);
        const uint32_t most = (n_gen_terms + 63) / 64;
        if (nwg > most) nwg = most;
        return nwg ? nwg : 1;
    }
    const uint32_t nblk_p = (uint32_t)((nbatch + 63) / 64);
    uint32_t per = (uint32_t)(((uint64_t)n_gen_terms * nblk_p + target - 1) / target);   // generator terms per wavefront
    if (per == 0) per = 1;
    const uint32_t nslice = (n_gen_terms + per - 1) / per;
    return (nslice + 3) / 4;
}
static void enqueue_fb_walk(bpgpu_ctx *c, hipStream_t s, fb_params prm, size_t nbatch, uint32_t n_gen_terms, uint32_t nwg, const uint32_t *d_gen_scalars, const uint32_t *d_ids,
                            ge_ext *d_partial, uint32_t *d_status) {
    if (nbatch < 32) {
        LAUNCH(c, s, "fb_walk", k_fb_walk1, (uint32_t)(nwg * nbatch), 64, prm, (uint32_t)nbatch, nwg, n_gen_terms, d_gen_scalars, d_ids, (const fb_entry *)c->d_table, d_partial, d_status);
    } else {
        const uint32_t nblk_p = (uint32_t)((nbatch + 63) / 64);
        LAUNCH(c, s, "fb_walk", k_fb_walk<4>, nwg * nblk_p, 256, prm, (uint32_t)nbatch, nblk_p, nwg, n_gen_terms, d_gen_scalars, d_ids, (const fb_entry *)c->d_table, d_partial, d_status);
    }
}
static bool bucket_fits(size_t nmsm, size_t total, bk_params prm) {
    return (uint64_t)nmsm * prm.nwin * prm.half <= 0x7fffffffull && (uint64_t)total * prm.nwin <= 0x7fffffffull;
}

static int msm_batch_dev_locked(bpgpu_ctx *c, size_t nbatch, const uint32_t *n_terms, const void *d_scalars, const void *d_points,
                                void *d_out, void *d_status_bytes, hipStream_t s) {
    if (nbatch == 0) return BPGPU_OK;
    {   // many terms per MSM: bucket path (bucket.h); otherwise the table-lookup path below
        uint64_t total = 0;
        for (size_t b = 0; b < nbatch; b++) total += n_terms[b];
        const bk_params prm = bk_make(pick_bucket_c(total / nbatch));
        if (total / nbatch >= (c->bucket_min ? c->bucket_min : BK_MIN_TERMS) && bucket_fits(nbatch, total, prm)) {
            size_t per_msm = 0;
            for (size_t b = 0; b < nbatch; b++) per_msm = n_terms[b] > per_msm ? n_terms[b] : per_msm;
            const bool fused = bucket2_applies(c, prm, per_msm);
            arena_plan ap;
            size_t off[12];
            if (fused) plan_bucket2(ap, nbatch, total, off);
            else plan_bucket(ap, nbatch, total, prm, off);
            const size_t off_status = ap.add(nbatch * 4);
            int rc = arena_reserve(c, ap.total);
            if (rc) return rc;
            bk_dev d;
            bucket_bind(c, off, d);
            uint32_t *d_status = (uint32_t *)(c->arena + off_status);
            HIPCHK(c, hipMemsetAsync(d_status, 0, nbatch * 4, s));
            rc = bucket_upload_first(c, s, nbatch, n_terms, 0, d);
            if (rc) return rc;
            if (fused) {
                rc = enqueue_bucket2(c, s, nbatch, total, per_msm, (const uint32_t *)d_scalars, (const uint32_t *)d_points, d_status, d);
            } else {
                LAUNCH(c, s, "bk_prepare", k_bk_prepare, ((uint32_t)total + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, (uint32_t)total, (uint32_t)nbatch, d.msm_first,
                       (const uint32_t *)d_scalars, (const uint32_t *)d_points, d.pts, d.rwords, d_status, prm);
                rc = enqueue_bucket_tail(c, s, prm, nbatch, total, per_msm, d);
            }
            if (rc) return rc;
            if (fused) {
                if (bucket2_fast_tail(c, nbatch))
                    LAUNCH(c, s, "msm_tail", k_msm_tail_fast, (uint32_t)nbatch, 256, (uint32_t)nbatch, 1, (const ge_ext *)d.gA, 0u, (const ge_ext *)nullptr,
                           (const uint32_t *)d_status, (uint32_t *)d_out, (uint8_t *)nullptr, (uint8_t *)d_status_bytes);
                else
                    LAUNCH(c, s, "msm_tail", k_msm_tail, (uint32_t)nbatch, 64, (uint32_t)nbatch, 1, (const ge_ext *)d.gS, (const ge_ext *)d.gA, 0u, (const ge_ext *)nullptr,
                           (const uint32_t *)d_status, (uint32_t *)d_out, (uint8_t *)nullptr, (uint8_t *)d_status_bytes);
            } else {
                LAUNCH(c, s, "vb_horner", k_vb_horner, ((uint32_t)nbatch + 63) / 64, 64, (uint32_t)nbatch, d.hq, d_status, (uint32_t *)d_out);
                LAUNCH(c, s, "status_bytes", k_status_bytes, ((uint32_t)nbatch + 63) / 64, 64, (uint32_t)nbatch, d_status, (uint8_t *)d_status_bytes);
            }
            HIPCHK(c, hipGetLastError());
            return BPGPU_OK;
        }
    }
    // a few small MSMs (the boundary function called from one thread: nothing else to fill the device with): the narrow form -- second
    // tables, chunks of ~sqrt(N) terms, one tail launch (k_msm.hip: k_vb_prepare_hi / k_vb_window_hi / k_vb_tail_narrow)
    uint64_t tot_terms = 0, max_terms = 0;
    for (size_t b = 0; b < nbatch; b++) {
        tot_terms += n_terms[b];
        if (n_terms[b] > max_terms) max_terms = n_terms[b];
    }
    const bool narrow = c->msm_narrow && nbatch <= 16 && tot_terms > 0 && tot_terms <= 768;   // (same-box A/B, profiles/r06/msm_narrow_ab.txt: 29 / 147 / 542 terms 0.44 / 0.475 / 0.52 -> 0.33 / 0.38 / 0.465 ms per blocking call; 1024 terms 0.56 -> 0.59: the wavefront-per-term role then needs a second round)
    uint32_t chunk = BP_VB_CHUNK;
    if (narrow) {
        chunk = 4;
        while ((uint64_t)chunk * chunk < max_terms && chunk < BP_VB_CHUNK) chunk++;
    }
    vb_plan pl;
    make_vb_plan(pl, nbatch, n_terms, chunk);
    arena_plan ap;
    size_t off[7];
    const uint32_t lev = narrow ? 2u : 1u;   // (four table levels -- a 16-window chain, as the narrowest range-proof chains take -- were measured here: no gain,
                                             // profiles/r06/msm_narrow_four_levels_ab.txt: this call's long pole is its first launch, not the chain)
    plan_vb(ap, pl, nbatch, off, 8 * lev);
    const size_t off_status = ap.add(nbatch * 4);
    int rc = arena_reserve(c, ap.total);
    if (rc) return rc;
    uint32_t *d_status = (uint32_t *)(c->arena + off_status);
    HIPCHK(c, hipMemsetAsync(d_status, 0, nbatch * 4, s));
    vb_dev d;
    if (narrow) {
        rc = enqueue_vb(c, s, pl, nbatch, off, (const uint32_t *)d_scalars, (const uint32_t *)d_points, d_status, d, true);
        if (rc) return rc;
        const uint32_t total = pl.total, n_lb = (total + BP_BLOCK - 1) / BP_BLOCK, nt = (uint32_t)pl.chunks.size() * 64;
        ge_cached *tab_hi = d.tab + (size_t)8 * total;
        LAUNCH(c, s, "vb_prepare", k_vb_prepare_hi, n_lb + (lev - 1) * total, BP_BLOCK, total, n_lb, d.chunks, d.term_chunk, (const uint32_t *)d_scalars, (const uint32_t *)d_points,
               d.tab, d.recoded, d_status, tab_hi, lev);
        LAUNCH(c, s, "vb_window", k_vb_window_hi, (nt + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, nt, d.chunks, d.tab, d.recoded, d.part, (const ge_cached *)tab_hi, lev, total);
        LAUNCH(c, s, "vb_tail", k_vb_tail_narrow, (uint32_t)nbatch, 64, (uint32_t)nbatch, d.chunk_first, d.part, (const uint32_t *)d_status, (uint32_t *)d_out,
               (uint8_t *)d_status_bytes, lev);
        HIPCHK(c, hipGetLastError());
        return BPGPU_OK;
    }
    rc = enqueue_vb(c, s, pl, nbatch, off, (const uint32_t *)d_scalars, (const uint32_t *)d_points, d_status, d);
    if (rc) return rc;
    LAUNCH(c, s, "vb_horner", k_vb_horner, ((uint32_t)nbatch + 63) / 64, 64, (uint32_t)nbatch, d.hq, d_status, (uint32_t *)d_out);
    LAUNCH(c, s, "status_bytes", k_status_bytes, ((uint32_t)nbatch + 63) / 64, 64, (uint32_t)nbatch, d_status, (uint8_t *)d_status_bytes);
    HIPCHK(c, hipGetLastError());
    return BPGPU_OK;
}

extern "C" int bpgpu_msm_batch_dev(bpgpu_ctx *c, size_t nbatch, const uint32_t *n_terms, const void *d_scalars, const void *d_points,
                                   void *d_out, void *d_status, void *stream) {
    if (!c || (nbatch && (!n_terms || !d_out || !d_status))) return BPGPU_ERR_INVALID_ARG;
    return dev_call(
        c, stream,
        [&] {
            uint64_t total = 0;
            for (size_t b = 0; b < nbatch; b++) total += n_terms[b];
            if (nbatch > 0x7fffffffu / 64 || total > 0x7fffffffu / 64) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large");
            return BPGPU_OK;
        },
        [&](hipStream_t s) { return msm_batch_dev_locked(c, nbatch, n_terms, d_scalars, d_points, d_out, d_status, s); });
}

extern "C" int bpgpu_msm_batch(bpgpu_ctx *c, size_t nbatch, const uint32_t *n_terms, const uint8_t *scalars, const uint8_t *points,
                               uint8_t *out, uint8_t *status) {
    if (!c || (nbatch && (!n_terms || !out || !status))) return BPGPU_ERR_INVALID_ARG;
    if (nbatch == 0) return BPGPU_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t total = 0;
    for (size_t b = 0; b < nbatch; b++) total += n_terms[b];
    if (total && (!scalars || !points)) return BPGPU_ERR_INVALID_ARG;
    if (nbatch > 0x7fffffffu / 64 || total > 0x7fffffffu / 64) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large");
    // persistent device IO buffer + pinned staging: no allocation in steady state, one wait at the end
    hipStream_t s = c->stream;
    host_call<bpgpu_ctx> io(c, s);
    const int r_s = io.in(total * 32 + 16), r_p = io.in(total * 32 + 16), r_o = io.out(nbatch * 32), r_st = io.out(nbatch);
    int rc = io.open();
    if (rc) return rc;
    if (total) {
        io.put(r_s, scalars, total * 32);
        io.put(r_p, points, total * 32);
        rc = io.upload();
    }
    if (!rc) rc = msm_batch_dev_locked(c, nbatch, n_terms, io.d(r_s), io.d(r_p), io.d(r_o), io.d(r_st), s);
    rc = io.finish(io.download(rc));
    if (rc) return rc;
    memcpy(out, io.h(r_o), nbatch * 32);
    memcpy(status, io.h(r_st), nbatch);
    return BPGPU_OK;
}

// ============================================================================
// shared-generator MSM
// ============================================================================
// (fixed: option fixed_splits; hint / busy_hint: what the pool said about this chain -- bpgpu_ctx::splits, splits_hint, busy_hint)
static uint32_t pick_splits(uint32_t fixed, uint32_t hint, int busy_hint, size_t nbatch, uint32_t npairs, bool walk_alone_in_launch = false) {
    if (fixed) return fixed;
    if (hint && npairs <= 8192) {   // the pool knows how much else is in flight (pool.hip flush_dev)
        uint32_t s = hint;
        while (s > 8 && npairs / s < 8) s -= 8;
        return s;
    }
    // >= 1024 wavefronts (one per SIMD).  A lone table walk runs 1.45x faster with 4096 (4 per SIMD hide its VALU
    // dependency stalls: 4.0 ms at 2048 wavefronts vs 2.8 ms at 4096, batch 16384), but it shares its launch with the
    // longer Horner role, and with several batches in flight the device is work-bound: every split costs one
    // more point addition per proof in the reduction (measured at 48 x 1024: 256 splits 4.35 M/s, 128: 4.5, 64:
    // 4.57, 32: 4.45) and with <= 64 partial sums the finish kernel needs no separate reduction launch.
    // Aggregated shapes (thousands of generator terms per proof, e.g. m = 16: 38950 pairs) are all table walk:
    // they keep the 4096-wavefront target (cfg3: 478 k/s vs 443 k/s).
    // A wide chain whose Horner chains run aside (rp_chain_forms) has the walk alone in launch 4 and nobody told it how much else is in
    // flight (a context on its own, >= 8192 proofs): two full rounds of three wavefronts per SIMD (a lone 16 384-proof chain ran its walk at 0.59 of the mixed-addition rate
    // with 2048 wavefronts, profiles/r03/chain16384_alone_kernel_stats.csv).
    const uint32_t nblk = (uint32_t)((nbatch + FB_BLOCK - 1) / FB_BLOCK);
    const bool lone = walk_alone_in_launch && busy_hint < 0;   // (a pool that said "busy" has other chains to fill the device)
    const uint32_t target = npairs > 8192 ? 4096 : (lone ? 6144 : 1024);
    uint32_t s = (target + nblk - 1) / nblk;
    s = (s + 7) & ~7u;
    if (lone && s > 64) s = 64;   // (more would need a reduction launch in front of the finish)
    while (s > 8 && npairs / s < 8) s -= 8;
    if (s < 8) s = 8;
    return s;
}
static uint32_t pick_splits(bpgpu_ctx *c, size_t nbatch, uint32_t npairs) { return pick_splits(c->splits, c->splits_hint, c->busy_hint, nbatch, npairs); }

// Tree-reduce the per-split partial points (8-way per level) until at most `until` remain per proof.
// `buf` must hold nsplit*nbatch + ceil(nsplit/8)*nbatch (+ ...) points: callers reserve 2*nsplit*nbatch.
#define FB_REDUCE_GROUP 8
static void enqueue_fb_reduce(bpgpu_ctx *c, hipStream_t s, uint32_t nbatch, uint32_t nsplit, ge_ext *buf, ge_ext **out, uint32_t *nout,
                              uint32_t until = FB_REDUCE_GROUP) {
    ge_ext *cur = buf;
    uint32_t n = nsplit;
    ge_ext *next = buf + (size_t)nsplit * nbatch;
    while (n > until) {
        const uint32_t ng = (n + FB_REDUCE_GROUP - 1) / FB_REDUCE_GROUP;
        const uint32_t nt = ng * nbatch;
        LAUNCH(c, s, "fb_reduce", k_fb_reduce, (nt + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, nt, nbatch, n, (uint32_t)FB_REDUCE_GROUP, cur, next);
        cur = next;
        next = next + (size_t)ng * nbatch;
        n = ng;
    }
    *out = cur;
    *nout = n;
}

static int msm_shared_dev_locked(bpgpu_ctx *c, size_t n, size_t m, size_t nbatch, size_t n_unique, const void *d_gen_scalars,
                                 const void *d_uniq_scalars, const void *d_uniq_points, void *d_out, void *d_status_bytes,
                                 void *d_verdict, hipStream_t s, bool g_only = false, bool ct = false) {
    // ct: the constant-time walk (generator terms only: n_unique == 0) -- the prover's V, A, S, T_1, T_2
    if (nbatch == 0) return BPGPU_OK;
    if (!c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    if (ct) {
        if (n_unique) return fail(c, BPGPU_ERR_INVALID_ARG, "the constant-time path serves generator terms only");
        const int rcc = build_ct_table(c);
        if (rcc) return rcc;
    }
    if (n == 0 || m == 0 || n > c->gens_capacity || m > c->party_capacity)
        return fail(c, BPGPU_ERR_NO_GENS, "generators too small for n=%zu m=%zu", n, m);
    const uint32_t n_gen_terms = (uint32_t)((g_only ? 1 : 2) * n * m + 2);   // g_only: d_gen_scalars rows are (B_blinding, B, G(n, m))
    const fb_params prm = ct ? c->prm_ct : c->prm;
    const uint32_t npairs = n_gen_terms * prm.nwin;
    // thread / element counts are 32-bit in the kernels: refuse what does not fit (grids of <= 2^31 / 64 blocks)
    if ((uint64_t)n_gen_terms * nbatch > 0x7fffffffull || (uint64_t)nbatch * ((n_unique + BP_VB_CHUNK - 1) / BP_VB_CHUNK) * 64 > 0x7fffffffull ||
        (uint64_t)nbatch * n_unique > 0x7fffffffull / 64)
        return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large for this shape");
    uint32_t *d_ids = nullptr;
    int rc = gen_ids_for(c, n, m, &d_ids, g_only);
    if (rc) return rc;
    const uint32_t nsplit = pick_splits(c, nbatch, npairs);
    const bk_params bkp = bk_make(pick_bucket_c(n_unique));
    const bool use_bucket = n_unique >= (c->bucket_min ? c->bucket_min : BK_MIN_TERMS) && bucket_fits(nbatch, nbatch * n_unique, bkp);
    arena_plan ap;
    size_t off[7], boff[12];
    const bool fused = use_bucket && !ct && bucket2_applies(c, bkp, n_unique);
    if (fused) plan_bucket2(ap, nbatch, nbatch * n_unique, boff);
    else if (use_bucket) plan_bucket(ap, nbatch, nbatch * n_unique, bkp, boff);
    // a few MSMs with a few points of their own (the mega-check of ONE proof as the caller's own MSM call: 130 generator terms + 17 points): the
    // narrow form -- second tables, ~sqrt chunks, the generator half as one launch with the recoding in registers, one tail launch
    const bool narrow_sh = c->msm_narrow && !ct && !use_bucket && n_unique > 0 && nbatch <= 16 && nbatch * n_unique <= 768;
    uint32_t sh_chunk = BP_VB_CHUNK;
    if (narrow_sh) {
        sh_chunk = 4;
        while ((size_t)sh_chunk * sh_chunk < n_unique && sh_chunk < BP_VB_CHUNK) sh_chunk++;
    }
    const uint32_t sh_lev = narrow_sh ? 2u : 1u;
    if (!fused && !use_bucket) plan_vb_uniform(ap, nbatch, n_unique, off, 8 * sh_lev, sh_chunk);
    const size_t off_status = ap.add(nbatch * 4);
    if (narrow_sh) {
        const uint32_t nwg = fb_walk_parts(c, nbatch, n_gen_terms);
        const size_t off_part = ap.add((size_t)nwg * nbatch * sizeof(ge_ext) + 16);
        rc = arena_reserve(c, ap.total);
        if (rc) return rc;
        uint32_t *d_status = (uint32_t *)(c->arena + off_status);
        ge_ext *d_part = (ge_ext *)(c->arena + off_part);
        HIPCHK(c, hipMemsetAsync(d_status, 0, nbatch * 4, s));
        hipStream_t s2 = c->msm_fork ? c->stream2 : s;
        if (s2 != s) {
            HIPCHK(c, hipEventRecord(c->fork_ev, s));
            HIPCHK(c, hipStreamWaitEvent(s2, c->fork_ev, 0));
        }
        enqueue_fb_walk(c, s2, prm, nbatch, n_gen_terms, nwg, (const uint32_t *)d_gen_scalars, d_ids, d_part, d_status);
        if (s2 != s) HIPCHK(c, hipEventRecord(c->join_ev, s2));
        bpgpu_ctx::plan_view pv;
        rc = uniform_plan(c, nbatch, n_unique, &pv, sh_chunk);
        if (rc) return rc;
        vb_dev d{};
        vb_bind(c, off, d);
        d.chunks = (vb_chunk *)pv.mem;
        d.chunk_first = (uint32_t *)(pv.mem + pv.o1);
        d.term_chunk = (uint32_t *)(pv.mem + pv.o2);
        const uint32_t total = pv.total, n_lb = (total + BP_BLOCK - 1) / BP_BLOCK, nt = (uint32_t)pv.n_chunks * 64;
        ge_cached *tab_hi = d.tab + (size_t)8 * total;
        LAUNCH(c, s, "vb_prepare", k_vb_prepare_hi, n_lb + (sh_lev - 1) * total, BP_BLOCK, total, n_lb, d.chunks, d.term_chunk, (const uint32_t *)d_uniq_scalars,
               (const uint32_t *)d_uniq_points, d.tab, d.recoded, d_status, tab_hi, sh_lev);
        LAUNCH(c, s, "vb_window", k_vb_window_hi, (nt + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, nt, d.chunks, d.tab, d.recoded, d.part, (const ge_cached *)tab_hi, sh_lev, total);
        if (s2 != s) HIPCHK(c, hipStreamWaitEvent(s, c->join_ev, 0));
        LAUNCH(c, s, "msm_tail", k_shared_tail_narrow, (uint32_t)nbatch, 128, (uint32_t)nbatch, d.chunk_first, d.part, nwg, (const ge_ext *)d_part,
               (const uint32_t *)d_status, (uint32_t *)d_out, (uint8_t *)d_verdict, (uint8_t *)d_status_bytes, sh_lev);
        HIPCHK(c, hipGetLastError());
        return BPGPU_OK;
    }
    if (fused) {   // the fused chain: generator half = one launch, tail = one launch (bucket2.h)
        const uint32_t nwg = fb_walk_parts(c, nbatch, n_gen_terms);
        const size_t off_part = ap.add((size_t)nwg * nbatch * sizeof(ge_ext) + 16);
        rc = arena_reserve(c, ap.total);
        if (rc) return rc;
        uint32_t *d_status = (uint32_t *)(c->arena + off_status);
        ge_ext *d_part = (ge_ext *)(c->arena + off_part);
        HIPCHK(c, hipMemsetAsync(d_status, 0, nbatch * 4, s));
        hipStream_t s2 = c->msm_fork ? c->stream2 : s;
        if (s2 != s) {
            HIPCHK(c, hipEventRecord(c->fork_ev, s));
            HIPCHK(c, hipStreamWaitEvent(s2, c->fork_ev, 0));
        }
        enqueue_fb_walk(c, s2, prm, nbatch, n_gen_terms, nwg, (const uint32_t *)d_gen_scalars, d_ids, d_part, d_status);
        if (s2 != s) HIPCHK(c, hipEventRecord(c->join_ev, s2));
        bk_dev bd;
        bucket_bind(c, boff, bd);
        rc = bucket_upload_first(c, s, nbatch, nullptr, n_unique, bd);
        if (rc) return rc;
        rc = enqueue_bucket2(c, s, nbatch, nbatch * n_unique, n_unique, (const uint32_t *)d_uniq_scalars, (const uint32_t *)d_uniq_points, d_status, bd);
        if (rc) return rc;
        if (s2 != s) HIPCHK(c, hipStreamWaitEvent(s, c->join_ev, 0));
        if (bucket2_fast_tail(c, nbatch))
            LAUNCH(c, s, "msm_tail", k_msm_tail_fast, (uint32_t)nbatch, 256, (uint32_t)nbatch, 1, (const ge_ext *)bd.gA, nwg, (const ge_ext *)d_part,
                   (const uint32_t *)d_status, (uint32_t *)d_out, (uint8_t *)d_verdict, (uint8_t *)d_status_bytes);
        else
            LAUNCH(c, s, "msm_tail", k_msm_tail, (uint32_t)nbatch, 64, (uint32_t)nbatch, 1, (const ge_ext *)bd.gS, (const ge_ext *)bd.gA, nwg, (const ge_ext *)d_part,
                   (const uint32_t *)d_status, (uint32_t *)d_out, (uint8_t *)d_verdict, (uint8_t *)d_status_bytes);
        HIPCHK(c, hipGetLastError());
        return BPGPU_OK;
    }
    const size_t off_digits = ap.add((size_t)npairs * nbatch * sizeof(fb_digit) + 16);
    const size_t off_partial = ap.add((size_t)2 * nsplit * nbatch * sizeof(ge_ext) + 16);
    rc = arena_reserve(c, ap.total);
    if (rc) return rc;
    uint32_t *d_status = (uint32_t *)(c->arena + off_status);
    fb_digit *d_digits = (fb_digit *)(c->arena + off_digits);
    ge_ext *d_partial = (ge_ext *)(c->arena + off_partial);
    HIPCHK(c, hipMemsetAsync(d_status, 0, nbatch * 4, s));
    // the generator-table half (recode, walk, partial reduction) on the context's second stream, beside the per-MSM points
    hipStream_t s2 = (n_unique && c->msm_fork) ? c->stream2 : s;
    if (s2 != s) {
        HIPCHK(c, hipEventRecord(c->fork_ev, s));
        HIPCHK(c, hipStreamWaitEvent(s2, c->fork_ev, 0));
    }
    const uint32_t nrec = n_gen_terms * (uint32_t)nbatch;
    const uint32_t nblk_p = (uint32_t)((nbatch + FB_BLOCK - 1) / FB_BLOCK);
    if (ct) {
        LAUNCH(c, s2, "fb_recode_ct", k_fb_recode_ct, (nrec + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, nrec, prm, (uint32_t)nbatch, n_gen_terms,
               (const uint32_t *)d_gen_scalars, d_digits);
        LAUNCH(c, s2, "fb_accum_ct", k_fb_accum_ct, nblk_p * nsplit, FB_BLOCK, prm, (uint32_t)nbatch, nblk_p, nsplit, npairs, d_ids, d_digits,
               c->d_table_ct, d_partial);
    } else {
        LAUNCH(c, s2, "fb_recode", k_fb_recode, (nrec + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, nrec, prm, (uint32_t)nbatch, n_gen_terms,
               (const uint32_t *)d_gen_scalars, d_digits, d_status);
        LAUNCH(c, s2, "fb_accum", k_fb_accum, nblk_p * nsplit, FB_BLOCK, prm, (uint32_t)nbatch, nblk_p, nsplit, npairs, d_ids, d_digits,
               c->d_table, d_partial);
    }
    ge_ext *d_red = nullptr;
    uint32_t nred = 0;
    enqueue_fb_reduce(c, s2, (uint32_t)nbatch, nsplit, d_partial, &d_red, &nred);
    if (s2 != s) HIPCHK(c, hipEventRecord(c->join_ev, s2));
    vb_dev d{};
    if (use_bucket) {   // many per-MSM points (the R1CS verifier's shape, r1cs/verifier.rs:459-491): bucket path
        bk_dev bd;
        bucket_bind(c, boff, bd);
        rc = bucket_upload_first(c, s, nbatch, nullptr, n_unique, bd);
        if (rc) return rc;
        const uint32_t total = (uint32_t)(nbatch * n_unique);   // (the fused chain left above: this is bucket.h's)
        LAUNCH(c, s, "bk_prepare", k_bk_prepare, (total + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, total, (uint32_t)nbatch, bd.msm_first,
               (const uint32_t *)d_uniq_scalars, (const uint32_t *)d_uniq_points, bd.pts, bd.rwords, d_status, bkp);
        rc = enqueue_bucket_tail(c, s, bkp, nbatch, total, n_unique, bd);
        if (rc) return rc;
        d.hq = bd.hq;
    } else if (n_unique) {
        rc = enqueue_vb_uniform(c, s, nbatch, n_unique, off, (const uint32_t *)d_uniq_scalars, (const uint32_t *)d_uniq_points, d_status, d);
        if (rc) return rc;
    }
    if (s2 != s) HIPCHK(c, hipStreamWaitEvent(s, c->join_ev, 0));
    LAUNCH(c, s, "shared_finish", k_shared_finish, ((uint32_t)nbatch + 63) / 64, 64, (uint32_t)nbatch, nred, d.hq, n_unique ? 1 : 0,
           d_red, d_status, (uint32_t *)d_out, (uint8_t *)d_verdict, (uint8_t *)d_status_bytes);   // (status bytes ride along: one launch fewer)
    HIPCHK(c, hipGetLastError());
    return BPGPU_OK;
}

extern "C" int bpgpu_msm_batch_shared_dev(bpgpu_ctx *c, size_t n, size_t m, size_t nbatch, size_t n_unique, const void *d_gen_scalars,
                                          const void *d_uniq_scalars, const void *d_uniq_points, void *d_out, void *d_status,
                                          void *stream) {
    if (!c || (nbatch && (!d_gen_scalars || !d_out || !d_status))) return BPGPU_ERR_INVALID_ARG;
    if (n_unique && (!d_uniq_scalars || !d_uniq_points)) return BPGPU_ERR_INVALID_ARG;
    return dev_call(c, stream, [&](hipStream_t s) {
        return msm_shared_dev_locked(c, n, m, nbatch, n_unique, d_gen_scalars, d_uniq_scalars, d_uniq_points, d_out, d_status, nullptr, s);
    });
}

extern "C" int bpgpu_msm_batch_shared(bpgpu_ctx *c, size_t n, size_t m, size_t nbatch, size_t n_unique, const uint8_t *gen_scalars,
                                      const uint8_t *uniq_scalars, const uint8_t *uniq_points, uint8_t *out, uint8_t *status) {
    if (!c || (nbatch && (!gen_scalars || !out || !status))) return BPGPU_ERR_INVALID_ARG;
    if (n_unique && (!uniq_scalars || !uniq_points)) return BPGPU_ERR_INVALID_ARG;
    if (nbatch == 0) return BPGPU_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t ng = (2 * n * m + 2) * nbatch * 32, nu = n_unique * nbatch * 32;
    hipStream_t s = c->stream;
    host_call<bpgpu_ctx> io(c, s);
    const int r_g = io.in(ng + 16), r_us = io.in(nu + 16), r_up = io.in(nu + 16), r_o = io.out(nbatch * 32), r_st = io.out(nbatch);
    int rc = io.open();
    if (rc) return rc;
    io.put(r_g, gen_scalars, ng);
    if (nu) {
        io.put(r_us, uniq_scalars, nu);
        io.put(r_up, uniq_points, nu);
    }
    rc = io.upload();
    if (!rc) rc = msm_shared_dev_locked(c, n, m, nbatch, n_unique, io.d(r_g), io.d(r_us), io.d(r_up), io.d(r_o), io.d(r_st), nullptr, s);
    rc = io.finish(io.download(rc));
    if (rc) return rc;
    memcpy(out, io.h(r_o), nbatch * 32);
    memcpy(status, io.h(r_st), nbatch);
    return BPGPU_OK;
}

// ============================================================================
// generator derivation on the device (BulletproofGens::new, PedersenGens::default)
// ============================================================================
static void host_shake_chain(std::vector<uint8_t> &out, uint8_t tag, uint32_t party, size_t count) {
    // GeneratorsChain::new(label): SHAKE256("GeneratorsChain" || tag || u32le(party))  (generators.rs:64-72,186-201)
    uint32_t w[50];
    kstate st;
    st.w = w;
    st.stride = 1;
    sponge k;
    sponge_init(k, st, BP_SHAKE256_RATE);
    const uint8_t dom[15] = {'G', 'e', 'n', 'e', 'r', 'a', 't', 'o', 'r', 's', 'C', 'h', 'a', 'i', 'n'};
    const uint8_t label[5] = {tag, (uint8_t)party, (uint8_t)(party >> 8), (uint8_t)(party >> 16), (uint8_t)(party >> 24)};
    sponge_absorb(k, dom, 15);
    sponge_absorb(k, label, 5);
    sponge_finish(k, 0x1f);
    const size_t off = out.size();
    out.resize(off + 64 * count);
    sponge_squeeze(k, out.data() + off, (uint32_t)(64 * count));
}

static const uint8_t BASEPOINT_COMPRESSED[32] = {0xe2, 0xf2, 0xae, 0x0a, 0x6a, 0xbc, 0x4e, 0x71, 0xa8, 0x84, 0xa9,
                                                 0x61, 0xc5, 0x00, 0x51, 0x5f, 0x58, 0xe3, 0x0b, 0x6a, 0xa5, 0x82,
                                                 0xdd, 0x8d, 0xb6, 0xa6, 0x59, 0x45, 0xe0, 0x8d, 0x2d, 0x76};

extern "C" int bpgpu_gens_create(bpgpu_ctx *c, size_t gens_capacity, size_t party_capacity) {
    if (!c || gens_capacity == 0 || party_capacity == 0) return BPGPU_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t tot = gens_capacity * party_capacity;
    // uniform bytes: [B_blinding seed][G party 0..][H party 0..]
    std::vector<uint8_t> uni;
    {
        uint32_t w[50];
        kstate st;
        st.w = w;
        st.stride = 1;
        sponge k;
        sponge_init(k, st, BP_SHA3_512_RATE);   // hash_from_bytes::<Sha3_512>(compress(B))  (generators.rs:48)
        sponge_absorb(k, BASEPOINT_COMPRESSED, 32);
        sponge_finish(k, 0x06);
        uni.resize(64);
        sponge_squeeze(k, uni.data(), 64);
    }
    for (size_t p = 0; p < party_capacity; p++) host_shake_chain(uni, 'G', (uint32_t)p, gens_capacity);
    for (size_t p = 0; p < party_capacity; p++) host_shake_chain(uni, 'H', (uint32_t)p, gens_capacity);
    const uint32_t cnt = (uint32_t)(1 + 2 * tot);
    uint32_t *d_uni = nullptr, *d_out = nullptr;
    HIPCHK(c, hipMalloc((void **)&d_uni, uni.size()));
    HIPCHK(c, hipMalloc((void **)&d_out, (size_t)cnt * 32));
    HIPCHK(c, hipMemcpyAsync(d_uni, uni.data(), uni.size(), hipMemcpyHostToDevice, c->stream));
    LAUNCH(c, c->stream, "from_uniform", k_from_uniform, (cnt + 63) / 64, 64, cnt, d_uni, d_out);
    std::vector<uint8_t> enc((size_t)cnt * 32);
    HIPCHK(c, hipMemcpyAsync(enc.data(), d_out, enc.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hipFree(d_uni);
    hipFree(d_out);
    return load_gens_locked(c, gens_capacity, party_capacity, enc.data() + 32, enc.data() + 32 + tot * 32, BASEPOINT_COMPRESSED,
                            enc.data());
}

// ============================================================================
// range-proof verification
// ============================================================================

// ---- Merlin transcripts on the host (Transcript::new / append_message / challenge_bytes on the 208-byte state) ----
static void ts_to_strobe(strobe &t, uint32_t w[50], const uint8_t *state) {
    memcpy(w, state, 200);
    t.st.w = w;
    t.st.stride = 1;
    t.pos = state[200];
    t.pos_begin = state[201];
    t.cur_flags = state[202];
}
static void ts_from_strobe(uint8_t *state, const strobe &t) {
    memset(state, 0, BPGPU_TRANSCRIPT_BYTES);
    memcpy(state, t.st.w, 200);
    state[200] = (uint8_t)t.pos;
    state[201] = (uint8_t)t.pos_begin;
    state[202] = (uint8_t)t.cur_flags;
}
static bool ts_state_ok(const uint8_t *state) { return state[200] < BP_STROBE_R && state[201] <= BP_STROBE_R; }
static const uint8_t DOM_SEP[7] = {'d', 'o', 'm', '-', 's', 'e', 'p'};

extern "C" int bpgpu_transcript_new(const uint8_t *label, size_t label_len, uint8_t state[BPGPU_TRANSCRIPT_BYTES]) {
    if (!state || (label_len && !label) || label_len > 0xffffffffu) return BPGPU_ERR_INVALID_ARG;
    uint32_t w[50];
    kstate st;
    st.w = w;
    st.stride = 1;
    strobe t;
    merlin_strobe_init(t, st);
    merlin_append_message(t, DOM_SEP, 7, label, (uint32_t)label_len);   // Transcript::new: append_message(b"dom-sep", label)
    ts_from_strobe(state, t);
    return BPGPU_OK;
}
extern "C" int bpgpu_transcript_append_message(uint8_t state[BPGPU_TRANSCRIPT_BYTES], const uint8_t *label, size_t label_len,
                                               const uint8_t *msg, size_t msg_len) {
    if (!state || (label_len && !label) || (msg_len && !msg) || label_len > 0xffffffffu || msg_len > 0xffffffffu || !ts_state_ok(state))
        return BPGPU_ERR_INVALID_ARG;
    uint32_t w[50];
    strobe t;
    ts_to_strobe(t, w, state);
    merlin_append_message(t, label, (uint32_t)label_len, msg, (uint32_t)msg_len);
    ts_from_strobe(state, t);
    return BPGPU_OK;
}
extern "C" int bpgpu_transcript_challenge_bytes(uint8_t state[BPGPU_TRANSCRIPT_BYTES], const uint8_t *label, size_t label_len,
                                                uint8_t *out, size_t out_len) {
    if (!state || (label_len && !label) || (out_len && !out) || label_len > 0xffffffffu || out_len > 0xffffffffu || !ts_state_ok(state))
        return BPGPU_ERR_INVALID_ARG;
    uint32_t w[50];
    strobe t;
    ts_to_strobe(t, w, state);
    merlin_challenge_bytes(t, label, (uint32_t)label_len, out, (uint32_t)out_len);
    ts_from_strobe(state, t);
    return BPGPU_OK;
}

// thread_rng() stand-in of the provers and of everything else that needs host-side random bytes: a per-thread ChaCha20 generator
// keyed and re-keyed from the OS CSPRNG (hostrng.h).  (The verification chains need 32 bytes each: rp_shape::seed.)
static int os_random(bpgpu_ctx *c, char *dst, size_t bytes) {
    if (!bp::fast_random((uint8_t *)dst, bytes)) return fail(c, BPGPU_ERR_HIP, "getrandom failed");
    return BPGPU_OK;
}
// the caller's transcript, not yet domain-separated: the kernel applies rangeproof_domain_sep(n, m) per proof
static void strobe_init_from_state(rp_strobe_init &init, const uint8_t *state) {
    memcpy(init.w, state, 200);
    init.pos = state[200];
    init.pos_begin = state[201];
    init.cur_flags = state[202];
}

static void make_strobe_init(rp_strobe_init &init, const uint8_t *label, size_t label_len, uint64_t n, uint64_t m) {
    // Transcript::new(label) followed by rangeproof_domain_sep(n, m) (transcript.rs:44-48): identical for
    // every proof of the batch, so it is replayed once here and the kernel starts from this state
    kstate st;
    st.w = init.w;
    st.stride = 1;
    strobe t;
    merlin_strobe_init(t, st);
    const uint8_t dom[7] = {'d', 'o', 'm', '-', 's', 'e', 'p'};
    const uint8_t rp[13] = {'r', 'a', 'n', 'g', 'e', 'p', 'r', 'o', 'o', 'f', ' ', 'v', '1'};
    const uint8_t ln[1] = {'n'}, lm[1] = {'m'};
    merlin_append_message(t, dom, 7, label, (uint32_t)label_len);
    merlin_append_message(t, dom, 7, rp, 13);
    merlin_append_u64(t, ln, 1, n);
    merlin_append_u64(t, lm, 1, m);
    init.pos = t.pos;
    init.pos_begin = t.pos_begin;
    init.cur_flags = t.cur_flags;
}

// the transcript script of a shape and start position (rp_script.h), cached on the device per context.
// The cache is bounded (callers whose transcripts sit at many different STROBE positions): beyond 64 entries the least recently
// used one gives its device block to the newcomer.  Uploads come from the pinned staging buffer on the call's stream, so the
// overwrite is ordered behind every earlier launch of this context that read the old script (ctx_enter orders the streams);
// nothing is freed and nothing synchronises the device while other lanes are running.
static int script_for(bpgpu_ctx *c, hipStream_t s, uint32_t n, uint32_t m, uint32_t k, const rp_strobe_init &init, bool domsep, const rp_script_hdr **out) {
    std::vector<uint32_t> key = {n, m, k, init.pos, init.pos_begin, init.cur_flags, domsep ? 1u : 0u};
    auto it = c->script_cache.find(key);
    if (it == c->script_cache.end()) {
        const std::vector<uint32_t> img = rp_script_build(n, m, k, init.pos, init.pos_begin, init.cur_flags, domsep);
        const size_t bytes = img.size() * 4;
        bpgpu_ctx::script_ent ent;
        if (c->script_cache.size() >= 64) {
            auto lru = c->script_cache.begin();
            for (auto jt = c->script_cache.begin(); jt != c->script_cache.end(); ++jt)
                if (jt->second.last_use < lru->second.last_use) lru = jt;
            ent = lru->second;
            c->script_cache.erase(lru);
            if (ent.cap < bytes) {   // too small for the newcomer: parked until the context goes away (a few KB; bounded by the shapes a process uses)
                c->script_retired.push_back(ent.mem);
                ent.mem = nullptr;
                ent.cap = 0;
            }
        }
        if (!ent.mem) {
            const size_t cap = bytes < 8192 ? 8192 : bytes;
            HIPCHK(c, hipMalloc((void **)&ent.mem, cap));
            ent.cap = cap;
        }
        char *h = nullptr;
        const int rc = c->io.pin_alloc(bytes, &h);
        if (rc) {
            c->script_retired.push_back(ent.mem);
            return rc;
        }
        memcpy(h, img.data(), bytes);
        HIPCHK(c, hipMemcpyAsync(ent.mem, h, bytes, hipMemcpyHostToDevice, s));
        it = c->script_cache.emplace(key, ent).first;
    }
    it->second.last_use = ++c->script_tick;
    *out = (const rp_script_hdr *)it->second.mem;
    return BPGPU_OK;
}

// Where a call's transcripts start: Transcript::new(label) (label), or one caller-supplied state for the whole batch
// (shared_ts, host, 208 bytes), or one state per proof (d_ts_in, device); d_ts_out (optional): the advanced states.
struct rp_transcripts {
    const uint8_t *label = nullptr;
    size_t label_len = 0;
    const uint8_t *shared_ts = nullptr;
    const void *d_ts_in = nullptr;
    void *d_ts_out = nullptr;
    // with d_ts_in: every state of the batch sits at this STROBE position (the pool's combining queue groups its requests that
    // way), so the per-shape script replaces the byte-wise replay although the sponge words differ from proof to proof
    bool ts_uniform = false;
    uint32_t u_pos = 0, u_pos_begin = 0, u_flags = 0;
    // coalesced launches (h_segs): the label of every item, all `label_len` bytes long (`label` is item 0's).  Items whose labels differ
    // start from their own state (rp_seg::init_w); positions depend on lengths only, so the chain's script serves them all
    const uint8_t *const *seg_labels = nullptr;
};

// ---- the forms a per-proof launch chain takes -----------------------------------------------------------------------------------
// One decision table for what used to be scattered conditions.  Inputs: the context options (0 / -1 = automatic), what the pool
// said about the chain (busy_hint: 1 = other chains run beside it, 0 = it is alone on the device, -1 = nobody said), its width.
//   WIDE     (>= 2048 proofs, or split_stage3 = 1): the window sums are a launch of their own -- their register allocation instead of
//            the generator-exponent role's 252 (+1.5 ... 3 %, profiles/r03/ab_split_stage3.txt).
//   WAVE     one wavefront per Horner chain (horner_wave.h): a small batch alone is a latency matter -- up to 256 proofs always (one call
//            0.85 -> 0.62 ms), up to 2304 when the pool knows the chain is alone (one host call of 1024 / 2048 / 4096 proofs, slices of
//            <= 2048: 1.37 / 2.14 / 2.84 M/s against 1.12 / 1.93 / 2.66 with quads; at 6144, slices of 3072, quads are ahead again).
//   ASIDE    one LANE per Horner chain, as its own launch on the context's second stream right after the window sums (half the quad
//            form's instructions, twice its latency: 0.76 ms that need other work beside them).  Wide chains when other chains run beside
//            them, or from 8192 proofs on a context nobody told anything: +2.6 ... 3.6 % steady state, +2 ... 4.6 % on 20 x 1024 bursts;
//            a lone host call of 2048 / 4096 proofs loses 22 / 16 % with it (profiles/r03/ab_horner_one_lane.txt, host_call_horner_forms.txt).
//   RADIX32  with ASIDE only, option per_proof_radix = 32: 16-entry tables, 51 windows (+1 % steady, -4.5 % bursts: off by default).
//   A_OUTSIDE with ASIDE only: A, whose coefficient is 1, is added after the chain instead of going through a table and 64 windows.
// Otherwise: four lanes per Horner chain inside launch 4 (horner_quad.h).  Batch-combined calls and shape verdicts take none of these.
enum { RPC_WIDE = 1, RPC_WAVE = 2, RPC_ASIDE = 4, RPC_RADIX32 = 8, RPC_A_OUTSIDE = 16 };
static uint32_t rp_chain_forms(uint32_t horner_lanes, int split_stage3, int busy_hint, uint32_t per_proof_radix, int a_outside, size_t nbatch,
                               bool combined_or_verdict_only, bool on_second_stream) {
    const bool wide = !combined_or_verdict_only && (split_stage3 == 1 || (split_stage3 < 0 && nbatch >= 2048));
    const bool throughput = busy_hint > 0 || (busy_hint < 0 && nbatch >= 8192);
    const bool wave = horner_lanes == 64 || (horner_lanes == 0 && (nbatch <= 256 || (busy_hint == 0 && nbatch <= 2304)));
    const bool aside = wide && !wave && !on_second_stream && (horner_lanes == 1 || (horner_lanes == 0 && throughput));
    uint32_t f = 0;
    if (wide) f |= RPC_WIDE;
    if (wave) f |= RPC_WAVE;
    if (aside) f |= RPC_ASIDE;
    if (aside && per_proof_radix == 32) f |= RPC_RADIX32;
    if (aside && a_outside) f |= RPC_A_OUTSIDE;
    return f;
}
// (for tests/test_abi_and_host.py: the table is plain host logic)
extern "C" uint32_t bpgpu_internal_chain_forms(int64_t horner_lanes, int64_t split_stage3, int64_t busy_hint, int64_t per_proof_radix, int64_t a_outside,
                                               uint64_t nbatch, int combined_or_verdict_only, int on_second_stream) {
    return rp_chain_forms((uint32_t)horner_lanes, (int)split_stage3, (int)busy_hint, (uint32_t)per_proof_radix, (int)a_outside, (size_t)nbatch,
                          combined_or_verdict_only != 0, on_second_stream != 0);
}

// (tests: pin the key the library would draw for a chain's device-expanded randomness, so that a call WITHOUT rng / weight buffers can be
// compared with one that passes the expansion's bytes explicitly; key = nullptr: back to the generator)
extern "C" int bpgpu_internal_set_chain_seed(bpgpu_ctx *c, const uint8_t *key32) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    c->test_seed_set = key32 != nullptr;
    if (key32) memcpy(c->test_seed, key32, 32);
    return BPGPU_OK;
}

// ---- what a proof length and a shape are, before any arithmetic -------------------------------------------------------------------------
// The length-only part of RangeProof::from_bytes / InnerProductProof::from_bytes (mod.rs:505-510, ipp.rs:374-388) -- one verdict for the whole
// batch --, then the parameter checks of verify_multiple_with_rng in the reference's order (mod.rs:358-366: Bitsize, GeneratorsLength; ipp.rs:209:
// n m == 2^k), reported per proof AFTER its own format check.  The one copy of these rules: the chain driver, the pool's "can these share a
// chain" and the mixed check's grouping all ask here.
struct rp_class {
    uint32_t all_verdict = 0;     // BPGPU_VERDICT_FORMAT_ERROR: every proof of the batch has the same malformed length
    uint32_t shape_verdict = 0;   // else: the code of every proof that passes its own format check (0: a shape to verify)
    size_t k = 0;                 // lg(n m) as the length has it (all_verdict == 0)
    bool unsupported = false;     // a shape to verify with k > BP_RP_MAX_K
};
static rp_class rp_classify(size_t n, size_t m, size_t proof_len, size_t gens_capacity, size_t party_capacity) {
    rp_class r;
    const size_t ne = proof_len / 32;   // 32-byte elements: A, S, T_1, T_2, t_x, t_x_blinding, e_blinding, k pairs (L, R), a, b
    if (proof_len % 32 != 0 || ne < 9 || (ne - 9) % 2 != 0 || (ne - 9) / 2 >= 32) {
        r.all_verdict = BPGPU_VERDICT_FORMAT_ERROR;
        return r;
    }
    r.k = (ne - 9) / 2;
    if (!(n == 8 || n == 16 || n == 32 || n == 64)) r.shape_verdict = BPGPU_VERDICT_INVALID_BITSIZE;
    else if (gens_capacity < n || party_capacity < m) r.shape_verdict = BPGPU_VERDICT_INVALID_GENERATORS_LENGTH;
    else if (m == 0 || n * m != ((size_t)1 << r.k)) r.shape_verdict = BPGPU_VERDICT_VERIFICATION_ERROR;   // ipp.rs:209
    else r.unsupported = r.k > BP_RP_MAX_K;
    return r;
}

// ---- the plan of a launch chain ------------------------------------------------------------------------------------------------------------
// Everything that is decided about a chain before its first launch, each thing once: the forms it takes (rp_chain_forms above is the first step;
// the narrow-chain forms follow it), the splits of the table walk, the chunk size of the window sums, every grid count, every arena offset and
// the arena's size.  Plain host logic -- its inputs are a snapshot of the context's options and hints, the shape and its class, the parameters of
// the window table the generator terms walk, and the facts of the call; it makes no HIP call and sees no context, so it is checked rule by rule
// on the CPU (bpgpu_internal_chain_plan below, tests/test_abi_and_host.py).
#define RP_NARROW_MAX 256   // proofs: up to here a chain is NARROW, a latency matter -- 32 lanes per proof in launch 1, one generator index per lane,
                            // small chunks of window sums under a wavefront per Horner chain, the walk with lane = split
struct rp_plan_opts {       // what a plan reads of a context (rp_plan_opts_of)
    uint32_t splits, splits_hint, horner_lanes, vb_radix, bucket_min;
    int busy_hint, a_outside, split_stage3, narrow_walk, narrow_hi_max, narrow_hi4_max, narrow_chunk, narrow_fused_finish, transcript_coop, coop_split,
        coop_defer_emit, exp_single, exp_pairs, exp_w3_min_nm, no_script;
};
static rp_plan_opts rp_plan_opts_of(const bpgpu_ctx *c) {
    return {c->splits, c->splits_hint, c->horner_lanes, c->vb_radix, c->bucket_min, c->busy_hint, c->a_outside, c->split_stage3, c->narrow_walk,
            c->narrow_hi_max, c->narrow_hi4_max, c->narrow_chunk, c->narrow_fused_finish, c->transcript_coop, c->coop_split, c->coop_defer_emit,
            c->exp_single, c->exp_pairs, c->exp_w3_min_nm, c->no_script ? 1 : 0};
}
struct rp_call_facts {
    size_t nbatch = 0;
    bool rlc = false;             // the batch-combined check
    bool ts_per_proof = false;    // one caller transcript per proof ...
    bool ts_uniform = false;      // ... all of them at one STROBE position
    bool want_out = false;        // someone wants the mega-check encodings (combined: the 33-byte result)
    bool second_stream = false;   // the call came on the context's second stream
    uint32_t nseg = 0;            // coalesced: items ...
    uint32_t nlabels = 0;         // ... and the distinct labels among them
};
enum { RP_EXP_FOUR = 0, RP_EXP_PAIRS = 1, RP_EXP_SINGLE = 2 };   // generator indices per lane of the exponent role: four, eight in mirrored pairs, one
struct rp_chain_plan {
    const char *refused = nullptr;   // the chain cannot be enqueued: why
    rp_shape sh;                     // as the kernels get it (radix5, a_outside, defer_emit, coop_split, narrow_hi decided here; the seed is the driver's)
    uint32_t lg_m, n_gen_terms, npairs;
    uint32_t forms;                  // rp_chain_forms
    bool wide, wave, aside, r5, a_out;
    bool scripted;                   // the per-shape transcript script replaces the byte-wise replay
    bool coop;                       // launch 1 with 32 lanes per proof
    bool narrow_walk;                // launch 4: lane = split, a proof's partial sums folded in the launch
    bool hi;                         // second (hi_levels = 2) or second to fourth (4) tables per point, a 32- / 16-window Horner chain
    uint32_t hi_levels;
    bool narrow_ok;                  // narrow chains of this context and mode take the wavefront-per-chain form, with small chunks
    uint32_t narrow_q, vb_chunk_sz;  // points per (chunk, window) lane: of those chains, of this one
    bool rlc_bucket;                 // combined check: ONE bucket MSM over all proofs' weighted terms
    bk_params bkp;
    size_t rlc_terms;
    bool quad, one_lane, one_chunk;  // Horner chains on four lanes / on one inside launch 4; U <= chunk: window sums are column sums
    uint32_t exp_form;               // RP_EXP_*
    bool exp_w3;                     // wide: the paired exponent launch at three wavefronts per SIMD
    bool fused_finish, finish1;      // no finish launch / lane = proof (else eight lanes per proof)
    uint32_t nsplit, nsplit1, nparts;   // splits of the walk, of the combined check's one-MSM walk; partial sums per proof that launch 4 leaves
    size_t n_chunks;
    // grids (workgroups) and the thread counts behind them
    uint32_t n_tr, n_pt, g_stage1, nexp, n_exp, nwin, n_win, nrows, n_rows, nwsum, g_wsum, g_colsum, n_sc, nblk_p, n_hw, g_stage4, walk_flags, g_finish;
    // arena
    size_t off[7], boff[12], off_digits, off_partial, off_fields, off_mv, off_segs, off_inits, off_acc, off_tree, off_dig1, off_part1, off_res1;
    size_t arena_need;               // this chain's
    size_t arena_reserve;            // ... and what a lane that will see chains of every width up to this one reserves
};
static void rp_plan_chain(rp_chain_plan &p, const rp_plan_opts &o, const rp_class &cl, size_t n, size_t m, size_t proof_len, const fb_params &prm,
                          const rp_call_facts &f) {
    const size_t nbatch = f.nbatch;
    const uint32_t nb32 = (uint32_t)nbatch;
    const bool rlc = f.rlc, verdict_only = cl.shape_verdict != 0, narrow = nbatch <= RP_NARROW_MAX;
    rp_shape &sh = p.sh;
    sh.n = (uint32_t)n;
    sh.m = (uint32_t)m;
    sh.nm = (uint32_t)(n * m);
    sh.k = (uint32_t)cl.k;
    sh.U = (uint32_t)(4 + 2 * cl.k + m);
    sh.proof_len = (uint32_t)proof_len;
    sh.nproofs = nb32;
    sh.shape_verdict = cl.shape_verdict;
    p.lg_m = 0;
    while (((size_t)1 << p.lg_m) < m) p.lg_m++;
    p.n_gen_terms = verdict_only ? 2 : (uint32_t)(2 * n * m + 2);
    p.npairs = p.n_gen_terms * prm.nwin;
    // ---- forms: the table above, then what narrow chains add to it
    p.forms = rp_chain_forms(o.horner_lanes, o.split_stage3, o.busy_hint, o.vb_radix, o.a_outside, nbatch, rlc || verdict_only, f.second_stream);
    p.wide = p.forms & RPC_WIDE, p.wave = p.forms & RPC_WAVE, p.aside = p.forms & RPC_ASIDE, p.r5 = p.forms & RPC_RADIX32, p.a_out = p.forms & RPC_A_OUTSIDE;
    p.scripted = (!f.ts_per_proof || f.ts_uniform) && !verdict_only && !o.no_script;   // every proof starts at one STROBE position
    p.coop = p.scripted && o.transcript_coop && narrow;
    sh.coop_split = (p.coop && o.coop_split && !rlc && !p.wide && !verdict_only && sh.k < 32) ? 1u : 0u;   // (launch 3 then carries the basepoint-coefficient role)
    // the walk with lane = split, a multiple of 64 splits per proof (rp_walk_narrow)
    p.narrow_walk = p.wave && !p.wide && !rlc && !verdict_only && narrow && o.narrow_walk;
    // ... and for VERY narrow ones every per-proof point gets a second table, of its 2^128 multiple, built beside the transcript by a wavefront of its own
    // (k_rp_stage1_coop's third role): the Horner chain has 32 windows, and the walk twice the splits to end with it; the very narrowest: three more
    // tables per point, a 16-window chain
    p.hi = p.narrow_walk && sh.coop_split && (int64_t)nbatch <= (int64_t)o.narrow_hi_max;
    p.hi_levels = !p.hi ? 1u : ((int64_t)nbatch <= (int64_t)o.narrow_hi4_max ? 4u : 2u);
    sh.narrow_hi = p.hi ? p.hi_levels : 0u;
    sh.radix5 = p.r5 ? 1u : 0u;
    sh.a_outside = p.a_out ? 1u : 0u;
    sh.defer_emit = o.coop_defer_emit ? 1u : 0u;
    p.nsplit = pick_splits(o.splits, o.splits_hint, o.busy_hint, nbatch, p.npairs, p.aside);
    if (p.narrow_walk) {
        if (p.hi && p.nsplit < 2 * FB_BLOCK) p.nsplit = 2 * FB_BLOCK;
        if (p.hi_levels == 4 && p.nsplit < 4 * FB_BLOCK) p.nsplit = 4 * FB_BLOCK;
        p.nsplit = (p.nsplit + FB_BLOCK - 1) / FB_BLOCK * FB_BLOCK;
        while (p.nsplit > FB_BLOCK && p.npairs / p.nsplit < 4) p.nsplit -= FB_BLOCK;
    }
    p.nsplit1 = rlc ? pick_splits(o.splits, o.splits_hint, o.busy_hint, 1, p.npairs) : 0;   // the combined check ends in a walk for ONE MSM
    p.nparts = p.narrow_walk ? p.nsplit / FB_BLOCK : p.nsplit;
    // thread / element counts are 32-bit in the kernels: refuse what does not fit
    if ((uint64_t)p.n_gen_terms * nbatch > 0x7fffffffull || (uint64_t)nbatch * sh.U > 0x7fffffffull / 64 ||
        (uint64_t)nbatch * ((sh.U + BP_VB_CHUNK - 1) / BP_VB_CHUNK) * 64 > 0x7fffffffull || (uint64_t)(sh.nm / 4 + 1) * nbatch > 0x7fffffffull ||
        (uint64_t)((nbatch + FB_BLOCK - 1) / FB_BLOCK) * p.nsplit > 0x7fffffffull) {
        p.refused = "batch too large for this shape";
        return;
    }
    // batch combination with enough per-proof terms: ONE bucket MSM (bucket.h) over all proofs' weighted terms
    p.rlc_terms = (size_t)nbatch * sh.U;
    p.bkp = bk_make(pick_bucket_c(p.rlc_terms));
    p.rlc_bucket = rlc && !verdict_only && p.rlc_terms >= (o.bucket_min ? o.bucket_min : BK_RLC_MIN_TERMS) && bucket_fits(1, p.rlc_terms, p.bkp);
    // Narrow chains (one wavefront per Horner chain, which adds the chunks' window sums itself): a (chunk, window) lane adding all U table
    // entries one after the other is ~50 us of a one-proof chain's launch 3.  With chunks of 8 terms a lane adds 8 entries and the Horner
    // wavefront's lane w adds the U / 8 rows of its window.  (Option narrow_chunk.)
    p.narrow_q = (uint32_t)o.narrow_chunk;
    if (p.narrow_q == 0) p.narrow_q = 8;   // (A/B at U = 17, profiles/r06/narrow_chain_ab.txt: 3 / 5 / 8 / 32 -> one call 0.456 / 0.457 / 0.448 / 0.464 ms; launch 3 is then bound by its basepoint-coefficient role)
    p.narrow_q = p.narrow_q < 2 ? 2u : (p.narrow_q > BP_VB_CHUNK ? (uint32_t)BP_VB_CHUNK : p.narrow_q);
    p.narrow_ok = !rlc && !verdict_only && (o.horner_lanes == 0 || o.horner_lanes == 64);
    p.vb_chunk_sz = (p.wave && !p.wide && p.narrow_ok && narrow) ? p.narrow_q : (uint32_t)BP_VB_CHUNK;
    p.n_chunks = (verdict_only || p.rlc_bucket) ? 0 : nbatch * ((sh.U + p.vb_chunk_sz - 1) / p.vb_chunk_sz);   // (as uniform_plan cuts them)
    p.one_chunk = p.n_chunks == nbatch;
    // Horner layout: quads (16 chains per wavefront, least total work) unless the chain takes the wavefront-per-chain form (lowest latency of a small
    // batch); with horner_lanes = 1 one lane per chain in the quads' place
    p.quad = !p.wave;
    p.one_lane = o.horner_lanes == 1;
    // the generator-exponent role: one index per lane for narrow chains (latency), eight in mirrored pairs otherwise (rp_expand_b8_thread: least work)
    const bool exp_single = !rlc && !p.wide && o.exp_single && narrow && sh.nm >= 4;
    const bool pairs = !rlc && !exp_single && o.exp_pairs && sh.nm >= 8;
    p.exp_form = exp_single ? RP_EXP_SINGLE : (pairs ? RP_EXP_PAIRS : RP_EXP_FOUR);
    p.exp_w3 = p.wide && pairs && sh.nm >= (uint32_t)o.exp_w3_min_nm;   // (aggregated shapes: three wavefronts per SIMD)
    // verdicts only (the crate's own call: nobody asks for the mega-check's encoding) and at most four partial sums per proof: the LAST of a proof's
    // 1 + nsplit / 64 workgroups of launch 4 to arrive adds them to the Horner result and writes the verdict -- no finish launch (option narrow_fused_finish)
    // (same-box A/B, profiles/r06/fused_finish_ab.txt: 64 threads +5 %, 256 threads +3 %, tickets and 16 threads unchanged, ONE proof per chain -2.5 % -- the
    // finisher's three additions then follow the Horner wavefront instead of overlapping with the launch of the next kernel: chains of >= 8 proofs only)
    p.fused_finish = p.narrow_walk && o.narrow_fused_finish && nbatch >= 8 && !f.want_out && p.nparts <= 4;
    uint32_t nred = p.nparts;   // (what enqueue_fb_reduce leaves: 8 lanes x <= 8 partials each in finish8)
    while (nred > 64) nred = (nred + FB_REDUCE_GROUP - 1) / FB_REDUCE_GROUP;
    p.finish1 = nred <= 2 && p.narrow_walk;   // one or two partial sums + the Horner result per proof: lane = proof (more: eight lanes per proof and a three-level fold)
    // ---- grids
    p.n_tr = p.coop ? (nb32 + 1) / 2 : (nb32 + RP_BLOCK - 1) / RP_BLOCK;   // 32 lanes per proof: two proofs per workgroup
    p.n_pt = verdict_only ? 0 : (nb32 * sh.U + RP_BLOCK - 1) / RP_BLOCK;
    p.g_stage1 = p.n_tr + p.n_pt + ((p.coop && p.hi) ? (p.hi_levels - 1) * nb32 * sh.U : 0u);
    p.nexp = (exp_single ? sh.nm : sh.nm / (pairs ? 8 : 4)) * nb32;   // four generator indices per lane (eight in pairs)
    p.nwin = (uint32_t)p.n_chunks * 64;
    p.n_win = (p.nwin + BP_BLOCK - 1) / BP_BLOCK, p.n_exp = (p.nexp + BP_BLOCK - 1) / BP_BLOCK;
    p.nrows = sh.coop_split ? nb32 : 0u, p.n_rows = (p.nrows + BP_BLOCK - 1) / BP_BLOCK;
    p.nwsum = p.r5 ? nb32 * BP_VB5_WINDOWS : (p.a_out ? nb32 * BP_VB_WINDOWS : p.nwin);   // wide: the window sums as their own launch
    p.g_wsum = (p.nwsum + BP_BLOCK - 1) / BP_BLOCK;
    p.g_colsum = (nb32 * 64 + BP_BLOCK - 1) / BP_BLOCK;
    p.n_sc = (p.n_gen_terms + BP_BLOCK - 1) / BP_BLOCK;
    p.nblk_p = (nb32 + FB_BLOCK - 1) / FB_BLOCK;
    p.n_hw = p.aside ? 0u : (p.quad ? (p.one_lane ? p.nblk_p : (nb32 + 15) / 16) : nb32);   // launch 4's Horner role: elsewhere, a lane, four lanes, a wavefront per chain
    p.g_stage4 = p.n_hw + ((p.narrow_walk && !p.quad) ? nb32 * p.nparts : p.nblk_p * p.nsplit);
    p.walk_flags = (p.narrow_walk && !p.quad) ? ((p.hi ? (p.hi_levels == 4 ? 9u : 3u) : 1u) | (p.fused_finish ? 4u : 0u)) : 0u;
    p.g_finish = p.finish1 ? (nb32 + 63) / 64 : (nb32 + 7) / 8;
    // ---- arena
    arena_plan ap;
    const rp_fields fl = rp_field_layout(sh.k, sh.m);
    if (p.rlc_bucket) plan_bucket(ap, 1, p.rlc_terms, p.bkp, p.boff);
    else plan_vb_uniform(ap, nbatch, verdict_only ? 0 : sh.U, p.off, p.hi ? 8 * p.hi_levels : (p.r5 ? 16 : 8), p.vb_chunk_sz);
    p.off_digits = ap.add((size_t)p.npairs * nbatch * sizeof(fb_digit) + 16);
    p.off_partial = ap.add((size_t)2 * p.nsplit * nbatch * sizeof(ge_ext) + 16);
    p.off_fields = ap.add((size_t)fl.count * nbatch * BP_RP_REC * 4 + 16);
    p.off_mv = ap.add(nbatch);
    p.off_segs = f.nseg > RP_SEG_INLINE ? ap.add((size_t)f.nseg * sizeof(rp_seg)) : 0;
    p.off_inits = f.nlabels > 1 ? ap.add((size_t)f.nlabels * 256) : 0;   // items whose labels differ start from their own states
    // batch-combination mode: coefficient accumulators, the column-sum reduction tree, and a batch-of-one table walk (digits, partial sums, result)
    const size_t n_rows0 = verdict_only ? 0 : nbatch * ((sh.U + BP_VB_CHUNK - 1) / BP_VB_CHUNK);
    p.off_acc = rlc ? ap.add((size_t)p.n_gen_terms * 10 * 8) : 0;
    p.off_tree = rlc ? ap.add((n_rows0 / 8 + 64) * 64 * sizeof(ge_ext)) : 0;
    p.off_dig1 = rlc ? ap.add((size_t)p.npairs * sizeof(fb_digit) + 16) : 0;
    p.off_part1 = rlc ? ap.add((size_t)2 * p.nsplit1 * sizeof(ge_ext) + 16) : 0;
    p.off_res1 = rlc ? ap.add(sizeof(ge_ext) + 64) : 0;   // Horner result, then 8 result words, verdict byte, chunk bounds
    p.arena_need = ap.total;
    // (a lane sized for wide chains also sees narrow ones, whose window sums come in more, smaller chunks)
    p.arena_reserve = p.arena_need + ((p.narrow_ok && !narrow) ? (size_t)RP_NARROW_MAX * ((sh.U + p.narrow_q - 1) / p.narrow_q) * 64 * sizeof(ge_ext) : 0);
}
// (for tests/test_abi_and_host.py: the classifier and the plan are plain host logic.  opt: the fields of rp_plan_opts in their order; fact: nbatch, rlc,
// ts_per_proof, ts_uniform, want_out, second_stream, nseg, nlabels.  out, when the shape is one to plan: [4 ..) as listed below; returns the count written)
extern "C" int bpgpu_internal_chain_plan(const int64_t *opt, uint64_t n, uint64_t m, uint64_t proof_len, uint64_t gens_capacity, uint64_t party_capacity,
                                         uint32_t window_bits, const int64_t *fact, uint64_t *out, uint32_t n_out) {
    if (!opt || !fact || !out || n_out < 32 || window_bits < 1) return -1;
    const rp_class cl = rp_classify(n, m, proof_len, gens_capacity, party_capacity);
    out[0] = cl.all_verdict, out[1] = cl.shape_verdict, out[2] = cl.k, out[3] = cl.unsupported;
    if (cl.all_verdict || cl.unsupported || fact[0] <= 0) return 4;
    const rp_plan_opts o = {(uint32_t)opt[0], (uint32_t)opt[1], (uint32_t)opt[2], (uint32_t)opt[3], (uint32_t)opt[4], (int)opt[5], (int)opt[6], (int)opt[7],
                            (int)opt[8], (int)opt[9], (int)opt[10], (int)opt[11], (int)opt[12], (int)opt[13], (int)opt[14], (int)opt[15], (int)opt[16],
                            (int)opt[17], (int)opt[18], (int)opt[19]};
    rp_call_facts f;
    f.nbatch = (size_t)fact[0], f.rlc = fact[1], f.ts_per_proof = fact[2], f.ts_uniform = fact[3], f.want_out = fact[4], f.second_stream = fact[5];
    f.nseg = (uint32_t)fact[6], f.nlabels = (uint32_t)fact[7];
    fb_params prm;
    prm.W = window_bits, prm.nwin = fb_nwin(window_bits), prm.half = 1u << (window_bits - 1), prm.n_gens = cl.shape_verdict ? 2 : (uint32_t)(2 * n * m + 2);
    rp_chain_plan p;
    rp_plan_chain(p, o, cl, n, m, proof_len, prm, f);
    out[4] = p.refused != nullptr;
    if (p.refused) return 5;
    const uint64_t v[] = {p.forms, p.scripted, p.coop, p.sh.coop_split, p.narrow_walk, p.sh.narrow_hi, p.vb_chunk_sz, p.rlc_bucket, p.exp_form, p.exp_w3,
                          p.fused_finish, p.finish1, p.nsplit, p.nsplit1, p.nparts, p.n_chunks, p.g_stage1, p.n_win + p.n_exp + p.n_rows, p.g_wsum, p.g_stage4,
                          p.g_finish, p.quad, p.one_lane, p.arena_need, p.arena_reserve, p.off_digits, p.off_res1};
    for (size_t i = 0; i < sizeof v / sizeof v[0]; i++) out[5 + i] = v[i];
    return 5 + (int)(sizeof v / sizeof v[0]);
}

// ---- one verification call (device pointers; the context is locked, the device set) -----------------------------------------------------------
struct rp_call {
    // inputs
    size_t n = 0, m = 0, nbatch = 0, proof_len = 0;
    const void *d_proofs = nullptr, *d_commitments = nullptr;
    rp_transcripts tr;
    const void *d_rng64 = nullptr;       // 64 bytes per proof; null: expanded on the device from the chain's key
    const void *d_weights64 = nullptr;   // combined check only; null: likewise
    // outputs
    void *d_verdict = nullptr;
    void *d_msm_out = nullptr;           // per-proof check: 32 bytes per proof, optional
    void *d_batch_out = nullptr;         // combined check: 33 bytes (batch verdict, encoding of the combined point), optional
    // mode
    bool rlc = false;                    // the batch-combined check (bpgpu_rangeproof_verify_rlc[_dev])
    hipStream_t s = nullptr;
    bool dev_call = false;               // a device-pointer entry point: nothing but this chain's own pieces is staged
    // coalesced launch (bpgpu_pool_*): the nbatch proofs are the concatenation of nseg submitted items, each with its own input / output buffers
    // (the pointers above stay null)
    const rp_seg *segs = nullptr;
    uint32_t nseg = 0;
    bool seg_wants_out = false;          // some item wants its encodings (combined: the 33-byte result)
    bool seg_brought_rng = false;        // every item brought its own rng bytes: the library draws none
};
// a chain on its way into the stream: the call, its plan, and the plan's pieces as pointers
struct rp_chain {
    bpgpu_ctx *c;
    hipStream_t s;
    const rp_call &a;
    const rp_chain_plan &p;
    rp_shape sh;                 // the plan's, with the chain's seed
    fb_params prm;               // the window table the generator terms walk, its entries and the shape's ids in it
    const fb_entry *gen_table;
    uint32_t *d_ids;
    rp_strobe_init init;
    uint32_t ts_flags;
    const rp_script_hdr *d_script;
    rp_seg_tab segtab;
    vb_dev d;
    bk_dev bd;
    ge_cached *tab_hi;           // the points' second to fourth tables (plan.hi), behind the first ones
    uint32_t *d_status, *d_fields;
    fb_digit *d_digits;
    ge_ext *d_partial;
    const uint8_t *rng_ptr, *wts_ptr;
    bool want_out;
};

// every proof of the batch has the same malformed length: FormatError for all, the callers' transcripts untouched, nothing to combine
static int rp_answer_malformed(bpgpu_ctx *c, const rp_call &a, uint32_t all_verdict) {
    const rp_transcripts &tr = a.tr;
    const size_t nbatch = a.nbatch;
    hipStream_t s = a.s;
    if (tr.d_ts_out) {
        if (tr.d_ts_in) HIPCHK(c, hipMemcpyAsync(tr.d_ts_out, tr.d_ts_in, nbatch * BPGPU_TRANSCRIPT_BYTES, hipMemcpyDeviceToDevice, s));
        else {
            char *h = nullptr;
            int rcp = c->io.pin_alloc(nbatch * BPGPU_TRANSCRIPT_BYTES, &h);
            if (rcp) return rcp;
            uint8_t st0[BPGPU_TRANSCRIPT_BYTES];
            if (tr.shared_ts) memcpy(st0, tr.shared_ts, BPGPU_TRANSCRIPT_BYTES);
            else bpgpu_transcript_new(tr.label, tr.label_len, st0);
            for (size_t b = 0; b < nbatch; b++) memcpy(h + b * BPGPU_TRANSCRIPT_BYTES, st0, BPGPU_TRANSCRIPT_BYTES);
            HIPCHK(c, hipMemcpyAsync(tr.d_ts_out, h, nbatch * BPGPU_TRANSCRIPT_BYTES, hipMemcpyHostToDevice, s));
        }
    }
    HIPCHK(c, hipMemsetAsync(a.d_verdict, (int)all_verdict, nbatch, s));
    if (a.d_msm_out) HIPCHK(c, hipMemsetAsync(a.d_msm_out, 0, nbatch * 32, s));
    if (a.rlc && a.d_batch_out) HIPCHK(c, hipMemsetAsync(a.d_batch_out, 0, 33, s));
    return BPGPU_OK;
}

// which window table the generator terms walk: the secondary one when the shape fits it (bpgpu_gens_add_shape), else the primary; the shape's ids in it
static int rp_table_for(bpgpu_ctx *c, const rp_class &cl, size_t n, size_t m, fb_params *prm, const fb_entry **table, uint32_t **d_ids) {
    const bool use_sec = c->sec.d_table && !cl.shape_verdict && n <= c->sec.n && m <= c->sec.m;
    *prm = use_sec ? c->sec.prm : c->prm;
    *table = use_sec ? c->sec.d_table : c->d_table;
    *d_ids = nullptr;
    if (cl.shape_verdict) return BPGPU_OK;
    return use_sec ? gen_ids_for_secondary(c, n, m, d_ids) : gen_ids_for(c, n, m, d_ids);
}

// the context's buffers as a plan wants them: the arena, the arrival counters of the fused finish, the status words
static int rp_reserve_buffers(bpgpu_ctx *c, size_t arena_bytes, size_t nbatch) {
    int rc = arena_reserve(c, arena_bytes);
    if (rc) return rc;
    if (!c->fin_cnt) {
        HIPCHK(c, hipMalloc((void **)&c->fin_cnt, 256 * 4));
        HIPCHK(c, hipMemset(c->fin_cnt, 0, 256 * 4));
    }
    if (c->rp_status_cap < nbatch) {
        if (c->rp_status) HIPCHK(c, hipFree(c->rp_status));
        c->rp_status = nullptr;
        c->rp_status_cap = 0;
        HIPCHK(c, hipMalloc((void **)&c->rp_status, nbatch * 4));
        c->rp_status_cap = nbatch;
        c->rp_status_dirty = true;
    }
    return BPGPU_OK;
}

// distinct labels among the items of a coalesced launch (usually one)
struct rp_seg_labels {
    std::vector<uint32_t> of;             // item -> index into `distinct`
    std::vector<const uint8_t *> distinct;
};
static void rp_distinct_labels(rp_seg_labels &l, const rp_transcripts &tr, uint32_t nseg) {
    l.of.resize(nseg);
    for (uint32_t i = 0; i < nseg; i++) {
        uint32_t j = 0;
        while (j < l.distinct.size() && tr.label_len != 0 && memcmp(l.distinct[j], tr.seg_labels[i], tr.label_len) != 0) j++;
        if (j == l.distinct.size()) l.distinct.push_back(tr.seg_labels[i]);
        l.of[i] = j;
    }
}

// What a chain needs in place before launch 1: its seed, the start states of its items' labels, the segment table, the transcript start and script
static int rp_stage_chain(rp_chain &ch, const rp_seg_labels &labels) {
    bpgpu_ctx *c = ch.c;
    const rp_call &a = ch.a;
    const rp_chain_plan &p = ch.p;
    const rp_transcripts &tr = a.tr;
    hipStream_t s = ch.s;
    char *arena = c->arena;
    int rc;
    // randomness the caller did not bring -- the batching challenge's rng bytes (thread_rng() in verify_multiple, mod.rs:455-470), the
    // combination weights (unpredictable to the prover) -- is expanded inside launch 1 from ONE key per launch chain (rp_shape::seed,
    // rangeproof.h): drawn here from the calling thread's generator (hostrng.h), carried in the kernel's argument block
    rp_shape &sh = ch.sh;
    if (!ch.rng_ptr && !a.seg_brought_rng) sh.seeded |= RP_SEED_RNG;
    if (a.rlc && !ch.wts_ptr) sh.seeded |= RP_SEED_WEIGHTS;
    if (sh.seeded) {
        if (c->test_seed_set) memcpy(sh.seed, c->test_seed, 32);
        else if (!bp::fast_random((uint8_t *)sh.seed, 32)) return fail(c, BPGPU_ERR_HIP, "getrandom failed");
    }
    const size_t nlabels = labels.distinct.size();
    const bool own_inits = nlabels > 1;
    if (own_inits) {   // Transcript::new(label) + rangeproof_domain_sep(n, m) of every distinct label: 50 sponge words each, staged ahead of the chain
        char *h = nullptr;
        rc = c->io.pin_alloc(nlabels * 256, &h);
        if (rc) return rc;
        for (size_t j = 0; j < nlabels; j++) {
            rp_strobe_init ij;
            make_strobe_init(ij, labels.distinct[j], tr.label_len, a.n, a.m);
            memcpy(h + j * 256, ij.w, 200);
        }
        HIPCHK(c, hipMemcpyAsync(arena + p.off_inits, h, nlabels * 256, hipMemcpyHostToDevice, s));
    }
    auto seg_fix = [&](rp_seg *dst) {   // (the pool's table carries no start states: they live in this chain's arena)
        for (uint32_t i = 0; i < a.nseg; i++) dst[i].init_w = own_inits ? (const uint32_t *)(arena + p.off_inits + (size_t)labels.of[i] * 256) : nullptr;
    };
    rp_seg_tab &segtab = ch.segtab;
    memset(&segtab, 0, sizeof segtab);
    if (a.segs && a.nseg <= RP_SEG_INLINE) {   // travels in the kernels' argument blocks
        segtab.n = a.nseg;
        memcpy(segtab.in, a.segs, (size_t)a.nseg * sizeof(rp_seg));
        seg_fix(segtab.in);
    } else if (a.segs) {
        char *h = nullptr;
        rc = c->io.pin_alloc((size_t)a.nseg * sizeof(rp_seg), &h);
        if (rc) return rc;
        memcpy(h, a.segs, (size_t)a.nseg * sizeof(rp_seg));
        seg_fix((rp_seg *)h);
        HIPCHK(c, hipMemcpyAsync(arena + p.off_segs, h, (size_t)a.nseg * sizeof(rp_seg), hipMemcpyHostToDevice, s));
        segtab.n = a.nseg;
        segtab.ext = (const rp_seg *)(arena + p.off_segs);
    }
    rp_strobe_init &init = ch.init;
    ch.ts_flags = 0;
    if (tr.d_ts_in || tr.shared_ts) {
        ch.ts_flags = BP_TS_DOMSEP;
        if (tr.shared_ts) strobe_init_from_state(init, tr.shared_ts);
        else {
            memset(&init, 0, sizeof init);
            if (tr.ts_uniform) {
                init.pos = tr.u_pos;
                init.pos_begin = tr.u_pos_begin;
                init.cur_flags = tr.u_flags;
            }
        }
    } else if (tr.d_ts_out) {   // label + states wanted back: start every proof from Transcript::new(label) and replay the domain separator on the device
        uint8_t st0[BPGPU_TRANSCRIPT_BYTES];
        bpgpu_transcript_new(tr.label, tr.label_len, st0);
        strobe_init_from_state(init, st0);
        ch.ts_flags = BP_TS_DOMSEP;
    } else {
        make_strobe_init(init, tr.label, tr.label_len, a.n, a.m);
    }
    ch.d_script = nullptr;
    if (p.scripted) {   // every proof starts at the position of `init`: the per-shape script replaces the byte-wise replay
        rc = script_for(c, s, sh.n, sh.m, sh.k, init, (ch.ts_flags & BP_TS_DOMSEP) != 0, &ch.d_script);
        if (rc) return rc;
    }
    if (c->io.pin_off > c->io.pin_marked && a.dev_call) {   // segment table / start states / a new transcript script staged above, nothing else will be
        rc = c->io.pin_mark(s);
        if (rc) return rc;
    }
    return BPGPU_OK;
}

// ---- the launches of a chain, one function per branch ----------------------------------------------------------------------------------------
// launch 1: transcripts and per-proof scalars || the proofs' points decoded into their tables -- 32 lanes per proof (narrow), lane = proof on the
// script, lane = proof replaying byte-wise
static int rp_enqueue_launch1(rp_chain &ch) {
    bpgpu_ctx *c = ch.c;
    const rp_chain_plan &p = ch.p;
    const rp_transcripts &tr = ch.a.tr;
    const bool bk = p.rlc_bucket;
#define RP_L1_HEAD                                                                                                                                 \
    ch.sh, ch.init, p.n_tr, (const uint8_t *)ch.a.d_proofs, (const uint8_t *)ch.a.d_commitments, ch.rng_ptr, ch.d_fields, ch.d.tab, ch.d_status, ch.prm, \
        p.lg_m, bk ? ch.bd.rwords : ch.d.recoded, ch.d_digits, ch.a.rlc ? ch.wts_ptr : (const uint8_t *)nullptr
#define RP_L1_TAIL                                                                                                                                 \
    (const uint32_t *)tr.d_ts_in, (uint32_t *)tr.d_ts_out, bk ? ch.bd.pts : (fb_entry *)nullptr, bk ? p.bkp.c : 0u, ch.segtab, ch.d_script
    if (p.coop) LAUNCH(c, ch.s, "rp_stage1", k_rp_stage1_coop, p.g_stage1, RP_BLOCK, RP_L1_HEAD, RP_L1_TAIL, p.n_pt, ch.tab_hi);
    else LAUNCH_TF(c, ch.s, ch.d_script != nullptr, "rp_stage1", k_rp_stage1, p.g_stage1, RP_BLOCK, RP_L1_HEAD, ch.ts_flags, RP_L1_TAIL);
#undef RP_L1_HEAD
#undef RP_L1_TAIL
    return BPGPU_OK;
}
// a shape the reference refuses: every proof that parsed gets the shape's code
static int rp_enqueue_shape_verdict(rp_chain &ch) {
    bpgpu_ctx *c = ch.c;
    const rp_call &a = ch.a;
    const uint32_t nb32 = ch.sh.nproofs;
    uint8_t *d_mv = (uint8_t *)(c->arena + ch.p.off_mv);
    HIPCHK(c, hipMemsetAsync(d_mv, 1, a.nbatch, ch.s));
    LAUNCH(c, ch.s, "rp_verdict", k_rp_verdict, (nb32 + 63) / 64, 64, nb32, ch.d_status, d_mv, (uint8_t *)a.d_verdict);
    if (a.d_msm_out) HIPCHK(c, hipMemsetAsync(a.d_msm_out, 0, a.nbatch * 32, ch.s));
    if (a.rlc && a.d_batch_out) HIPCHK(c, hipMemsetAsync(a.d_batch_out, 0, 33, ch.s));
    return BPGPU_OK;
}
// the last launch of a combined check: the one MSM's partial sums + its Horner result, the identity test, every proof's verdict
static void rp_enqueue_rlc_finish(rp_chain &ch, const ge_ext *hq, const ge_ext *part1) {
    LAUNCH_TF(ch.c, ch.s, ch.want_out, "rlc_finish", k_rlc_finish, 1, 64, ch.p.nsplit1, hq, part1, ch.sh.nproofs, ch.d_status, (uint8_t *)ch.a.d_verdict,
              (uint8_t *)ch.a.d_batch_out, ch.segtab);
}
// ---- batch combination, bucket variant: R = sum_i rho_i MegaCheck_i with the per-proof terms as ONE MSM ----
static int rp_enqueue_rlc_buckets(rp_chain &ch) {
    bpgpu_ctx *c = ch.c;
    hipStream_t s = ch.s;
    const rp_chain_plan &p = ch.p;
    const bk_params &bkp = p.bkp;
    bk_dev &bd = ch.bd;
    char *a = c->arena;
    unsigned long long *d_acc = (unsigned long long *)(a + p.off_acc);
    HIPCHK(c, hipMemsetAsync(d_acc, 0, (size_t)p.n_gen_terms * 10 * 8, s));
    LAUNCH(c, s, "rlc_stage3", k_rlc_stage3, p.n_exp, BP_BLOCK, 0u, 0u, (const vb_chunk *)nullptr, (const ge_cached *)nullptr, (const uint32_t *)nullptr,
           (ge_ext *)nullptr, p.nexp, ch.sh, ch.prm, ch.d_fields, ch.d_status, d_acc, (ch.a.nbatch % 64 == 0) ? 1 : 0);
    const uint32_t tot32 = (uint32_t)p.rlc_terms;
    int rc = enqueue_bucket_sort(c, s, bkp, 1u, tot32, p.rlc_terms, 1, bd, ch.d_status, ch.sh.U);
    if (rc) return rc;
    fb_digit *d_dig1 = (fb_digit *)(a + p.off_dig1);
    ge_ext *d_part1 = (ge_ext *)(a + p.off_part1);
    uint32_t *d_ctl = (uint32_t *)(a + p.off_res1 + sizeof(ge_ext));
    const uint32_t nt = bkp.nwin * bkp.half, n_acc = (nt + BP_BLOCK - 1) / BP_BLOCK;
    const uint32_t lim = bk_chain_lim(p.rlc_terms, bkp);
    LAUNCH(c, s, "rlc_accum", k_rlc_accum_scalars, n_acc + p.n_sc, BP_BLOCK, n_acc, nt, bkp, tot32, bd.desc, bd.idx, bd.pts, bd.bsum, p.n_gen_terms,
           (const unsigned long long *)d_acc, d_dig1, ch.prm, d_ctl, lim);
    const uint32_t hg = bk_heavy_groups(bkp, 1);
    LAUNCH(c, s, "bk_heavy", k_bk_heavy, bkp.nwin * hg, 64, bkp, tot32, (const bk_desc *)bd.desc, (const uint32_t *)bd.idx, (const fb_entry *)bd.pts, bd.bsum, lim, hg);
    enqueue_bucket_reduce(c, s, bkp, bkp.nwin, bd);
    LAUNCH(c, s, "rlc_stage4", k_rlc_stage4b, 1 + p.nsplit1, FB_BLOCK, bd.colq16, bd.hq, ch.prm, p.nsplit1, p.npairs, ch.d_ids, d_dig1, ch.gen_table, d_part1);
    rp_enqueue_rlc_finish(ch, bd.hq, d_part1);
    return BPGPU_OK;
}
// ---- batch combination (rlc.h): R = sum_i rho_i MegaCheck_i, the per-proof terms through the window sums and a tree of column sums ----
static int rp_enqueue_rlc_tree(rp_chain &ch) {
    bpgpu_ctx *c = ch.c;
    hipStream_t s = ch.s;
    const rp_chain_plan &p = ch.p;
    vb_dev &d = ch.d;
    char *a = c->arena;
    unsigned long long *d_acc = (unsigned long long *)(a + p.off_acc);
    HIPCHK(c, hipMemsetAsync(d_acc, 0, (size_t)p.n_gen_terms * 10 * 8, s));
    LAUNCH(c, s, "rlc_stage3", k_rlc_stage3, p.n_win + p.n_exp, BP_BLOCK, p.n_win, p.nwin, d.chunks, d.tab, d.recoded, d.part, p.nexp, ch.sh, ch.prm,
           ch.d_fields, ch.d_status, d_acc, (ch.a.nbatch % 64 == 0) ? 1 : 0);
    // column sums over ALL chunks of ALL proofs: rows of 64 window sums, tree-added 16- then 8-way until <= 8 rows
    // remain; the Horner wavefront adds those itself
    fb_digit *d_dig1 = (fb_digit *)(a + p.off_dig1);
    ge_ext *d_part1 = (ge_ext *)(a + p.off_part1), *d_hq1 = (ge_ext *)(a + p.off_res1);
    uint32_t *d_ctl = (uint32_t *)(a + p.off_res1 + sizeof(ge_ext));   // [0] unused, [1] zero, [2..4) chunk bounds {0, rows}
    ge_ext *cur = d.part, *next = (ge_ext *)(a + p.off_tree);
    uint32_t rows = (uint32_t)p.n_chunks;
    // a level leaves ng groups of rows; the coefficient reduction shares the launch of the last level (ng <= 8) -- or, where <= 8 rows need no level
    // (ng = 0), has that launch to itself
    for (bool last = false; !last;) {
        const uint32_t group = rows > 64 ? 16 : 8, ng = rows > 8 ? (rows + group - 1) / group : 0, nt = ng * 64, n_level = (nt + BP_BLOCK - 1) / BP_BLOCK;
        last = ng <= 8;
        if (last)
            LAUNCH(c, s, "rlc_colsum", k_rlc_colsum_scalars, n_level + p.n_sc, BP_BLOCK, n_level, nt, ng ? rows : 0u, ng ? group : 1u, (const ge_ext *)cur, next,
                   p.n_gen_terms, (const unsigned long long *)d_acc, d_dig1, ch.prm, d_ctl, ng ? ng : rows);
        else LAUNCH(c, s, "rlc_colsum", k_fb_reduce, n_level, BP_BLOCK, nt, 64u, rows, group, cur, next);
        if (ng) cur = next, next = next + (size_t)nt, rows = ng;
    }
    LAUNCH(c, s, "rlc_stage4", k_rp_stage4<64>, 1 + p.nsplit1, FB_BLOCK, 1u, d_ctl + 2, cur, (const ge_cached *)nullptr, d_hq1, ch.prm, 1u, 1u,
           p.nsplit1, p.npairs, ch.d_ids, d_dig1, ch.gen_table, d_part1, 0u, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint8_t *)nullptr, rp_seg_tab{});
    rp_enqueue_rlc_finish(ch, d_hq1, d_part1);
    return BPGPU_OK;
}

// more than one chunk per proof: the chunks' window sums added into column sums, as cached points (both the quad and the one-lane chain read them)
static void rp_enqueue_colsum(rp_chain &ch) {
    LAUNCH(ch.c, ch.s, "vb_colsum", k_vb_colsum, ch.p.g_colsum, BP_BLOCK, ch.sh.nproofs * 64, ch.d.chunk_first, ch.d.part, (uint32_t *)nullptr, (ge_cached *)ch.d.colq16);
}
// Launch 3 holds two independent roles -- window sums and generator exponents.  Narrow chains keep them fused (one launch fewer on the
// latency path); wide chains split them, and may move the Horner chains to the second stream (rp_chain_forms).
static int rp_enqueue_launch3_wide(rp_chain &ch) {
    bpgpu_ctx *c = ch.c;
    hipStream_t s = ch.s;
    const rp_chain_plan &p = ch.p;
    const rp_shape &sh = ch.sh;
    vb_dev &d = ch.d;
    const uint32_t nb32 = sh.nproofs;
    ge_cached *d_colc = p.quad ? (ge_cached *)d.colq16 : nullptr;
    const bool wide_sums = p.r5 || p.a_out;
    // After launch 1 a chain has two INDEPENDENT branches: the proof's own points (window sums -> Horner chain) and the generator terms
    // (exponents -> table walk); they meet in the finish.  With the Horner chains aside, the first branch's LAST kernel goes to the
    // second stream.  (Moving the whole branch there, or the exponents instead, were options until round 6: no gain in their A/B.)
    // (A burst of two wide chains runs its phases in lockstep -- profiles/r06/headline_burst_kernel_sequence.txt: both window sums, then both
    // exponent launches, 470 us at two wavefronts per SIMD beside nothing but the Horner chains, then the walks.  Issuing the exponents on the second
    // stream FIRST, under the window sums, was built and measured on the same box: no difference in any bench form, cfg4 -1.3 %
    // (profiles/r06/exp_early_ab.txt) -- removed again.)
    if (wide_sums) LAUNCH_TF(c, s, p.r5, "rp_stage3w", k_vb_window_wide, p.g_wsum, BP_BLOCK, p.nwsum, sh.U, p.a_out ? 1u : 0u, d.tab, d.recoded, d_colc);
    else LAUNCH(c, s, "rp_stage3w", k_vb_window_colc, p.g_wsum, BP_BLOCK, p.nwsum, d.chunks, d.tab, d.recoded, d.part, (p.quad && p.one_chunk) ? d_colc : (ge_cached *)nullptr);
    if (p.aside) {
        if (!p.one_chunk && !wide_sums) rp_enqueue_colsum(ch);
        HIPCHK(c, hipEventRecord(c->fork_ev, s));
        HIPCHK(c, hipStreamWaitEvent(c->stream2, c->fork_ev, 0));
        const ge_cached *extra = p.a_out ? d.tab : (const ge_cached *)nullptr;
        if (wide_sums) LAUNCH_TF(c, c->stream2, p.r5, "rp_horner1", k_rp_horner_wide, p.nblk_p, FB_BLOCK, nb32, d_colc, extra, (p.r5 ? 16u : 8u) * sh.U, d.hq);
        else LAUNCH(c, c->stream2, "rp_horner1", k_rp_horner1, p.nblk_p, FB_BLOCK, nb32, d_colc, d.hq);
        HIPCHK(c, hipEventRecord(c->join_ev, c->stream2));
    }
    if (p.exp_w3) LAUNCH(c, s, "rp_stage3", k_rp_exponents_w3, p.n_exp, BP_BLOCK, p.nexp, sh, ch.prm, ch.d_fields, ch.d_digits, ch.d_status);
    else LAUNCH_TF(c, s, p.exp_form == RP_EXP_PAIRS, "rp_stage3", k_rp_exponents, p.n_exp, BP_BLOCK, p.nexp, sh, ch.prm, ch.d_fields, ch.d_digits, ch.d_status);
    return BPGPU_OK;
}
static int rp_enqueue_launch3_fused(rp_chain &ch) {
    const rp_chain_plan &p = ch.p;
    vb_dev &d = ch.d;
    ge_cached *colc3 = (p.quad && p.one_chunk) ? (ge_cached *)d.colq16 : (ge_cached *)nullptr;
    LAUNCH_SEL3(ch.c, ch.s, p.exp_form, 0, 1, 2, "rp_stage3", k_rp_stage3, p.n_win + p.n_exp + p.n_rows, BP_BLOCK, p.n_win, p.nwin, d.chunks, d.tab, d.recoded, d.part,
                colc3, p.nexp, ch.sh, ch.prm, ch.d_fields, ch.d_digits, ch.d_status, p.n_exp, p.nrows, p.lg_m, (const ge_cached *)ch.tab_hi);
    return BPGPU_OK;
}
// launch 4: the Horner chains (unless they ran aside) || the walk of the generator table -- one lane, four lanes (also the form without a Horner role)
// or a wavefront per chain; a narrow walk (lane = split: k_rp34.hip rp_walk_narrow) folds a proof's partial sums itself and may finish the proof
static int rp_enqueue_launch4(rp_chain &ch) {
    bpgpu_ctx *c = ch.c;
    const rp_chain_plan &p = ch.p;
    vb_dev &d = ch.d;
    const bool folds = p.walk_flags != 0;
    const ge_cached *d_colc = p.quad ? (const ge_cached *)d.colq16 : nullptr;
    LAUNCH_SEL3(c, ch.s, !p.quad ? 2 : ((p.one_lane && !p.aside) ? 0 : 1), 1, 4, 64, "rp_stage4", k_rp_stage4, p.g_stage4, FB_BLOCK, p.n_hw, d.chunk_first, d.part, d_colc,
                d.hq, ch.prm, ch.sh.nproofs, p.nblk_p, p.nsplit, p.npairs, ch.d_ids, ch.d_digits, ch.gen_table, ch.d_partial, p.walk_flags,
                folds ? c->fin_cnt : (uint32_t *)nullptr, folds ? ch.d_status : (uint32_t *)nullptr, folds ? (uint8_t *)ch.a.d_verdict : (uint8_t *)nullptr,
                folds ? ch.segtab : rp_seg_tab{});
    if (p.aside) HIPCHK(c, hipStreamWaitEvent(ch.s, c->join_ev, 0));
    return BPGPU_OK;
}
// the finish: a proof's partial sums + its Horner result, the identity test, the verdict (and the encoding, where wanted)
static int rp_enqueue_finish(rp_chain &ch) {
    bpgpu_ctx *c = ch.c;
    const rp_chain_plan &p = ch.p;
    const uint32_t nb32 = ch.sh.nproofs;
    ge_ext *d_red = nullptr;
    uint32_t nred = 0;
    enqueue_fb_reduce(c, ch.s, nb32, p.nparts, ch.d_partial, &d_red, &nred, 64);   // 8 lanes x <= 8 partials each in finish8
#define RP_FINISH_ARGS nb32, nred, ch.d.hq, d_red, ch.d_status, (uint32_t *)ch.a.d_msm_out, (uint8_t *)ch.a.d_verdict, 1, ch.segtab
    if (p.finish1) LAUNCH_TF(c, ch.s, ch.want_out, "finish1", k_finish1, p.g_finish, 64, RP_FINISH_ARGS);
    else LAUNCH_TF(c, ch.s, ch.want_out, "finish8", k_finish8, p.g_finish, 64, RP_FINISH_ARGS);
#undef RP_FINISH_ARGS
    return BPGPU_OK;
}
static int rp_enqueue_chain(rp_chain &ch) {
    const rp_chain_plan &p = ch.p;
    int rc = rp_enqueue_launch1(ch);
    if (rc) return rc;
    if (ch.sh.shape_verdict) return rp_enqueue_shape_verdict(ch);
    if (p.rlc_bucket) return rp_enqueue_rlc_buckets(ch);
    if (ch.a.rlc) return rp_enqueue_rlc_tree(ch);
    rc = p.wide ? rp_enqueue_launch3_wide(ch) : rp_enqueue_launch3_fused(ch);
    if (rc) return rc;
    if (p.quad && !p.one_chunk && !p.aside) rp_enqueue_colsum(ch);
    rc = rp_enqueue_launch4(ch);
    if (rc || p.fused_finish) return rc;   // (fused: the last workgroup of every proof has written its verdict and zeroed its status word)
    return rp_enqueue_finish(ch);
}

// One launch chain over a.nbatch proofs of one shape: classify, plan, reserve, stage, enqueue.
static int rp_verify_chain(bpgpu_ctx *c, const rp_call &a) {
    const rp_transcripts &tr = a.tr;
    hipStream_t s = a.s;
    if (a.nbatch == 0) {
        if (a.rlc && a.d_batch_out) HIPCHK(c, hipMemsetAsync(a.d_batch_out, 0, 33, s));
        return BPGPU_OK;
    }
    if (!c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    if (a.nbatch > 0x7fffffffu / 64) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large");
    const rp_class cl = rp_classify(a.n, a.m, a.proof_len, c->gens_capacity, c->party_capacity);
    if (tr.shared_ts && !ts_state_ok(tr.shared_ts)) return fail(c, BPGPU_ERR_INVALID_ARG, "malformed transcript state");
    if (a.segs && (cl.all_verdict || tr.d_ts_in || tr.d_ts_out || tr.shared_ts || (a.rlc && a.d_weights64)))   // (the pool sends such items through the ordinary entry point)
        return fail(c, BPGPU_ERR_INVALID_ARG, "coalesced launches take well-formed shapes and a label only (batch-combined ones: library-drawn weights)");
    if (cl.all_verdict) return rp_answer_malformed(c, a, cl.all_verdict);
    if (cl.unsupported) return fail(c, BPGPU_ERR_INVALID_ARG, "n*m > 2^%d not supported", BP_RP_MAX_K);
    if (a.segs && cl.shape_verdict) return fail(c, BPGPU_ERR_INVALID_ARG, "coalesced launches take well-formed shapes only");
    rp_seg_labels labels;
    if (a.segs && tr.seg_labels) rp_distinct_labels(labels, tr, a.nseg);
    rp_call_facts f;
    f.nbatch = a.nbatch;
    f.rlc = a.rlc;
    f.ts_per_proof = tr.d_ts_in != nullptr;
    f.ts_uniform = tr.ts_uniform;
    f.want_out = a.segs ? a.seg_wants_out : (a.rlc ? a.d_batch_out : a.d_msm_out) != nullptr;
    f.second_stream = s == c->stream2;
    f.nseg = a.segs ? a.nseg : 0;
    f.nlabels = (uint32_t)labels.distinct.size();
    fb_params prm;
    const fb_entry *gen_table;
    uint32_t *d_ids;
    int rc = rp_table_for(c, cl, a.n, a.m, &prm, &gen_table, &d_ids);
    if (rc) return rc;
    rp_chain_plan p;
    rp_plan_chain(p, rp_plan_opts_of(c), cl, a.n, a.m, a.proof_len, prm, f);
    if (p.refused) return fail(c, BPGPU_ERR_INVALID_ARG, "%s", p.refused);
    rc = rp_reserve_buffers(c, p.arena_need, a.nbatch);
    if (rc) return rc;
    rp_chain ch = {c, s, a, p, p.sh, prm, gen_table, d_ids};
    char *arena = c->arena;
    ch.d_status = c->rp_status;
    ch.d_digits = (fb_digit *)(arena + p.off_digits);
    ch.d_partial = (ge_ext *)(arena + p.off_partial);
    ch.d_fields = (uint32_t *)(arena + p.off_fields);
    ch.rng_ptr = (const uint8_t *)a.d_rng64;
    ch.wts_ptr = (const uint8_t *)a.d_weights64;
    ch.want_out = f.want_out;
    rc = rp_stage_chain(ch, labels);
    if (rc) return rc;
    if (c->rp_status_dirty) {   // (a chain whose enqueue failed half way: its status words and arrival counters were not handed back clean)
        HIPCHK(c, hipMemsetAsync(ch.d_status, 0, c->rp_status_cap * 4, s));
        HIPCHK(c, hipMemsetAsync(c->fin_cnt, 0, 256 * 4, s));
    }
    c->rp_status_dirty = true;   // until the kernel that resets the words has been enqueued: every error return below leaves it set
    // the proof-specific ("variable-base") terms: decomposition into chunks is cached per (U, chunk size)
    if (p.rlc_bucket) bucket_bind(c, p.boff, ch.bd);
    else if (!cl.shape_verdict) {
        bpgpu_ctx::plan_view pv;
        rc = uniform_plan(c, a.nbatch, ch.sh.U, &pv, p.vb_chunk_sz);
        if (rc) return rc;
        vb_bind(c, p.off, ch.d);
        ch.d.chunks = (vb_chunk *)pv.mem;
        ch.d.chunk_first = (uint32_t *)(pv.mem + pv.o1);
        ch.d.hq = (ge_ext *)((char *)ch.d.colq16 + a.nbatch * 64 * sizeof(ge_cached));
        ch.tab_hi = p.hi ? ch.d.tab + (size_t)8 * ch.sh.nproofs * ch.sh.U : (ge_cached *)nullptr;
    }
    rc = rp_enqueue_chain(ch);
    if (rc) return rc;
    HIPCHK(c, hipGetLastError());
    c->rp_status_dirty = false;
    return BPGPU_OK;
}

// ---- entry points: device pointers ----------------------------------------------------------------------
// what every call brings: the shape, the proofs with their commitments and transcripts, the rng bytes, where the verdicts go.  The rest -- encodings,
// the combined check with its weights and result, segments -- is set by name
static rp_call rp_call_of(size_t n, size_t m, size_t nbatch, const void *d_proofs, size_t proof_len, const void *d_commitments, const rp_transcripts &tr,
                          const void *d_rng64, void *d_verdict) {
    rp_call a;
    a.n = n, a.m = m, a.nbatch = nbatch, a.proof_len = proof_len;
    a.d_proofs = d_proofs, a.d_commitments = d_commitments, a.tr = tr, a.d_rng64 = d_rng64, a.d_verdict = d_verdict;
    return a;
}
static int rp_dev_call(bpgpu_ctx *c, rp_call a, void *stream) {
    const rp_transcripts &tr = a.tr;
    if (!c || (a.nbatch && (!a.d_proofs || !a.d_verdict || (a.m && !a.d_commitments))) || (tr.label_len && !tr.label)) return BPGPU_ERR_INVALID_ARG;
    if (((uintptr_t)a.d_proofs | (uintptr_t)a.d_commitments | (uintptr_t)a.d_rng64 | (uintptr_t)a.d_weights64 | (uintptr_t)tr.d_ts_in | (uintptr_t)tr.d_ts_out) & 3)
        return fail(c, BPGPU_ERR_INVALID_ARG, "device buffers must be 4-byte aligned");
    a.dev_call = true;
    return dev_call(c, stream, [&](hipStream_t s) {
        a.s = s;
        return rp_verify_chain(c, a);
    });
}

// ---- hooks of the pool (pool.hip; not part of the C ABI) -----------------------------------------------------
// can batches of this shape share a launch chain?  (malformed lengths / parameter errors take the ordinary entry point,
// which reports them per proof)
bool bpgpu_internal_rp_coalescible(bpgpu_ctx *c, size_t n, size_t m, size_t proof_len) {
    std::lock_guard<std::mutex> lk(c->mu);
    const rp_class cl = rp_classify(n, m, proof_len, c->gens_capacity, c->party_capacity);
    return c->d_table && !cl.all_verdict && !cl.shape_verdict && !cl.unsupported;
}
// has everything enqueued on the context's own stream completed?
bool bpgpu_internal_idle(bpgpu_ctx *c) {
    std::lock_guard<std::mutex> lk(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) return false;
    const hipError_t e = hipStreamQuery(c->stream);
    if (e != hipSuccess) (void)hipGetLastError();   // hipErrorNotReady is not an error
    return e == hipSuccess;
}
// What the pool knows about the chain it issues on this context -- busy: 1 = others run beside it, 0 = alone, -1 = nothing -- is an
// argument of the two hooks below and is forgotten when the call returns: a lane never runs on what an earlier call left behind.
// (bpgpu_internal_set_busy_hint stays for the host-pointer slices, whose worker sets it immediately before every submit.)
void bpgpu_internal_set_busy_hint(bpgpu_ctx *c, int busy) {
    std::lock_guard<std::mutex> lk(c->mu);
    c->busy_hint = busy;
}
// one coalesced launch chain over the concatenation of `nseg` items, on the context's own stream (asynchronous)
// rlc: ONE batch-combined check over all items (bpgpu_pool_rangeproof_submit_rlc_dev); any_msm then means "some item wants the 33-byte result"
int bpgpu_internal_rp_verify_segs(bpgpu_ctx *c, size_t n, size_t m, size_t proof_len, const uint8_t *const *labels, size_t label_len, const rp_seg *segs,
                                  uint32_t nseg, bool any_msm, uint32_t splits_hint, int busy, bool rlc) {
    if (!c || !segs || nseg == 0 || !labels) return BPGPU_ERR_INVALID_ARG;
    const uint8_t *label = labels[0];
    const size_t total = (size_t)segs[nseg - 1].first + segs[nseg - 1].count;
    bool any_rng_missing = false;
    for (uint32_t i = 0; i < nseg; i++) any_rng_missing = any_rng_missing || !segs[i].rng64;
    return dev_call(c, nullptr, [&](hipStream_t s) {   // (no stream: the context's own)
        rp_transcripts tr;
        tr.label = label;
        tr.label_len = label_len;
        tr.seg_labels = labels;
        c->splits_hint = splits_hint;
        c->busy_hint = busy;
        rp_call a = rp_call_of(n, m, total, nullptr, proof_len, nullptr, tr, nullptr, nullptr);   // (inputs and outputs: the items' own)
        a.rlc = rlc;
        a.s = s;
        a.dev_call = true;
        a.segs = segs;
        a.nseg = nseg;
        a.seg_wants_out = any_msm;
        a.seg_brought_rng = !any_rng_missing;   // (the library then draws no randomness: nobody would read it)
        const int rc = rp_verify_chain(c, a);
        c->splits_hint = 0;
        c->busy_hint = -1;
        return rc;
    });
}
// buffers of the context sized for chains of up to `nbatch_max` proofs of this shape -- the arena, the status words, the cached chunk decompositions:
// a lane of the pool's combining queue sees chains of every width and should not grow its buffers (a device-wide synchronisation each time) on the way
// up.  Sized from the plan of the widest per-proof chain on a label, beside other chains (rp_chain_plan::arena_reserve).
int bpgpu_internal_rp_reserve(bpgpu_ctx *c, size_t n, size_t m, size_t proof_len, size_t nbatch_max) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (nbatch_max == 0) return BPGPU_OK;
    if (!c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    if (nbatch_max > 0x7fffffffu / 64) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large");
    const rp_class cl = rp_classify(n, m, proof_len, c->gens_capacity, c->party_capacity);
    if (cl.all_verdict) return BPGPU_OK;   // (a malformed length never reaches a chain)
    if (cl.unsupported) return fail(c, BPGPU_ERR_INVALID_ARG, "n*m > 2^%d not supported", BP_RP_MAX_K);
    fb_params prm;
    const fb_entry *gen_table;
    uint32_t *d_ids;
    int rc = rp_table_for(c, cl, n, m, &prm, &gen_table, &d_ids);
    if (rc) return rc;
    rp_plan_opts o = rp_plan_opts_of(c);
    o.busy_hint = 1;
    rp_call_facts f;
    f.nbatch = nbatch_max;
    rp_chain_plan p;
    rp_plan_chain(p, o, cl, n, m, proof_len, prm, f);
    if (p.refused) return fail(c, BPGPU_ERR_INVALID_ARG, "%s", p.refused);
    rc = rp_reserve_buffers(c, p.arena_reserve, nbatch_max);
    if (rc || cl.shape_verdict) return rc;
    bpgpu_ctx::plan_view pv0;
    if (p.narrow_ok && p.narrow_q != BP_VB_CHUNK) {   // the narrow chains the lane will see
        rc = uniform_plan(c, nbatch_max < RP_NARROW_MAX ? nbatch_max : RP_NARROW_MAX, p.sh.U, &pv0, p.narrow_q);
        if (rc) return rc;
    }
    return (nbatch_max > RP_NARROW_MAX || p.vb_chunk_sz == BP_VB_CHUNK) ? uniform_plan(c, nbatch_max, p.sh.U, &pv0) : BPGPU_OK;
}
// the context's own stream (the pool's combining queue enqueues its staging copies around the chain)
void *bpgpu_internal_stream(bpgpu_ctx *c) { return c ? (void *)c->stream : nullptr; }
// one launch chain over device-resident inputs on the context's own stream (asynchronous): what the combining queue of the pool
// issues for a sealed buffer.  Transcripts: `shared_ts` (one 208-byte state for every proof; no states handed back), or one state
// per proof in d_ts_in / d_ts_out -- with ts_uniform all of them at STROBE position (pos, pos_begin, flags): the scripted replay.
int bpgpu_internal_rp_verify_chain(bpgpu_ctx *c, size_t n, size_t m, size_t nbatch, const void *d_proofs, size_t proof_len, const void *d_commitments,
                                   const uint8_t *shared_ts, const void *d_ts_in, void *d_ts_out, int ts_uniform, uint32_t pos, uint32_t pos_begin,
                                   uint32_t flags, const void *d_rng64, void *d_verdict, void *d_msm_out, uint32_t splits_hint, int busy) {
    if (!c || !d_proofs || !d_verdict || !d_rng64 || (shared_ts == nullptr) == (d_ts_in == nullptr)) return BPGPU_ERR_INVALID_ARG;
    return dev_call(c, nullptr, [&](hipStream_t s) {   // (no stream: the context's own)
        rp_transcripts tr;
        tr.shared_ts = shared_ts;
        tr.d_ts_in = d_ts_in;
        tr.d_ts_out = d_ts_out;
        tr.ts_uniform = d_ts_in && ts_uniform;
        tr.u_pos = pos;
        tr.u_pos_begin = pos_begin;
        tr.u_flags = flags;
        c->splits_hint = splits_hint;
        c->busy_hint = busy;
        rp_call a = rp_call_of(n, m, nbatch, d_proofs, proof_len, d_commitments, tr, d_rng64, d_verdict);
        a.d_msm_out = d_msm_out;
        a.s = s;
        a.dev_call = true;
        const int rc = rp_verify_chain(c, a);
        c->splits_hint = 0;
        c->busy_hint = -1;
        return rc;
    });
}

extern "C" int bpgpu_rangeproof_verify_batch_dev(bpgpu_ctx *c, size_t n, size_t m, size_t nbatch, const void *d_proofs, size_t proof_len,
                                                 const void *d_commitments, const uint8_t *label, size_t label_len, const void *d_rng64,
                                                 void *d_verdict, void *d_msm_out, void *stream) {
    rp_transcripts tr;
    tr.label = label;
    tr.label_len = label_len;
    rp_call a = rp_call_of(n, m, nbatch, d_proofs, proof_len, d_commitments, tr, d_rng64, d_verdict);
    a.d_msm_out = d_msm_out;
    return rp_dev_call(c, a, stream);
}

extern "C" int bpgpu_rangeproof_verify_batch_ts_dev(bpgpu_ctx *c, size_t n, size_t m, size_t nbatch, const void *d_proofs, size_t proof_len,
                                                    const void *d_commitments, const uint8_t *shared_transcript, const void *d_transcripts,
                                                    const void *d_rng64, void *d_verdict, void *d_msm_out, void *d_transcripts_out,
                                                    void *stream) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    if ((shared_transcript != nullptr) == (d_transcripts != nullptr))
        return fail(c, BPGPU_ERR_INVALID_ARG, "give exactly one of shared_transcript / d_transcripts");
    rp_transcripts tr;
    tr.shared_ts = shared_transcript;
    tr.d_ts_in = d_transcripts;
    tr.d_ts_out = d_transcripts_out;
    rp_call a = rp_call_of(n, m, nbatch, d_proofs, proof_len, d_commitments, tr, d_rng64, d_verdict);
    a.d_msm_out = d_msm_out;
    return rp_dev_call(c, a, stream);
}

extern "C" int bpgpu_rangeproof_verify_rlc_dev(bpgpu_ctx *c, size_t n, size_t m, size_t nbatch, const void *d_proofs, size_t proof_len,
                                               const void *d_commitments, const uint8_t *label, size_t label_len, const void *d_rng64,
                                               const void *d_weights64, void *d_verdict, void *d_batch_out, void *stream) {
    rp_transcripts tr;
    tr.label = label;
    tr.label_len = label_len;
    rp_call a = rp_call_of(n, m, nbatch, d_proofs, proof_len, d_commitments, tr, d_rng64, d_verdict);
    a.rlc = true;
    a.d_weights64 = d_weights64;
    a.d_batch_out = d_batch_out;
    return rp_dev_call(c, a, stream);
}

// ---- entry points: host pointers -------------------------------------------------------------------------
// Inputs are packed into the context's pinned staging buffer and go to the persistent device IO buffer in ONE
// asynchronous copy; results come back in one copy; one wait at the end.  No allocation in steady state.
static int rp_host_call(bpgpu_ctx *c, size_t n, size_t m, size_t nbatch, const uint8_t *proofs, size_t proof_len, const uint8_t *commitments,
                        rp_transcripts tr, const uint8_t *ts_in_host, const uint8_t *rng64, uint8_t *verdict, uint8_t *msm_out,
                        uint8_t *ts_out_host, bool rlc, const uint8_t *weights64, uint8_t *batch_out, bool submit = false) {
    if (!c || (nbatch && (!proofs || !verdict || (m && !commitments))) || (tr.label_len && !tr.label)) return BPGPU_ERR_INVALID_ARG;
    if (nbatch == 0) {
        if (batch_out) memset(batch_out, 0, 33);
        return BPGPU_OK;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t TS = BPGPU_TRANSCRIPT_BYTES;
    hipStream_t s = c->stream;
    host_call<bpgpu_ctx> io(c, s);
    const int r_p = io.in(nbatch * proof_len + 64), r_c = io.in(nbatch * m * 32 + 64), r_r = io.in(rng64 ? nbatch * 64 : 0),
              r_w = io.in(weights64 ? nbatch * 64 : 0), r_ti = io.in(ts_in_host ? nbatch * TS : 0);
    const int r_v = io.out(nbatch), r_o = io.out(msm_out ? nbatch * 32 : 0), r_b = io.out(rlc ? 64 : 0), r_to = io.out(ts_out_host ? nbatch * TS : 0);
    int rc = io.open();
    if (rc) return rc;
    io.put(r_p, proofs, nbatch * proof_len);
    if (m) io.put(r_c, commitments, nbatch * m * 32);
    if (rng64) io.put(r_r, rng64, nbatch * 64);
    if (weights64) io.put(r_w, weights64, nbatch * 64);
    if (ts_in_host) io.put(r_ti, ts_in_host, nbatch * TS);
    tr.d_ts_in = ts_in_host ? io.d(r_ti) : nullptr;
    tr.d_ts_out = ts_out_host ? io.d(r_to) : nullptr;
    char *d_rng = rng64 ? io.d(r_r) : nullptr;
    rc = io.upload();
    rp_call a = rp_call_of(n, m, nbatch, io.d(r_p), proof_len, io.d(r_c), tr, d_rng, io.d(r_v));
    a.s = s;
    a.d_msm_out = msm_out ? io.d(r_o) : nullptr;
    a.rlc = rlc;
    a.d_weights64 = weights64 ? io.d(r_w) : nullptr;
    a.d_batch_out = rlc ? io.d(r_b) : nullptr;
    if (!rc) rc = rp_verify_chain(c, a);
    rc = io.download(rc);
    if (submit && !rc) {   // asynchronous form: leave the results in flight; bpgpu_ctx_collect (or the next call) delivers them
        const int rcl = io.leave_in_flight();
        if (rcl) return rcl;
        c->pend.active = true;
        c->pend.h_out = io.h(r_v);
        c->pend.nbatch = nbatch;
        c->pend.off_msm = io.off[r_o] - io.off[r_v];
        c->pend.off_ts = io.off[r_to] - io.off[r_v];
        c->pend.verdict = verdict;
        c->pend.msm_out = msm_out;
        c->pend.ts_out = ts_out_host;
        return BPGPU_OK;
    }
    rc = io.finish(rc);
    if (rc) return rc;
    if (rlc) {
        // where the combination is not the identity some proof fails: find out which, proof by proof (inputs are still on the device)
        rc = io.deliver_combined(r_v, verdict, nbatch, r_b, batch_out, r_to, ts_out_host, nbatch * TS,
                                 [&] {   // the per-proof chain on the same inputs
                                     a.rlc = false;
                                     a.d_weights64 = a.d_batch_out = nullptr;
                                     return rp_verify_chain(c, a);
                                 });
        if (rc) return rc;
    } else {
        memcpy(verdict, io.h(r_v), nbatch);
        if (ts_out_host) memcpy(ts_out_host, io.h(r_to), nbatch * TS);
    }
    if (msm_out) memcpy(msm_out, io.h(r_o), nbatch * 32);
    return BPGPU_OK;
}

extern "C" int bpgpu_rangeproof_verify_batch(bpgpu_ctx *c, size_t n, size_t m, size_t nbatch, const uint8_t *proofs, size_t proof_len,
                                             const uint8_t *commitments, const uint8_t *label, size_t label_len, const uint8_t *rng64,
                                             uint8_t *verdict, uint8_t *msm_out) {
    rp_transcripts tr;
    tr.label = label;
    tr.label_len = label_len;
    return rp_host_call(c, n, m, nbatch, proofs, proof_len, commitments, tr, nullptr, rng64, verdict, msm_out, nullptr, false, nullptr, nullptr);
}

// asynchronous forms: enqueue and return; verdict / msm_out (and the input buffers' contents are already staged) are
// filled by bpgpu_ctx_collect or implicitly by the next call on the context
extern "C" int bpgpu_rangeproof_verify_batch_submit(bpgpu_ctx *c, size_t n, size_t m, size_t nbatch, const uint8_t *proofs, size_t proof_len,
                                                    const uint8_t *commitments, const uint8_t *label, size_t label_len, const uint8_t *rng64,
                                                    uint8_t *verdict, uint8_t *msm_out) {
    rp_transcripts tr;
    tr.label = label;
    tr.label_len = label_len;
    return rp_host_call(c, n, m, nbatch, proofs, proof_len, commitments, tr, nullptr, rng64, verdict, msm_out, nullptr, false, nullptr, nullptr, true);
}
extern "C" int bpgpu_ctx_collect(bpgpu_ctx *c) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return collect_locked(c);
}

extern "C" int bpgpu_rangeproof_verify_batch_ts(bpgpu_ctx *c, size_t n, size_t m, size_t nbatch, const uint8_t *proofs, size_t proof_len,
                                                const uint8_t *commitments, const uint8_t *transcripts, size_t transcript_stride,
                                                const uint8_t *rng64, uint8_t *verdict, uint8_t *msm_out, uint8_t *transcripts_out) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    if (!transcripts || (transcript_stride != 0 && transcript_stride != BPGPU_TRANSCRIPT_BYTES))
        return fail(c, BPGPU_ERR_INVALID_ARG, "transcripts missing, or transcript_stride neither 0 nor BPGPU_TRANSCRIPT_BYTES");
    if (transcript_stride)
        for (size_t b = 0; b < nbatch; b++)
            if (!ts_state_ok(transcripts + b * BPGPU_TRANSCRIPT_BYTES)) return fail(c, BPGPU_ERR_INVALID_ARG, "malformed transcript state %zu", b);
    rp_transcripts tr;
    if (!transcript_stride) tr.shared_ts = transcripts;
    return rp_host_call(c, n, m, nbatch, proofs, proof_len, commitments, tr, transcript_stride ? transcripts : nullptr, rng64, verdict, msm_out,
                        transcripts_out, false, nullptr, nullptr);
}

// ---- batch combination entry points (rlc.h; SURVEY 8f-3, additional to the reference's API) ---------------
extern "C" int bpgpu_rangeproof_verify_rlc(bpgpu_ctx *c, size_t n, size_t m, size_t nbatch, const uint8_t *proofs, size_t proof_len,
                                           const uint8_t *commitments, const uint8_t *label, size_t label_len, const uint8_t *rng64,
                                           const uint8_t *weights64, uint8_t *verdict, uint8_t *batch_out) {
    rp_transcripts tr;
    tr.label = label;
    tr.label_len = label_len;
    uint8_t bo[33];
    return rp_host_call(c, n, m, nbatch, proofs, proof_len, commitments, tr, nullptr, rng64, verdict, nullptr, nullptr, true, weights64,
                        batch_out ? batch_out : bo);
}

// ============================================================================
// stand-alone inner-product proofs
// ============================================================================
// working set of the inner-product / linear / audit entry points (separate from the arena, which the MSMs they call claim):
// grown on demand, never shrunk; a call that grows it first waits for everything that may still read the old block
static int ipp_reserve(bpgpu_ctx *c, size_t need) {
    if (c->ipp_cap >= need) return BPGPU_OK;
    HIPCHK(c, hipDeviceSynchronize());
    if (c->ipp_buf) HIPCHK(c, hipFree(c->ipp_buf));
    c->ipp_buf = nullptr;
    c->ipp_cap = 0;
    if (hipMalloc((void **)&c->ipp_buf, need + need / 4) != hipSuccess) return fail(c, BPGPU_ERR_HIP, "out of device memory (%zu bytes of working set)", need + need / 4);
    c->ipp_cap = need + need / 4;
    return BPGPU_OK;
}
// what a front end leaves there for the multiscalar multiplication(s): the unique terms' scalars and points, the generator-table rows, its
// own status words, then the status bytes and the results of the multiplication(s)
struct front_staged {
    char *d_sc = nullptr, *d_pt = nullptr, *d_gen = nullptr, *d_stat = nullptr, *d_mst = nullptr, *d_out = nullptr;
    size_t sz_b = 0, sz_o = 0;   // the widths of d_mst and d_out
};
// ... carved in that order (the term lists `terms` bytes each), everything the front end writes zeroed: scalars, points, generator rows, status
static int front_stage_locked(bpgpu_ctx *c, hipStream_t s, size_t terms, size_t gen, size_t stat, size_t mst, size_t out, front_staged &stg) {
    const size_t sz_terms = align_up(terms), sz_gen = align_up(gen), sz_st = align_up(stat);
    stg.sz_b = align_up(mst), stg.sz_o = align_up(out);
    const int rc = ipp_reserve(c, 2 * sz_terms + sz_gen + sz_st + stg.sz_b + stg.sz_o);
    if (rc) return rc;
    stg.d_sc = c->ipp_buf, stg.d_pt = stg.d_sc + sz_terms, stg.d_gen = stg.d_pt + sz_terms, stg.d_stat = stg.d_gen + sz_gen, stg.d_mst = stg.d_stat + sz_st,
    stg.d_out = stg.d_mst + stg.sz_b;
    HIPCHK(c, hipMemsetAsync(stg.d_sc, 0, 2 * sz_terms + sz_gen + sz_st, s));
    return BPGPU_OK;
}

// Transcript::new(label) [or the caller's 208-byte state] followed by innerproduct_domain_sep(n) (transcript.rs:50-53): the
// batch-invariant prefix of the stand-alone inner-product and linear proofs, replayed once on the host
static void ipp_domain_sep_state(uint8_t st0[BPGPU_TRANSCRIPT_BYTES], const uint8_t *label, size_t label_len, const uint8_t *shared_ts, size_t n,
                                 rp_strobe_init *init) {
    if (shared_ts) memcpy(st0, shared_ts, BPGPU_TRANSCRIPT_BYTES);
    else bpgpu_transcript_new(label, label_len, st0);
    uint32_t w[50];
    strobe t;
    ts_to_strobe(t, w, st0);
    const uint8_t ipp[6] = {'i', 'p', 'p', ' ', 'v', '1'}, ln[1] = {'n'};
    merlin_append_message(t, DOM_SEP, 7, ipp, 6);
    merlin_append_u64(t, ln, 1, n);
    ts_from_strobe(st0, t);
    if (init) {
        memcpy(init->w, w, 200);
        init->pos = t.pos;
        init->pos_begin = t.pos_begin;
        init->cur_flags = t.cur_flags;
    }
}

// The callers' own transcripts of the bpgpu_ipp_*_ts / bpgpu_linear_*_ts entry points: states BEFORE innerproduct_domain_sep(n), which the
// lanes apply themselves (ipp.h: ipp_ts_start).  One state for every proof -- `shared` (host memory, handed to the kernels by value), or
// d_in with stride 0 -- or one per proof (d_in, stride BP_TS_WORDS).  With an ipp_ts the label / shared_ts arguments are not looked at.
struct ipp_ts {
    const uint8_t *shared = nullptr;
    const void *d_in = nullptr;
    uint32_t stride = 0;       // words between the states at d_in
    void *d_out = nullptr;     // nbatch states (optional; the inner-product calls only: the linear ones have had a d_ts_out all along)
};
static void ipp_ts_init(rp_strobe_init &init, const ipp_ts &ts) {
    memset(&init, 0, sizeof init);
    if (ts.shared) strobe_init_from_state(init, ts.shared);
}
// the argument checks of the host forms: every state is looked at before anything is staged
static int ipp_ts_host_args(bpgpu_ctx *c, const uint8_t *transcripts, size_t transcript_stride, size_t nbatch) {
    if (!transcripts || (transcript_stride != 0 && transcript_stride != BPGPU_TRANSCRIPT_BYTES))
        return fail(c, BPGPU_ERR_INVALID_ARG, "transcripts missing, or transcript_stride neither 0 nor BPGPU_TRANSCRIPT_BYTES");
    for (size_t b = 0; b < (transcript_stride ? nbatch : 1); b++)
        if (!ts_state_ok(transcripts + b * BPGPU_TRANSCRIPT_BYTES)) return fail(c, BPGPU_ERR_INVALID_ARG, "malformed transcript state %zu", b);
    return BPGPU_OK;
}
// ... and the staged copy as the kernels take it
static ipp_ts ipp_ts_staged(const void *d_in, size_t transcript_stride) {
    ipp_ts ts;
    ts.d_in = d_in;
    ts.stride = transcript_stride ? BP_TS_WORDS : 0;
    return ts;
}
// ... and of the _dev forms: one checked host state or nbatch device states (which the lanes guard themselves)
static int ipp_ts_dev_args(bpgpu_ctx *c, const uint8_t *shared_transcript, const void *d_transcripts, const void *d_transcripts_out, ipp_ts &ts) {
    if ((shared_transcript != nullptr) == (d_transcripts != nullptr))
        return fail(c, BPGPU_ERR_INVALID_ARG, "give exactly one of shared_transcript / d_transcripts");
    if (shared_transcript && !ts_state_ok(shared_transcript)) return fail(c, BPGPU_ERR_INVALID_ARG, "malformed transcript state");
    if (((uintptr_t)d_transcripts | (uintptr_t)d_transcripts_out) & 3) return fail(c, BPGPU_ERR_INVALID_ARG, "device buffers must be 4-byte aligned");
    ts.shared = shared_transcript;
    ts.d_in = d_transcripts;
    ts.stride = BP_TS_WORDS;
    return BPGPU_OK;
}

static int ipp_verify_dev_locked(bpgpu_ctx *c, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len, const uint8_t *label,
                                 size_t label_len, const uint8_t *shared_ts, const void *d_Gf, const void *d_Hf, const void *d_P,
                                 const void *d_Q, const void *d_G, const void *d_H, int bases_shared, void *d_verdict, void *d_msm_out,
                                 hipStream_t s, const ipp_ts *ts = nullptr) {
    if (nbatch > 0x7fffffffu / 64) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large");
    if (!ts && shared_ts && !ts_state_ok(shared_ts)) return fail(c, BPGPU_ERR_INVALID_ARG, "malformed transcript state");
    const uint32_t nb32 = (uint32_t)nbatch;
    rp_strobe_init init;
    if (ts) ipp_ts_init(init, *ts);
    // InnerProductProof::from_bytes, length part (ipp.rs:374-388)
    size_t k = 0;
    bool fmt = false;
    if (proof_len % 32 != 0) fmt = true;
    else {
        const size_t ne = proof_len / 32;
        if (ne < 2 || (ne - 2) % 2 != 0) fmt = true;
        else {
            k = (ne - 2) / 2;
            if (k >= 32) fmt = true;
        }
    }
    if (fmt) {
        HIPCHK(c, hipMemsetAsync(d_verdict, BPGPU_VERDICT_FORMAT_ERROR, nbatch, s));
        if (d_msm_out) HIPCHK(c, hipMemsetAsync(d_msm_out, 0, nbatch * 32, s));
        if (ts && ts->d_out)   // from_bytes rejects every proof: the callers' states go back as they came
            LAUNCH(c, s, "ipp_ts_input", k_ipp_ts_input, (nb32 + 63) / 64, 64, nb32, init, (const uint32_t *)ts->d_in, ts->stride, (uint32_t *)ts->d_out);
        return BPGPU_OK;
    }
    ipp_shape sh;
    sh.n = (uint32_t)n;
    sh.k = (uint32_t)k;
    sh.proof_len = (uint32_t)proof_len;
    sh.nproofs = (uint32_t)nbatch;
    sh.bases_shared = bases_shared ? 1u : 0u;
    if (n == ((size_t)1 << k) && k > BP_RP_MAX_K) return fail(c, BPGPU_ERR_INVALID_ARG, "n > 2^%d not supported", BP_RP_MAX_K);
    sh.shape_verdict = (n == ((size_t)1 << k)) ? 0 : BPGPU_VERDICT_VERIFICATION_ERROR;   // ipp.rs:203-211
    const size_t n_eff = sh.shape_verdict ? 0 : n;
    sh.N = (uint32_t)(2 * n_eff + 2 * (sh.shape_verdict ? 0 : k) + 2);
    if (sh.shape_verdict) sh.n = 0;   // only the canonical-scalar check runs
    const size_t N = sh.N;
    if ((uint64_t)nbatch * N > 0x7fffffffull / 64) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large for this shape");
    // scratch: the (scalar, point) term lists, front-end status, MSM status / result; own allocation because the MSM below
    // claims the arena
    const size_t sz_terms = align_up(nbatch * N * 32 + 64), sz_st = align_up(nbatch * 4), sz_b = align_up(nbatch + 64), sz_o = align_up(nbatch * 32 + 64);
    const size_t need = 2 * sz_terms + sz_st + sz_b + sz_o;
    {
        const int rcr = ipp_reserve(c, need);
        if (rcr) return rcr;
    }
    char *d_sc = c->ipp_buf, *d_pt = d_sc + sz_terms, *d_stat = d_pt + sz_terms, *d_mst = d_stat + sz_st, *d_out = d_mst + sz_b;
    HIPCHK(c, hipMemsetAsync(d_sc, 0, 2 * sz_terms + sz_st, s));   // scalars, points, status
    if (ts) {
        LAUNCH(c, s, "ipp_prepare_ts", k_ipp_prepare_ts, (nb32 + RP_BLOCK - 1) / RP_BLOCK, RP_BLOCK, sh, init, (const uint8_t *)d_proofs, (const uint8_t *)d_Gf,
               (const uint8_t *)d_Hf, (const uint8_t *)d_P, (const uint8_t *)d_Q, (const uint8_t *)d_G, (const uint8_t *)d_H, (uint32_t *)d_sc,
               (uint32_t *)d_pt, (uint32_t *)d_stat, (const uint32_t *)ts->d_in, ts->stride, (uint32_t *)ts->d_out);
    } else {
        uint8_t st0[BPGPU_TRANSCRIPT_BYTES];
        ipp_domain_sep_state(st0, label, label_len, shared_ts, n, &init);
        LAUNCH(c, s, "ipp_prepare", k_ipp_prepare, (nb32 + RP_BLOCK - 1) / RP_BLOCK, RP_BLOCK, sh, init, (const uint8_t *)d_proofs, (const uint8_t *)d_Gf,
               (const uint8_t *)d_Hf, (const uint8_t *)d_P, (const uint8_t *)d_Q, (const uint8_t *)d_G, (const uint8_t *)d_H, (uint32_t *)d_sc,
               (uint32_t *)d_pt, (uint32_t *)d_stat);
    }
    std::vector<uint32_t> nt(nbatch, (uint32_t)N);
    int rc = msm_batch_dev_locked(c, nbatch, nt.data(), d_sc, d_pt, d_out, d_mst, s);
    if (rc) return rc;
    LAUNCH(c, s, "ipp_verdict", k_ipp_verdict, (nb32 + 63) / 64, 64, nb32, (const uint32_t *)d_stat, (const uint8_t *)d_mst, (const uint32_t *)d_out,
           (uint8_t *)d_verdict);
    if (d_msm_out) HIPCHK(c, hipMemcpyAsync(d_msm_out, d_out, nbatch * 32, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipGetLastError());
    return BPGPU_OK;
}

extern "C" int bpgpu_ipp_verify_batch_dev(bpgpu_ctx *c, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len, const uint8_t *label,
                                          size_t label_len, const uint8_t *shared_transcript, const void *d_G_factors, const void *d_H_factors,
                                          const void *d_P, const void *d_Q, const void *d_G, const void *d_H, int bases_shared, void *d_verdict,
                                          void *d_msm_out, void *stream) {
    if (!c || (label_len && !label)) return BPGPU_ERR_INVALID_ARG;
    if (nbatch == 0) return BPGPU_OK;
    if (!d_proofs || !d_verdict || !d_P || !d_Q || (n && (!d_G_factors || !d_H_factors || !d_G || !d_H))) return BPGPU_ERR_INVALID_ARG;
    if (((uintptr_t)d_proofs | (uintptr_t)d_G_factors | (uintptr_t)d_H_factors | (uintptr_t)d_P | (uintptr_t)d_Q | (uintptr_t)d_G | (uintptr_t)d_H) & 3)
        return fail(c, BPGPU_ERR_INVALID_ARG, "device buffers must be 4-byte aligned");
    return dev_call(c, stream, [&](hipStream_t s) {
        return ipp_verify_dev_locked(c, n, nbatch, d_proofs, proof_len, label, label_len, shared_transcript, d_G_factors, d_H_factors, d_P, d_Q, d_G, d_H,
                                   bases_shared, d_verdict, d_msm_out, s);
    });
}

// InnerProductProof::from_bytes + verification_scalars (ipp.rs:198-253, 373-407) for nbatch proofs, host pointers
extern "C" int bpgpu_ipp_verification_scalars(bpgpu_ctx *c, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len, const uint8_t *label,
                                              size_t label_len, const uint8_t *transcripts, size_t transcript_stride, uint8_t *u_sq, uint8_t *u_inv_sq,
                                              uint8_t *s_out, uint8_t *transcripts_out, uint8_t *status) {
    if (!c || (label_len && !label)) return BPGPU_ERR_INVALID_ARG;
    if (nbatch == 0) return BPGPU_OK;
    if (!proofs || !status || !u_sq || !u_inv_sq || (n && !s_out)) return BPGPU_ERR_INVALID_ARG;
    if (transcripts && transcript_stride != 0 && transcript_stride != BPGPU_TRANSCRIPT_BYTES)
        return fail(c, BPGPU_ERR_INVALID_ARG, "transcript_stride neither 0 nor BPGPU_TRANSCRIPT_BYTES");
    const bool per_proof = transcripts && transcript_stride;
    if (transcripts)
        for (size_t b = 0; b < (per_proof ? nbatch : 1); b++)
            if (!ts_state_ok(transcripts + b * BPGPU_TRANSCRIPT_BYTES)) return fail(c, BPGPU_ERR_INVALID_ARG, "malformed transcript state %zu", b);
    // InnerProductProof::from_bytes, length part (ipp.rs:374-388)
    size_t k = 0;
    bool fmt = proof_len % 32 != 0;
    if (!fmt) {
        const size_t ne = proof_len / 32;
        if (ne < 2 || (ne - 2) % 2 != 0) fmt = true;
        else {
            k = (ne - 2) / 2;
            if (k >= 32) fmt = true;
        }
    }
    // the caller's transcript as it is handed back when nothing was absorbed: from_bytes failed, or n != 2^k (ipp.rs:203-211 returns before
    // innerproduct_domain_sep)
    uint8_t st_start[BPGPU_TRANSCRIPT_BYTES];
    if (transcripts && !per_proof) memcpy(st_start, transcripts, BPGPU_TRANSCRIPT_BYTES);
    else if (!transcripts) bpgpu_transcript_new(label, label_len, st_start);
    auto untouched = [&](size_t b) {
        if (transcripts_out) memcpy(transcripts_out + b * BPGPU_TRANSCRIPT_BYTES, per_proof ? transcripts + b * BPGPU_TRANSCRIPT_BYTES : st_start, BPGPU_TRANSCRIPT_BYTES);
    };
    if (fmt) {
        memset(status, BPGPU_VERDICT_FORMAT_ERROR, nbatch);
        for (size_t b = 0; b < nbatch; b++) untouched(b);
        return BPGPU_OK;
    }
    const bool shape_bad = n != ((size_t)1 << k);   // ipp.rs:203-211 (k >= 32 was refused above)
    if (!shape_bad && k > BP_RP_MAX_K) return fail(c, BPGPU_ERR_INVALID_ARG, "n > 2^%d not supported", BP_RP_MAX_K);
    if ((uint64_t)nbatch * (n ? n : 1) > 0x7fffffffull / 64) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large for this shape");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    ipp_shape sh;
    sh.n = (uint32_t)n;
    sh.k = (uint32_t)k;
    sh.N = 0;
    sh.proof_len = (uint32_t)proof_len;
    sh.nproofs = (uint32_t)nbatch;
    sh.shape_verdict = shape_bad ? BPGPU_VERDICT_VERIFICATION_ERROR : 0;
    sh.bases_shared = 0;
    const size_t n_eff = shape_bad ? 0 : n, TS = BPGPU_TRANSCRIPT_BYTES;
    hipStream_t s = c->stream;
    host_call<bpgpu_ctx> io(c, s);
    const int r_pr = io.in(nbatch * proof_len + 64), r_ti = io.in(per_proof ? nbatch * TS : 0);
    const int r_us = io.out(nbatch * (k ? k : 1) * 32), r_ui = io.out(nbatch * (k ? k : 1) * 32), r_s = io.out(nbatch * (n_eff ? n_eff : 1) * 32),
              r_to = io.out(transcripts_out ? nbatch * TS : 0), r_st = io.out(nbatch * 4);
    const int r_tab = io.dev(nbatch * (k ? k : 1) * 2 * 40);
    int rc = io.open();
    do {
        if (rc) break;
        char *d_pr = io.d(r_pr), *d_ti = io.d(r_ti), *d_us = io.d(r_us), *d_ui = io.d(r_ui), *d_s = io.d(r_s), *d_to = io.d(r_to), *d_st = io.d(r_st), *d_tab = io.d(r_tab);
        io.put(r_pr, proofs, nbatch * proof_len);
        if (per_proof) io.put(r_ti, transcripts, nbatch * TS);
        if (io.upload() || hipMemsetAsync(d_us, 0, io.out_bytes(), s) != hipSuccess) {
            rc = fail(c, BPGPU_ERR_HIP, "staging failed");
            break;
        }
        rp_strobe_init init;
        memset(&init, 0, sizeof init);
        if (!per_proof) {   // one start state: innerproduct_domain_sep(n) replayed once on the host
            uint8_t st0[BPGPU_TRANSCRIPT_BYTES];
            ipp_domain_sep_state(st0, label, label_len, transcripts, n, &init);
        }
        const uint32_t nb32 = (uint32_t)nbatch;
        LAUNCH(c, s, "ipp_vs_front", k_ipp_vs_front, (nb32 + RP_BLOCK - 1) / RP_BLOCK, RP_BLOCK, sh, init, (const uint8_t *)d_pr, per_proof ? (const uint32_t *)d_ti : (const uint32_t *)nullptr,
               (uint32_t *)d_us, (uint32_t *)d_ui, (uint32_t *)d_tab, transcripts_out ? (uint32_t *)d_to : (uint32_t *)nullptr, (uint32_t *)d_st);
        if (n_eff) {
            const uint32_t nt = (uint32_t)(n_eff * nbatch);
            LAUNCH(c, s, "ipp_vs_s", k_ipp_vs_s, (nt + 63) / 64, 64, nt, sh, (const uint32_t *)d_tab, (const uint32_t *)d_st, (uint32_t *)d_s);
        }
        rc = io.download(0);
    } while (0);
    rc = io.finish(rc);
    if (rc) return rc;
    memcpy(u_sq, io.h(r_us), nbatch * k * 32);
    memcpy(u_inv_sq, io.h(r_ui), nbatch * k * 32);
    if (n_eff) memcpy(s_out, io.h(r_s), nbatch * n_eff * 32);
    if (transcripts_out) memcpy(transcripts_out, io.h(r_to), nbatch * TS);
    const uint32_t *st32 = (const uint32_t *)io.h(r_st);
    for (size_t b = 0; b < nbatch; b++) {
        status[b] = (uint8_t)st32[b];
        // (with one start state for the batch the device replays from the state BEHIND the domain separator: where the reference never
        // got that far, the caller's state goes back as it came)
        if (status[b] == BPGPU_VERDICT_FORMAT_ERROR || shape_bad) untouched(b);
    }
    return BPGPU_OK;
}

// host pointers.  ts_host (with ts_stride 0 or BPGPU_TRANSCRIPT_BYTES): the callers' own transcripts, checked by the caller, in place of the label
static int ipp_verify_host_call(bpgpu_ctx *c, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len, const uint8_t *label, size_t label_len,
                                const uint8_t *ts_host, size_t ts_stride, const uint8_t *G_factors, const uint8_t *H_factors, const uint8_t *P,
                                const uint8_t *Q, const uint8_t *G, const uint8_t *H, int bases_shared, uint8_t *verdict, uint8_t *msm_out,
                                uint8_t *ts_out_host) {
    if (nbatch == 0) return BPGPU_OK;
    if (!proofs || !verdict || !P || !Q || (n && (!G_factors || !H_factors || !G || !H))) return BPGPU_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    host_call<bpgpu_ctx> io(c, s);
    const size_t TS = BPGPU_TRANSCRIPT_BYTES, nb_g = bases_shared ? 1 : nbatch, nstates = !ts_host ? 0 : ts_stride ? nbatch : 1;
    const size_t b_f = nbatch * n * 32 + 64, b_g = nb_g * n * 32 + 64, b_pq = nbatch * 32 + 64;
    const int r_pr = io.in(nbatch * proof_len + 64), r_gf = io.in(b_f), r_hf = io.in(b_f), r_g = io.in(b_g), r_h = io.in(b_g), r_p = io.in(b_pq), r_q = io.in(b_pq),
              r_ti = io.in(nstates * TS);
    const int r_v = io.out(nbatch), r_o = io.out(nbatch * 32), r_to = io.out(ts_out_host ? nbatch * TS : 0);
    int rc = io.open();
    if (rc) return rc;
    io.put(r_pr, proofs, nbatch * proof_len);
    if (n) {
        io.put(r_gf, G_factors, nbatch * n * 32);
        io.put(r_hf, H_factors, nbatch * n * 32);
        io.put(r_g, G, nb_g * n * 32);
        io.put(r_h, H, nb_g * n * 32);
    }
    io.put(r_p, P, nbatch * 32);
    io.put(r_q, Q, nbatch * 32);
    ipp_ts ts;
    if (ts_host) {
        io.put(r_ti, ts_host, nstates * TS);
        ts.d_in = io.d(r_ti);
        ts.stride = ts_stride ? BP_TS_WORDS : 0;
        ts.d_out = ts_out_host ? io.d(r_to) : nullptr;
    }
    rc = io.upload();
    if (!rc)
        rc = ipp_verify_dev_locked(c, n, nbatch, io.d(r_pr), proof_len, label, label_len, nullptr, io.d(r_gf), io.d(r_hf), io.d(r_p), io.d(r_q), io.d(r_g), io.d(r_h),
                                   bases_shared, io.d(r_v), io.d(r_o), s, ts_host ? &ts : nullptr);
    rc = io.finish(io.download(rc));
    if (rc) return rc;
    memcpy(verdict, io.h(r_v), nbatch);
    if (msm_out) memcpy(msm_out, io.h(r_o), nbatch * 32);
    if (ts_out_host) memcpy(ts_out_host, io.h(r_to), nbatch * TS);
    return BPGPU_OK;
}

extern "C" int bpgpu_ipp_verify_batch(bpgpu_ctx *c, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len, const uint8_t *label,
                                      size_t label_len, const uint8_t *G_factors, const uint8_t *H_factors, const uint8_t *P,
                                      const uint8_t *Q, const uint8_t *G, const uint8_t *H, uint8_t *verdict, uint8_t *msm_out) {
    if (!c || (label_len && !label)) return BPGPU_ERR_INVALID_ARG;
    return ipp_verify_host_call(c, n, nbatch, proofs, proof_len, label, label_len, nullptr, 0, G_factors, H_factors, P, Q, G, H, 0, verdict, msm_out, nullptr);
}

// ---- the same verification on the callers' own transcripts (ipp.h: ipp_prepare_lane<true>) ----
extern "C" int bpgpu_ipp_verify_batch_ts(bpgpu_ctx *c, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len, const uint8_t *transcripts,
                                         size_t transcript_stride, const uint8_t *G_factors, const uint8_t *H_factors, const uint8_t *P,
                                         const uint8_t *Q, const uint8_t *G, const uint8_t *H, int bases_shared, uint8_t *verdict, uint8_t *msm_out,
                                         uint8_t *transcripts_out) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    const int rca = ipp_ts_host_args(c, transcripts, transcript_stride, nbatch);
    if (rca) return rca;
    return ipp_verify_host_call(c, n, nbatch, proofs, proof_len, nullptr, 0, transcripts, transcript_stride, G_factors, H_factors, P, Q, G, H, bases_shared,
                                verdict, msm_out, transcripts_out);
}

extern "C" int bpgpu_ipp_verify_batch_ts_dev(bpgpu_ctx *c, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len, const uint8_t *shared_transcript,
                                             const void *d_transcripts, const void *d_G_factors, const void *d_H_factors, const void *d_P,
                                             const void *d_Q, const void *d_G, const void *d_H, int bases_shared, void *d_verdict, void *d_msm_out,
                                             void *d_transcripts_out, void *stream) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    ipp_ts ts;
    const int rca = ipp_ts_dev_args(c, shared_transcript, d_transcripts, d_transcripts_out, ts);
    if (rca) return rca;
    ts.d_out = d_transcripts_out;
    if (nbatch == 0) return BPGPU_OK;
    if (!d_proofs || !d_verdict || !d_P || !d_Q || (n && (!d_G_factors || !d_H_factors || !d_G || !d_H))) return BPGPU_ERR_INVALID_ARG;
    if (((uintptr_t)d_proofs | (uintptr_t)d_G_factors | (uintptr_t)d_H_factors | (uintptr_t)d_P | (uintptr_t)d_Q | (uintptr_t)d_G | (uintptr_t)d_H) & 3)
        return fail(c, BPGPU_ERR_INVALID_ARG, "device buffers must be 4-byte aligned");
    return dev_call(c, stream, [&](hipStream_t s) {
        return ipp_verify_dev_locked(c, n, nbatch, d_proofs, proof_len, nullptr, 0, nullptr, d_G_factors, d_H_factors, d_P, d_Q, d_G, d_H, bases_shared, d_verdict,
                                   d_msm_out, s, &ts);
    });
}

// what the front end of a LinearProof batch leaves on the device (c->ipp_buf) for its multiscalar multiplication(s): its own order
// (the generator rows last, and only in generator-table mode)
struct lin_staged : front_staged {
    lin_shape sh;
    bool fmt = false;     // proof_len is not a LinearProof length: nothing was launched, every proof is a FormatError
    bool fixed = false;   // generator-table mode
    const void *d_G = nullptr, *d_F = nullptr, *d_B = nullptr;   // the bases in use (the context's generators in generator-table mode)
};

// LinearProof::from_bytes' length part, the staging and the k_lin_prepare launch (lane = proof) of nbatch proofs
static int lin_front_dev_locked(bpgpu_ctx *c, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len, const uint8_t *label,
                                size_t label_len, const uint8_t *shared_ts, const void *d_C, const void *d_G, const void *d_F,
                                const void *d_B, const void *d_b, int b_shared, void *d_ts_out, hipStream_t s, lin_staged &stg,
                                const ipp_ts *ts = nullptr) {
    if (nbatch > 0x7fffffffu / 64) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large");
    if (!ts && shared_ts && !ts_state_ok(shared_ts)) return fail(c, BPGPU_ERR_INVALID_ARG, "malformed transcript state");
    // LinearProof::from_bytes, length part (linear_proof.rs:350-366)
    size_t k = 0;
    bool fmt = false;
    if (proof_len % 32 != 0) fmt = true;
    else {
        const size_t ne = proof_len / 32;
        if (ne < 3 || (ne - 3) % 2 != 0) fmt = true;
        else {
            k = (ne - 3) / 2;
            if (k >= 32) fmt = true;
        }
    }
    if (fmt) {
        if (d_ts_out) return fail(c, BPGPU_ERR_INVALID_ARG, "proof_len is not a LinearProof length: no transcripts to return");
        stg.fmt = true;
        return BPGPU_OK;
    }
    lin_shape &sh = stg.sh;
    sh.n = (uint32_t)n;
    sh.k = (uint32_t)k;
    sh.proof_len = (uint32_t)proof_len;
    sh.nproofs = (uint32_t)nbatch;
    sh.b_shared = b_shared ? 1u : 0u;
    if (n == ((size_t)1 << k) && k > BP_RP_MAX_K) return fail(c, BPGPU_ERR_INVALID_ARG, "n > 2^%d not supported", BP_RP_MAX_K);
    sh.shape_verdict = (n == ((size_t)1 << k)) ? 0 : BPGPU_VERDICT_VERIFICATION_ERROR;   // linear_proof.rs:263-265
    if (sh.shape_verdict) sh.n = 0;   // only the canonical-scalar check runs
    // generator-table mode: G, F, B not given = the context's bp_gens.share(0).G(n), pc_gens.B, pc_gens.B_blinding (what the
    // reference's own callers pass, linear_proof.rs:405-411): their n + 2 coefficients go through the window tables
    const bool fixed = d_G == nullptr && d_F == nullptr && d_B == nullptr;
    if (fixed) {
        if (!c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
        if (!sh.shape_verdict && n > c->gens_capacity) return fail(c, BPGPU_ERR_NO_GENS, "InvalidGeneratorsLength: generators too small for n=%zu", n);
        d_G = c->d_gens + 2 * 8;
        d_F = c->d_gens + 8;
        d_B = c->d_gens;
    }
    sh.fixed = fixed ? 1u : 0u;
    sh.N = (uint32_t)(fixed ? 2 * k + 2 : sh.shape_verdict ? 4 : n + 2 * k + 4);
    const size_t N = sh.N;
    if ((uint64_t)nbatch * (n + 2 * k + 4) > 0x7fffffffull / 64) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large for this shape");
    const size_t sz_terms = align_up(nbatch * N * 32 + 64), sz_st = align_up(nbatch * 4), sz_b = align_up(nbatch + 64), sz_o = align_up(nbatch * 32 + 64);
    const size_t sz_gen = fixed ? align_up(nbatch * (sh.n + 2) * 32 + 64) : 0;
    const size_t need = 2 * sz_terms + sz_st + sz_b + sz_o + sz_gen;
    {
        const int rcr = ipp_reserve(c, need);
        if (rcr) return rcr;
    }
    char *d_sc = c->ipp_buf, *d_pt = d_sc + sz_terms, *d_stat = d_pt + sz_terms, *d_mst = d_stat + sz_st, *d_out = d_mst + sz_b;
    char *d_gen = fixed ? d_out + sz_o : nullptr;
    HIPCHK(c, hipMemsetAsync(d_sc, 0, 2 * sz_terms + sz_st, s));   // scalars, points, status
    if (fixed) HIPCHK(c, hipMemsetAsync(d_gen, 0, sz_gen, s));
    rp_strobe_init init;
    const uint32_t nb32 = (uint32_t)nbatch;
    if (ts) {
        ipp_ts_init(init, *ts);
        LAUNCH(c, s, "lin_prepare_ts", k_lin_prepare_ts, (nb32 + RP_BLOCK - 1) / RP_BLOCK, RP_BLOCK, sh, init, (const uint8_t *)d_proofs, (const uint8_t *)d_C,
               (const uint8_t *)d_b, (const uint8_t *)d_G, (const uint8_t *)d_F, (const uint8_t *)d_B, (uint32_t *)d_sc, (uint32_t *)d_pt,
               (uint32_t *)d_stat, (uint32_t *)d_ts_out, (uint32_t *)d_gen, (const uint32_t *)ts->d_in, ts->stride, (uint32_t)n);
    } else {
        uint8_t st0[BPGPU_TRANSCRIPT_BYTES];
        ipp_domain_sep_state(st0, label, label_len, shared_ts, n, &init);
        LAUNCH(c, s, "lin_prepare", k_lin_prepare, (nb32 + RP_BLOCK - 1) / RP_BLOCK, RP_BLOCK, sh, init, (const uint8_t *)d_proofs, (const uint8_t *)d_C,
               (const uint8_t *)d_b, (const uint8_t *)d_G, (const uint8_t *)d_F, (const uint8_t *)d_B, (uint32_t *)d_sc, (uint32_t *)d_pt,
               (uint32_t *)d_stat, (uint32_t *)d_ts_out, (uint32_t *)d_gen);
    }
    stg.fixed = fixed;
    stg.d_sc = d_sc, stg.d_pt = d_pt, stg.d_stat = d_stat, stg.d_mst = d_mst, stg.d_out = d_out, stg.d_gen = d_gen;
    stg.d_G = d_G, stg.d_F = d_F, stg.d_B = d_B;
    stg.sz_b = sz_b, stg.sz_o = sz_o;
    return BPGPU_OK;
}

// LinearProof::verify for nbatch proofs (linear.h): front end (lane = proof) -> bpgpu_msm_batch's MSM -> verdicts.
// G (n encodings), F, B are shared by the batch; b is per proof unless b_shared.
static int lin_verify_dev_locked(bpgpu_ctx *c, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len, const uint8_t *label,
                                 size_t label_len, const uint8_t *shared_ts, const void *d_C, const void *d_G, const void *d_F,
                                 const void *d_B, const void *d_b, int b_shared, void *d_verdict, void *d_msm_out, void *d_ts_out,
                                 hipStream_t s, const ipp_ts *ts = nullptr) {
    lin_staged stg;
    int rc = lin_front_dev_locked(c, n, nbatch, d_proofs, proof_len, label, label_len, shared_ts, d_C, d_G, d_F, d_B, d_b, b_shared, d_ts_out, s, stg, ts);
    if (rc) return rc;
    if (stg.fmt) {
        HIPCHK(c, hipMemsetAsync(d_verdict, BPGPU_VERDICT_FORMAT_ERROR, nbatch, s));
        if (d_msm_out) HIPCHK(c, hipMemsetAsync(d_msm_out, 0, nbatch * 32, s));
        return BPGPU_OK;
    }
    const lin_shape &sh = stg.sh;
    const bool fixed = stg.fixed;
    const size_t N = sh.N, sz_b = stg.sz_b, sz_o = stg.sz_o;
    const uint32_t nb32 = (uint32_t)nbatch;
    char *d_sc = stg.d_sc, *d_pt = stg.d_pt, *d_stat = stg.d_stat, *d_mst = stg.d_mst, *d_out = stg.d_out, *d_gen = stg.d_gen;
    if (fixed && sh.shape_verdict) {      // nothing to multiply: every proof already carries its verdict
        HIPCHK(c, hipMemsetAsync(d_mst, 0, sz_b + sz_o, s));
        rc = BPGPU_OK;
    } else if (fixed) {
        rc = msm_shared_dev_locked(c, n, 1, nbatch, N, d_gen, d_sc, d_pt, d_out, d_mst, nullptr, s, true);
    } else {
        std::vector<uint32_t> nt(nbatch, (uint32_t)N);
        rc = msm_batch_dev_locked(c, nbatch, nt.data(), d_sc, d_pt, d_out, d_mst, s);
    }
    if (rc) return rc;
    LAUNCH(c, s, "lin_verdict", k_ipp_verdict, (nb32 + 63) / 64, 64, nb32, (const uint32_t *)d_stat, (const uint8_t *)d_mst, (const uint32_t *)d_out,
           (uint8_t *)d_verdict);
    if (d_msm_out) HIPCHK(c, hipMemcpyAsync(d_msm_out, d_out, nbatch * 32, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipGetLastError());
    return BPGPU_OK;
}

extern "C" int bpgpu_linear_verify_batch_dev(bpgpu_ctx *c, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len, const uint8_t *label,
                                             size_t label_len, const uint8_t *shared_transcript, const void *d_C, const void *d_G,
                                             const void *d_F, const void *d_B, const void *d_b, int b_shared, void *d_verdict, void *d_msm_out,
                                             void *d_transcripts_out, void *stream) {
    if (!c || (label_len && !label)) return BPGPU_ERR_INVALID_ARG;
    if (nbatch == 0) return BPGPU_OK;
    const bool from_gens = !d_G && !d_F && !d_B;
    if (!d_proofs || !d_verdict || !d_C || (n && !d_b) || (!from_gens && (!d_F || !d_B || (n && !d_G)))) return BPGPU_ERR_INVALID_ARG;
    if (((uintptr_t)d_proofs | (uintptr_t)d_C | (uintptr_t)d_G | (uintptr_t)d_F | (uintptr_t)d_B | (uintptr_t)d_b | (uintptr_t)d_transcripts_out) & 3)
        return fail(c, BPGPU_ERR_INVALID_ARG, "device buffers must be 4-byte aligned");
    return dev_call(c, stream, [&](hipStream_t s) {
        return lin_verify_dev_locked(c, n, nbatch, d_proofs, proof_len, label, label_len, shared_transcript, d_C, d_G, d_F, d_B, d_b, b_shared, d_verdict,
                                   d_msm_out, d_transcripts_out, s);
    });
}

// host pointers.  ts_host (with ts_stride 0 or BPGPU_TRANSCRIPT_BYTES): the callers' own transcripts, checked by the caller, in place of label /
// shared_transcript
static int lin_verify_host_call(bpgpu_ctx *c, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len, const uint8_t *label, size_t label_len,
                                const uint8_t *shared_transcript, const uint8_t *ts_host, size_t ts_stride, const uint8_t *C, const uint8_t *G,
                                const uint8_t *F, const uint8_t *B, const uint8_t *b, int b_shared, uint8_t *verdict, uint8_t *msm_out,
                                uint8_t *transcripts_out) {
    if (nbatch == 0) return BPGPU_OK;
    const bool from_gens = !G && !F && !B;
    if (!proofs || !verdict || !C || (n && !b) || (!from_gens && (!F || !B || (n && !G)))) return BPGPU_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nb_b = b_shared ? 1 : nbatch;
    hipStream_t s = c->stream;
    host_call<bpgpu_ctx> io(c, s);
    const size_t nstates = !ts_host ? 0 : ts_stride ? nbatch : 1;
    const int r_pr = io.in(nbatch * proof_len + 64), r_c = io.in(nbatch * 32 + 64), r_g = io.in(n * 32 + 64), r_fb = io.in(64 + 64), r_bv = io.in(nb_b * n * 32 + 64),
              r_ti = io.in(nstates * BPGPU_TRANSCRIPT_BYTES);
    const int r_v = io.out(nbatch), r_o = io.out(nbatch * 32), r_t = io.out(transcripts_out ? nbatch * BPGPU_TRANSCRIPT_BYTES : 0);
    int rc = io.open();
    if (rc) return rc;
    io.put(r_pr, proofs, nbatch * proof_len);
    io.put(r_c, C, nbatch * 32);
    if (n) {
        if (!from_gens) io.put(r_g, G, n * 32);
        io.put(r_bv, b, nb_b * n * 32);
    }
    if (!from_gens) {
        memcpy(io.h(r_fb), F, 32);
        memcpy(io.h(r_fb) + 32, B, 32);
    }
    ipp_ts ts;
    if (ts_host) {
        io.put(r_ti, ts_host, nstates * BPGPU_TRANSCRIPT_BYTES);
        ts.d_in = io.d(r_ti);
        ts.stride = ts_stride ? BP_TS_WORDS : 0;
    }
    rc = io.upload();
    if (!rc)
        rc = lin_verify_dev_locked(c, n, nbatch, io.d(r_pr), proof_len, label, label_len, shared_transcript, io.d(r_c), from_gens ? nullptr : io.d(r_g),
                                   from_gens ? nullptr : io.d(r_fb), from_gens ? nullptr : io.d(r_fb) + 32, io.d(r_bv), b_shared, io.d(r_v), io.d(r_o),
                                   transcripts_out ? io.d(r_t) : nullptr, s, ts_host ? &ts : nullptr);
    rc = io.finish(io.download(rc));
    if (rc) return rc;
    memcpy(verdict, io.h(r_v), nbatch);
    if (msm_out) memcpy(msm_out, io.h(r_o), nbatch * 32);
    if (transcripts_out) memcpy(transcripts_out, io.h(r_t), nbatch * BPGPU_TRANSCRIPT_BYTES);
    return BPGPU_OK;
}

extern "C" int bpgpu_linear_verify_batch(bpgpu_ctx *c, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len, const uint8_t *label,
                                         size_t label_len, const uint8_t *shared_transcript, const uint8_t *C, const uint8_t *G, const uint8_t *F,
                                         const uint8_t *B, const uint8_t *b, int b_shared, uint8_t *verdict, uint8_t *msm_out,
                                         uint8_t *transcripts_out) {
    if (!c || (label_len && !label)) return BPGPU_ERR_INVALID_ARG;
    return lin_verify_host_call(c, n, nbatch, proofs, proof_len, label, label_len, shared_transcript, nullptr, 0, C, G, F, B, b, b_shared, verdict, msm_out,
                                transcripts_out);
}

// ---- the same verification on the callers' own transcripts (linear.h: lin_prepare_lane<true>) ----
extern "C" int bpgpu_linear_verify_batch_ts(bpgpu_ctx *c, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len, const uint8_t *transcripts,
                                            size_t transcript_stride, const uint8_t *C, const uint8_t *G, const uint8_t *F, const uint8_t *B,
                                            const uint8_t *b, int b_shared, uint8_t *verdict, uint8_t *msm_out, uint8_t *transcripts_out) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    const int rca = ipp_ts_host_args(c, transcripts, transcript_stride, nbatch);
    if (rca) return rca;
    return lin_verify_host_call(c, n, nbatch, proofs, proof_len, nullptr, 0, nullptr, transcripts, transcript_stride, C, G, F, B, b, b_shared, verdict, msm_out,
                                transcripts_out);
}

extern "C" int bpgpu_linear_verify_batch_ts_dev(bpgpu_ctx *c, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len,
                                                const uint8_t *shared_transcript, const void *d_transcripts, const void *d_C, const void *d_G,
                                                const void *d_F, const void *d_B, const void *d_b, int b_shared, void *d_verdict, void *d_msm_out,
                                                void *d_transcripts_out, void *stream) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    ipp_ts ts;
    const int rca = ipp_ts_dev_args(c, shared_transcript, d_transcripts, d_transcripts_out, ts);
    if (rca) return rca;
    if (nbatch == 0) return BPGPU_OK;
    const bool from_gens = !d_G && !d_F && !d_B;
    if (!d_proofs || !d_verdict || !d_C || (n && !d_b) || (!from_gens && (!d_F || !d_B || (n && !d_G)))) return BPGPU_ERR_INVALID_ARG;
    if (((uintptr_t)d_proofs | (uintptr_t)d_C | (uintptr_t)d_G | (uintptr_t)d_F | (uintptr_t)d_B | (uintptr_t)d_b) & 3)
        return fail(c, BPGPU_ERR_INVALID_ARG, "device buffers must be 4-byte aligned");
    return dev_call(c, stream, [&](hipStream_t s) {
        return lin_verify_dev_locked(c, n, nbatch, d_proofs, proof_len, nullptr, 0, nullptr, d_C, d_G, d_F, d_B, d_b, b_shared, d_verdict, d_msm_out, d_transcripts_out,
                                   s, &ts);
    });
}

// ProofShare::audit_share for nshares shares of bitsize n (audit.h): front end (lane = share) -> the ragged (2n + 3, 5) pairs of
// multiscalar multiplications through bpgpu_msm_batch's engine -> Ok / Err per share.  Host pointers (the dealer's blame path).
extern "C" int bpgpu_rangeproof_audit_shares(bpgpu_ctx *c, size_t n, size_t nshares, const uint32_t *party_index, const uint8_t *shares,
                                             const uint8_t *bit_commitments, const uint8_t *poly_commitments, const uint8_t *challenges,
                                             int challenges_shared, uint8_t *verdict, uint8_t *checks_out) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    if (nshares == 0) return BPGPU_OK;
    if (!party_index || !shares || !bit_commitments || !poly_commitments || !challenges || !verdict) return BPGPU_ERR_INVALID_ARG;
    if (!(n == 8 || n == 16 || n == 32 || n == 64)) return fail(c, BPGPU_ERR_INVALID_ARG, "InvalidBitsize: n must be 8, 16, 32 or 64 (party.rs:41-43)");
    if ((uint64_t)nshares * (2 * n + 8) > 0x7fffffffull / 64) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large for this shape");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_gens) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    if (n > c->gens_capacity) {   // check_size (messages.rs:70-72): Err(()) for every share
        memset(verdict, BPGPU_VERDICT_VERIFICATION_ERROR, nshares);
        if (checks_out) memset(checks_out, 0, nshares * 64);
        return BPGPU_OK;
    }
    hipStream_t s = c->stream;
    const size_t share_len = 32 * (3 + 2 * n), nch = challenges_shared ? 1 : nshares;
    host_call<bpgpu_ctx> io(c, s);
    const int r_pi = io.in(nshares * 4 + 64), r_sh = io.in(nshares * share_len + 64), r_bc = io.in(nshares * 96 + 64), r_pc = io.in(nshares * 64 + 64),
              r_ch = io.in(nch * 96 + 64);
    const int r_v = io.out(nshares), r_o = io.out(nshares * 64);
    int rc = io.open();
    if (rc) return rc;
    char *d_pi = io.d(r_pi), *d_sh = io.d(r_sh), *d_bc = io.d(r_bc), *d_pc = io.d(r_pc), *d_ch = io.d(r_ch), *d_v = io.d(r_v), *d_o = io.d(r_o);
    io.put(r_pi, party_index, nshares * 4);
    io.put(r_sh, shares, nshares * share_len);
    io.put(r_bc, bit_commitments, nshares * 96);
    io.put(r_pc, poly_commitments, nshares * 64);
    io.put(r_ch, challenges, nch * 96);
    rc = io.upload();
    do {
        if (rc) break;
        const size_t per = 2 * n + 8;
        const size_t sz_terms = align_up(nshares * per * 32 + 64), sz_st = align_up(nshares * 4), sz_b = align_up(2 * nshares + 64);
        const size_t need = 2 * sz_terms + sz_st + sz_b;
        rc = ipp_reserve(c, need);
        if (rc) break;
        char *d_sc = c->ipp_buf, *d_pt = d_sc + sz_terms, *d_stat = d_pt + sz_terms, *d_mst = d_stat + sz_st;
        if (hipMemsetAsync(d_sc, 0, 2 * sz_terms + sz_st, s) != hipSuccess) { rc = fail(c, BPGPU_ERR_HIP, "memset failed"); break; }
        aud_shape sh;
        sh.n = (uint32_t)n;
        sh.lg_n = 0;
        while (((size_t)1 << sh.lg_n) < n) sh.lg_n++;
        sh.nshares = (uint32_t)nshares;
        sh.gens_capacity = (uint32_t)c->gens_capacity;
        sh.party_capacity = (uint32_t)c->party_capacity;
        sh.chal_shared = challenges_shared ? 1u : 0u;
        const uint32_t ns32 = (uint32_t)nshares;
        LAUNCH(c, s, "aud_prepare", k_aud_prepare, (ns32 + 63) / 64, 64, sh, (const uint32_t *)d_pi, (const uint8_t *)d_sh, (const uint8_t *)d_bc,
               (const uint8_t *)d_pc, (const uint8_t *)d_ch, (const uint32_t *)c->d_gens, (uint32_t *)d_sc, (uint32_t *)d_pt, (uint32_t *)d_stat);
        std::vector<uint32_t> nt(2 * nshares);
        for (size_t i = 0; i < nshares; i++) {
            nt[2 * i] = (uint32_t)(2 * n + 3);     // P_check (messages.rs:128-141)
            nt[2 * i + 1] = 5;                     // t_check (:149-160)
        }
        rc = msm_batch_dev_locked(c, 2 * nshares, nt.data(), d_sc, d_pt, d_o, d_mst, s);
        if (rc) break;
        LAUNCH(c, s, "aud_verdict", k_aud_verdict, (ns32 + 63) / 64, 64, ns32, (const uint32_t *)d_stat, (const uint8_t *)d_mst, (const uint32_t *)d_o,
               (uint8_t *)d_v);
        if (hipGetLastError() != hipSuccess) rc = fail(c, BPGPU_ERR_HIP, "launch failed");
    } while (0);
    rc = io.finish(io.download(rc));
    if (rc) return rc;
    memcpy(verdict, io.h(r_v), nshares);
    if (checks_out) memcpy(checks_out, io.h(r_o), nshares * 64);
    return BPGPU_OK;
}

// The rounds of InnerProductProof::create for nbatch proofs (ipp_prover.h): inputs and outputs in device memory.
// d_ts: the proofs' transcript states AFTER innerproduct_domain_sep(n), advanced in place.  The k (L, R) pairs and the
// final a, b go to d_proofs + p * proof_stride (+ 64 j, + 64 k); status_bytes (optional): BPGPU_MSM_* per proof.
// `fixed` (optional): G, H are the context's G(gn, gm), H(gn, gm) (n = gn gm) and Q = w B with w[p] given: every L_j / R_j
// is a pure generator-table MSM (msm_shared's walk) instead of a variable-base one -- no point decoding, no Horner chain.
struct ippc_fixed {
    size_t gn, gm;
    const uint32_t *w;       // [nbatch][8 words]
    uint32_t *gen_scalars;   // scratch, >= 2 nbatch (2n + 2) scalars
};
static int ippc_core(bpgpu_ctx *c, hipStream_t s, size_t n, size_t k, size_t nbatch, const void *d_a, const void *d_b, const void *d_gf, const void *d_hf,
                     const void *d_q, const void *d_G, const void *d_H, int bases_shared, uint32_t *d_ts, uint8_t *d_proofs, size_t proof_stride,
                     uint8_t *d_status_bytes, const ippc_fixed *fixed = nullptr) {
    const size_t N = n + 1, w_v = align_up(nbatch * n * 32), w_u = align_up(nbatch * 32), w_terms = align_up(2 * nbatch * N * 32 + 64),
                 w_out = align_up(2 * nbatch * 32), w_st = align_up(2 * nbatch + 64), w_status = align_up(nbatch * 4);
    const size_t need = 4 * w_v + 2 * w_u + 2 * w_terms + w_out + w_st + w_status;
    {
        const int rcr = ipp_reserve(c, need);
        if (rcr) return rcr;
    }
    char *wb = c->ipp_buf;
    uint32_t *w_a = (uint32_t *)wb, *w_b = (uint32_t *)(wb + w_v), *w_G = (uint32_t *)(wb + 2 * w_v), *w_H = (uint32_t *)(wb + 3 * w_v);
    uint32_t *w_uu = (uint32_t *)(wb + 4 * w_v), *w_ui = (uint32_t *)(wb + 4 * w_v + w_u);
    uint32_t *m_sc = (uint32_t *)(wb + 4 * w_v + 2 * w_u), *m_pt = (uint32_t *)((char *)m_sc + w_terms), *m_out = (uint32_t *)((char *)m_pt + w_terms);
    uint8_t *m_st = (uint8_t *)m_out + w_out;
    uint32_t *d_status = (uint32_t *)(m_st + w_st);
    HIPCHK(c, hipMemsetAsync(d_status, 0, nbatch * 4, s));
    ippc_shape sh;
    sh.n = (uint32_t)n;
    sh.k = (uint32_t)k;
    sh.nproofs = (uint32_t)nbatch;
    sh.bases_shared = bases_shared ? 1u : 0u;
    const uint32_t nb32 = (uint32_t)nbatch, nt32 = (uint32_t)(nbatch * n);
    LAUNCH(c, s, "ippc_init", k_ippc_init, (nt32 + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, nt32, sh, (const uint8_t *)d_a, (const uint8_t *)d_b, (const uint8_t *)d_gf,
           (const uint8_t *)d_hf, w_a, w_b, w_G, w_H, d_status);
    std::vector<uint32_t> nterms(2 * nbatch, (uint32_t)N);
    const uint32_t n_q = (nb32 + BP_BLOCK - 1) / BP_BLOCK;
    for (uint32_t j = 0; j < k; j++) {
        int rc;
        if (fixed) {
            LAUNCH(c, s, "ippc_terms", k_ippc_terms_fixed, n_q + (nt32 + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, n_q, nt32, sh, j, (const uint32_t *)w_a,
                   (const uint32_t *)w_b, (const uint32_t *)w_G, (const uint32_t *)w_H, fixed->w, fixed->gen_scalars);
            rc = msm_shared_dev_locked(c, fixed->gn, fixed->gm, 2 * nbatch, 0, fixed->gen_scalars, nullptr, nullptr, m_out, m_st, nullptr, s);
        } else {
            LAUNCH(c, s, "ippc_terms", k_ippc_terms, n_q + (nt32 + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, n_q, nt32, sh, j, (const uint32_t *)w_a, (const uint32_t *)w_b,
                   (const uint32_t *)w_G, (const uint32_t *)w_H, (const uint8_t *)d_G, (const uint8_t *)d_H, (const uint8_t *)d_q, m_sc, m_pt);
            rc = msm_batch_dev_locked(c, 2 * nbatch, nterms.data(), m_sc, m_pt, m_out, m_st, s);   // all L_j and R_j of the batch (ipp.rs:87-113)
        }
        if (rc) return rc;   // (callers drain the stream before they reuse their staging buffers)
        LAUNCH(c, s, "ippc_challenge", k_ippc_challenge, (nb32 + RP_BLOCK - 1) / RP_BLOCK, RP_BLOCK, sh, j, (const uint32_t *)m_out, (const uint8_t *)m_st,
               d_ts, w_uu, w_ui, d_proofs, (uint32_t)proof_stride, d_status);
        LAUNCH(c, s, "ippc_fold", k_ippc_fold, (nt32 + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, nt32, sh, j, (const uint32_t *)w_uu, (const uint32_t *)w_ui, w_a, w_b, w_G,
               w_H);
    }
    LAUNCH(c, s, "ippc_final", k_ippc_final, (nb32 + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, sh, (const uint32_t *)w_a, (const uint32_t *)w_b, d_proofs,
           (uint32_t)proof_stride, (const uint32_t *)d_status, d_status_bytes);
    HIPCHK(c, hipGetLastError());
    return BPGPU_OK;
}

// ============================================================================
// batched inner-product-proof creation (ipp_prover.h)
// ============================================================================
// ---- the common exit of the prover entry points -------------------------------------------------------------------
// The provers stage SECRETS (values, blindings, the witness vectors, every random scalar) in the context's persistent buffers:
// the pinned staging block, the device IO buffer, their working sets and -- as window digits of secret scalars -- the arena.
// The reference zeroizes its party state on Drop (party.rs:148-260, 308+); here every entered call, successful or not, leaves
// through host_call::finish with secrets() declared: the device buffers are cleared on the stream behind the call's last copy, the
// call's end is recorded (ctx_leave), the stream is drained (host_wait), then the secret part of the staging block is cleared.
// What is NOT cleared: registers / LDS of finished kernels and the caller's own buffers.
// HIPRC: a HIP call as a return code, for exits that must go through finish.
static int hip_rc(bpgpu_ctx *c, hipError_t e, const char *call) {
    return e == hipSuccess ? BPGPU_OK : fail(c, BPGPU_ERR_HIP, "%s failed: %s", call, hipGetErrorString(e));
}
#define HIPRC(c, call) hip_rc(c, (call), #call)

// ts_host (with ts_stride 0 or BPGPU_TRANSCRIPT_BYTES): the callers' own transcripts, checked by the caller, in place of label / shared_transcript:
// k_ipp_ts_fill turns them into the rounds' working states, which ts_out_host (optional) gets back as create() leaves them
static int ipp_create_host_call(bpgpu_ctx *c, size_t n, size_t nbatch, const uint8_t *label, size_t label_len, const uint8_t *shared_transcript,
                                const uint8_t *ts_host, size_t ts_stride, const uint8_t *Q, const uint8_t *G_factors, const uint8_t *H_factors,
                                const uint8_t *G, const uint8_t *H, int bases_shared, const uint8_t *a, const uint8_t *b, uint8_t *proofs_out,
                                uint8_t *status_out, uint8_t *ts_out_host) {
    if (nbatch == 0) return BPGPU_OK;
    if (!Q || !G_factors || !H_factors || !G || !H || !a || !b || !proofs_out || !status_out) return BPGPU_ERR_INVALID_ARG;
    if (n == 0 || (n & (n - 1))) return fail(c, BPGPU_ERR_INVALID_ARG, "n must be a power of two (ipp.rs:54-59)");
    size_t k = 0;
    while (((size_t)1 << k) < n) k++;
    if (k > BP_RP_MAX_K) return fail(c, BPGPU_ERR_INVALID_ARG, "n > 2^%d not supported", BP_RP_MAX_K);
    if ((uint64_t)nbatch * 2 * (n + 1) > 0x7fffffffull / 64) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large for this shape");
    if (shared_transcript && !ts_state_ok(shared_transcript)) return fail(c, BPGPU_ERR_INVALID_ARG, "malformed transcript state");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t proof_len = 32 * (2 * k + 2), TS = BPGPU_TRANSCRIPT_BYTES;
    // ---- inputs: one pinned staging block -> the persistent device IO buffer
    host_call<bpgpu_ctx> io(c, s);
    const size_t b_v = nbatch * n * 32 + 64, b_base = (bases_shared ? 1 : nbatch) * n * 32 + 64;
    const int r_a = io.in(b_v), r_b = io.in(b_v), r_gf = io.in(b_v), r_hf = io.in(b_v), r_q = io.in(nbatch * 32 + 64), r_G = io.in(b_base), r_H = io.in(b_base),
              r_ts = io.in((!ts_host ? nbatch : ts_stride ? nbatch : 1) * TS);
    const int r_proofs = io.out(nbatch * proof_len), r_stb = io.out(nbatch), r_to = io.out(ts_host ? nbatch * TS : 0);
    io.secrets(io.off[r_gf]);   // the witness a, b
    int rc = io.open();
    if (rc) return io.finish(rc);
    io.put(r_a, a, nbatch * n * 32);
    io.put(r_b, b, nbatch * n * 32);
    io.put(r_gf, G_factors, nbatch * n * 32);
    io.put(r_hf, H_factors, nbatch * n * 32);
    io.put(r_q, Q, nbatch * 32);
    io.put(r_G, G, (bases_shared ? 1 : nbatch) * n * 32);
    io.put(r_H, H, (bases_shared ? 1 : nbatch) * n * 32);
    if (ts_host) {
        io.put(r_ts, ts_host, (ts_stride ? nbatch : 1) * TS);
    } else {   // every proof's transcript after innerproduct_domain_sep(n) (transcript.rs:50-53)
        uint8_t st0[BPGPU_TRANSCRIPT_BYTES];
        ipp_domain_sep_state(st0, label, label_len, shared_transcript, n, nullptr);
        for (size_t p = 0; p < nbatch; p++) memcpy(io.h(r_ts) + p * TS, st0, TS);
    }
    uint32_t *d_ts = (uint32_t *)io.d(ts_host ? r_to : r_ts);   // the rounds' working states
    rc = io.upload();
    if (!rc) rc = HIPRC(c, hipMemsetAsync(io.d(r_proofs), 0, nbatch * proof_len, s));
    if (!rc && ts_host) {   // the separator per proof on the device
        const uint32_t nb32 = (uint32_t)nbatch;
        LAUNCH(c, s, "ipp_ts_fill", k_ipp_ts_fill, (nb32 + RP_BLOCK - 1) / RP_BLOCK, RP_BLOCK, nb32, (uint32_t)n, (const uint32_t *)io.d(r_ts),
               (uint32_t)(ts_stride ? BP_TS_WORDS : 0), d_ts);
        rc = HIPRC(c, hipGetLastError());
    }
    // ---- rounds (ippc_core: own working set, the batched MSMs claim the arena)
    if (!rc)
        rc = ippc_core(c, s, n, k, nbatch, io.d(r_a), io.d(r_b), io.d(r_gf), io.d(r_hf), io.d(r_q), io.d(r_G), io.d(r_H), bases_shared, d_ts,
                       (uint8_t *)io.d(r_proofs), proof_len, (uint8_t *)io.d(r_stb));
    rc = io.finish(io.download(rc));
    if (rc) return rc;
    memcpy(proofs_out, io.h(r_proofs), nbatch * proof_len);
    memcpy(status_out, io.h(r_stb), nbatch);
    if (ts_out_host) memcpy(ts_out_host, io.h(r_to), nbatch * TS);
    return BPGPU_OK;
}

extern "C" int bpgpu_ipp_create_batch(bpgpu_ctx *c, size_t n, size_t nbatch, const uint8_t *label, size_t label_len, const uint8_t *shared_transcript,
                                      const uint8_t *Q, const uint8_t *G_factors, const uint8_t *H_factors, const uint8_t *G, const uint8_t *H,
                                      int bases_shared, const uint8_t *a, const uint8_t *b, uint8_t *proofs_out, uint8_t *status_out) {
    if (!c || (label_len && !label)) return BPGPU_ERR_INVALID_ARG;
    return ipp_create_host_call(c, n, nbatch, label, label_len, shared_transcript, nullptr, 0, Q, G_factors, H_factors, G, H, bases_shared, a, b, proofs_out,
                                status_out, nullptr);
}

extern "C" int bpgpu_ipp_create_batch_ts(bpgpu_ctx *c, size_t n, size_t nbatch, const uint8_t *transcripts, size_t transcript_stride, const uint8_t *Q,
                                         const uint8_t *G_factors, const uint8_t *H_factors, const uint8_t *G, const uint8_t *H, int bases_shared,
                                         const uint8_t *a, const uint8_t *b, uint8_t *proofs_out, uint8_t *status_out, uint8_t *transcripts_out) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    const int rca = ipp_ts_host_args(c, transcripts, transcript_stride, nbatch);
    if (rca) return rca;
    return ipp_create_host_call(c, n, nbatch, nullptr, 0, nullptr, transcripts, transcript_stride, Q, G_factors, H_factors, G, H, bases_shared, a, b, proofs_out,
                                status_out, transcripts_out);
}

// ============================================================================
// batched linear-proof creation (linear_prover.h)
// ============================================================================
// ts_host == NULL: `rng` holds 64 (2 lg n + 2) bytes per proof (NULL: the OS generator's) and every proof starts from the label's / the shared
// state.  ts_host (with ts_stride 0 or BPGPU_TRANSCRIPT_BYTES): the callers' own transcripts, checked by the caller, and `rng` holds ONE 32-byte
// seed per proof (NULL: the OS generator's), from which linc_public_lane draws on the device -- no buffer of draws anywhere on the host.
static int lin_create_host_call(bpgpu_ctx *c, size_t n, size_t nbatch, const uint8_t *label, size_t label_len, const uint8_t *shared_transcript,
                                const uint8_t *ts_host, size_t ts_stride, const uint8_t *rng, const uint8_t *C, const uint8_t *r, const uint8_t *a,
                                const uint8_t *b, int b_shared, const uint8_t *G, const uint8_t *F, const uint8_t *B, uint8_t *proofs_out,
                                uint8_t *status_out, uint8_t *transcripts_out) {
    if (nbatch == 0) return BPGPU_OK;
    const bool from_gens = !G && !F && !B;   // bases = the context's generators: every MSM through the window tables
    if (!C || !r || !a || !b || (!from_gens && (!G || !F || !B)) || !proofs_out || !status_out) return BPGPU_ERR_INVALID_ARG;
    if (n == 0 || (n & (n - 1))) return fail(c, BPGPU_ERR_INVALID_ARG, "InvalidInputLength: n must be a power of two (linear_proof.rs:68-70)");
    size_t k = 0;
    while (((size_t)1 << k) < n) k++;
    if (k > BP_RP_MAX_K) return fail(c, BPGPU_ERR_INVALID_ARG, "n > 2^%d not supported", BP_RP_MAX_K);
    if ((uint64_t)nbatch * (n + 4) > 0x7fffffffull / 64) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large for this shape");
    if (shared_transcript && !ts_state_ok(shared_transcript)) return fail(c, BPGPU_ERR_INVALID_ARG, "malformed transcript state");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (from_gens) {
        if (!c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
        if (n > c->gens_capacity) return fail(c, BPGPU_ERR_NO_GENS, "InvalidGeneratorsLength: generators too small for n=%zu", n);
    }
    const size_t proof_len = 32 * (2 * k + 3), TS = BPGPU_TRANSCRIPT_BYTES, nd = 2 * k + 2, nb_b = b_shared ? 1 : nbatch;
    // ---- inputs: one pinned staging block -> the persistent device IO buffer
    host_call<bpgpu_ctx> io(c, s);
    const int r_a = io.in(nbatch * n * 32 + 64), r_b = io.in(nb_b * n * 32 + 64), r_C = io.in(nbatch * 32 + 64), r_r = io.in(nbatch * 32 + 64), r_G = io.in(n * 32 + 64),
              r_fb = io.in(64 + 64), r_rng = io.in(ts_host ? nbatch * 32 : nbatch * nd * 64), r_ts = io.in((!ts_host ? nbatch : ts_stride ? nbatch : 1) * TS);
    const int r_proofs = io.out(nbatch * proof_len), r_stb = io.out(nbatch), r_to = io.out(ts_host ? nbatch * TS : 0);
    // a, r, the random draws or the seeds (and the public inputs between them); without ts_host the transcript block behind is reused for the way back
    io.secrets(io.off[r_ts]);
    int rc = io.open();
    if (rc) return io.finish(rc);
    char *d_a = io.d(r_a), *d_b = io.d(r_b), *d_C = io.d(r_C), *d_r = io.d(r_r), *d_G = io.d(r_G), *d_fb = io.d(r_fb), *d_rng = io.d(r_rng), *d_ts = io.d(r_ts),
         *d_proofs = io.d(r_proofs), *d_stb = io.d(r_stb);
    if (ts_host) d_ts = io.d(r_to);   // the working states: filled by k_linc_public_ts from the callers' at r_ts
    io.put(r_a, a, nbatch * n * 32);
    io.put(r_b, b, nb_b * n * 32);
    io.put(r_C, C, nbatch * 32);
    io.put(r_r, r, nbatch * 32);
    if (!from_gens) {
        io.put(r_G, G, n * 32);
        memcpy(io.h(r_fb), F, 32);
        memcpy(io.h(r_fb) + 32, B, 32);
    }
    const uint8_t *e_G = from_gens ? (const uint8_t *)(c->d_gens + 16) : (const uint8_t *)d_G;          // encodings the transcript absorbs
    const uint8_t *e_F = from_gens ? (const uint8_t *)(c->d_gens + 8) : (const uint8_t *)d_fb;
    const uint8_t *e_B = from_gens ? (const uint8_t *)c->d_gens : (const uint8_t *)d_fb + 32;
    if (ts_host) {
        if (rng) io.put(r_rng, rng, nbatch * 32);
        else if ((rc = os_random(c, io.h(r_rng), nbatch * 32)) != 0) return io.finish(rc);
        io.put(r_ts, ts_host, (ts_stride ? nbatch : 1) * TS);
    } else {
        if (rng) io.put(r_rng, rng, nbatch * nd * 64);
        else if ((rc = os_random(c, io.h(r_rng), nbatch * nd * 64)) != 0) return io.finish(rc);   // Scalar::random(&mut thread_rng())
        // every proof's transcript after innerproduct_domain_sep(n) (linear_proof.rs:73)
        uint8_t st0[BPGPU_TRANSCRIPT_BYTES];
        ipp_domain_sep_state(st0, label, label_len, shared_transcript, n, nullptr);
        for (size_t p = 0; p < nbatch; p++) memcpy(io.h(r_ts) + p * TS, st0, TS);
    }
    rc = io.upload();
    if (!rc) rc = HIPRC(c, hipMemsetAsync(d_proofs, 0, nbatch * proof_len, s));
    do {
        if (rc) break;
        // ---- working set (own allocation: the batched MSMs claim the arena)
        const size_t N = n / 2 + 2, NS = n + 2;
        const size_t w_v = align_up(nbatch * n * 32), w_u = align_up(nbatch * 32), w_d = align_up(nbatch * nd * 32),
                     w_terms = align_up(std::max(2 * nbatch * (from_gens ? NS : N), nbatch * NS) * 32 + 64), w_out = align_up(2 * nbatch * 32), w_st = align_up(2 * nbatch + 64),
                     w_status = align_up(nbatch * 4);
        const size_t need = 3 * w_v + 3 * w_u + w_d + 2 * w_terms + w_out + w_st + w_status;
        rc = ipp_reserve(c, need);
        if (rc) break;
        char *wb = c->ipp_buf;
        uint32_t *w_a = (uint32_t *)wb, *w_b = (uint32_t *)(wb + w_v), *w_G = (uint32_t *)(wb + 2 * w_v);
        uint32_t *w_r = (uint32_t *)(wb + 3 * w_v), *w_x = (uint32_t *)((char *)w_r + w_u), *w_xi = (uint32_t *)((char *)w_x + w_u);
        uint32_t *w_dr = (uint32_t *)((char *)w_xi + w_u);
        uint32_t *m_sc = (uint32_t *)((char *)w_dr + w_d), *m_pt = (uint32_t *)((char *)m_sc + w_terms), *m_out = (uint32_t *)((char *)m_pt + w_terms);
        uint8_t *m_st = (uint8_t *)m_out + w_out;
        uint32_t *d_status = (uint32_t *)(m_st + w_st);
        if (hipMemsetAsync(d_status, 0, nbatch * 4, s) != hipSuccess) { rc = fail(c, BPGPU_ERR_HIP, "memset failed"); break; }
        linc_shape sh;
        sh.n = (uint32_t)n;
        sh.k = (uint32_t)k;
        sh.nproofs = (uint32_t)nbatch;
        sh.b_shared = b_shared ? 1u : 0u;
        const uint32_t nb32 = (uint32_t)nbatch, nt32 = (uint32_t)(nbatch * n), n_q = (nb32 + BP_BLOCK - 1) / BP_BLOCK;
        LAUNCH(c, s, "linc_init", k_linc_init, (nt32 + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, nt32, sh, (const uint8_t *)d_a, (const uint8_t *)d_b, w_a, w_b, w_G,
               d_status);
        if (ts_host)
            LAUNCH(c, s, "linc_public_ts", k_linc_public_ts, (nb32 + RP_BLOCK - 1) / RP_BLOCK, RP_BLOCK, sh, (const uint8_t *)d_C, (const uint8_t *)d_b, e_G, e_F, e_B,
                   (const uint8_t *)d_r, (const uint8_t *)d_rng, (const uint32_t *)io.d(r_ts), (uint32_t)(ts_stride ? BP_TS_WORDS : 0), (uint32_t *)d_ts, w_r, w_dr,
                   d_status);
        else
            LAUNCH(c, s, "linc_public", k_linc_public, (nb32 + RP_BLOCK - 1) / RP_BLOCK, RP_BLOCK, sh, (const uint8_t *)d_C, (const uint8_t *)d_b, e_G, e_F, e_B,
                   (const uint8_t *)d_r, (const uint8_t *)d_rng, (uint32_t *)d_ts, w_r, w_dr, d_status);
        std::vector<uint32_t> nterms(2 * nbatch, (uint32_t)N);
        for (uint32_t j = 0; j < k && !rc; j++) {
            if (from_gens) {   // rows of generator-table scalars (B_blinding, B, G_0..): m_sc holds [2 nbatch][n + 2] scalars
                LAUNCH(c, s, "linc_terms", k_linc_terms_fixed, n_q + (nt32 + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, n_q, nt32, sh, j, (const uint32_t *)w_a,
                       (const uint32_t *)w_b, (const uint32_t *)w_G, (const uint32_t *)w_dr, m_sc);
                rc = msm_shared_dev_locked(c, n, 1, 2 * nbatch, 0, m_sc, nullptr, nullptr, m_out, m_st, nullptr, s, true);
            } else {
                LAUNCH(c, s, "linc_terms", k_linc_terms, n_q + (nt32 + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, n_q, nt32, sh, j, (const uint32_t *)w_a, (const uint32_t *)w_b,
                       (const uint32_t *)w_G, (const uint32_t *)w_dr, e_G, e_F, e_B, m_sc, m_pt);
                rc = msm_batch_dev_locked(c, 2 * nbatch, nterms.data(), m_sc, m_pt, m_out, m_st, s);   // all L_j and R_j of the batch (:104-117)
            }
            if (rc) break;
            LAUNCH(c, s, "linc_challenge", k_linc_challenge, (nb32 + RP_BLOCK - 1) / RP_BLOCK, RP_BLOCK, sh, j, (const uint32_t *)m_out, (const uint8_t *)m_st,
                   (uint32_t *)d_ts, (const uint32_t *)w_dr, w_r, w_x, w_xi, (uint8_t *)d_proofs, (uint32_t)proof_len, d_status);
            LAUNCH(c, s, "linc_fold", k_linc_fold, (nt32 + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, nt32, sh, j, (const uint32_t *)w_x, (const uint32_t *)w_xi, w_a, w_b, w_G);
        }
        if (rc) break;
        if (from_gens) {
            LAUNCH(c, s, "linc_sterms", k_linc_sterms_fixed, n_q + (nt32 + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, n_q, nt32, sh, (const uint32_t *)w_b,
                   (const uint32_t *)w_G, (const uint32_t *)w_dr, m_sc);
            rc = msm_shared_dev_locked(c, n, 1, nbatch, 0, m_sc, nullptr, nullptr, m_out, m_st, nullptr, s, true);
        } else {
            LAUNCH(c, s, "linc_sterms", k_linc_sterms, n_q + (nt32 + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, n_q, nt32, sh, (const uint32_t *)w_b, (const uint32_t *)w_G,
                   (const uint32_t *)w_dr, e_G, e_F, e_B, m_sc, m_pt);
            std::vector<uint32_t> nts(nbatch, (uint32_t)NS);
            rc = msm_batch_dev_locked(c, nbatch, nts.data(), m_sc, m_pt, m_out, m_st, s);               // every S (:155-157)
        }
        if (rc) break;
        LAUNCH(c, s, "linc_final", k_linc_final, (nb32 + RP_BLOCK - 1) / RP_BLOCK, RP_BLOCK, sh, (const uint32_t *)m_out, (const uint8_t *)m_st, (uint32_t *)d_ts,
               (const uint32_t *)w_a, (const uint32_t *)w_dr, (const uint32_t *)w_r, (uint8_t *)d_proofs, (uint32_t)proof_len, d_status, (uint8_t *)d_stb);
        if (hipGetLastError() != hipSuccess) rc = fail(c, BPGPU_ERR_HIP, "launch failed");
    } while (0);
    rc = io.download(rc);
    // without ts_host the transcript block of the staging buffer is free again: reuse it for the way back (with it the states are an output region)
    char *h_ts = io.h(ts_host ? r_to : r_ts);
    if (!rc && transcripts_out && !ts_host && hipMemcpyAsync(h_ts, d_ts, nbatch * TS, hipMemcpyDeviceToHost, s) != hipSuccess)
        rc = fail(c, BPGPU_ERR_HIP, "D2H copy failed");
    rc = io.finish(rc);   // (on an error too: the stream is drained before the staging buffers are reused, the secrets cleared)
    if (rc) return rc;
    memcpy(proofs_out, io.h(r_proofs), nbatch * proof_len);
    memcpy(status_out, io.h(r_stb), nbatch);
    if (transcripts_out) memcpy(transcripts_out, h_ts, nbatch * TS);
    return BPGPU_OK;
}

extern "C" int bpgpu_linear_create_batch(bpgpu_ctx *c, size_t n, size_t nbatch, const uint8_t *label, size_t label_len, const uint8_t *shared_transcript,
                                         const uint8_t *rng, const uint8_t *C, const uint8_t *r, const uint8_t *a, const uint8_t *b, int b_shared,
                                         const uint8_t *G, const uint8_t *F, const uint8_t *B, uint8_t *proofs_out, uint8_t *status_out,
                                         uint8_t *transcripts_out) {
    if (!c || (label_len && !label)) return BPGPU_ERR_INVALID_ARG;
    return lin_create_host_call(c, n, nbatch, label, label_len, shared_transcript, nullptr, 0, rng, C, r, a, b, b_shared, G, F, B, proofs_out, status_out,
                                transcripts_out);
}

extern "C" int bpgpu_linear_create_batch_ts(bpgpu_ctx *c, size_t n, size_t nbatch, const uint8_t *transcripts, size_t transcript_stride,
                                            const uint8_t *rng32, const uint8_t *C, const uint8_t *r, const uint8_t *a, const uint8_t *b, int b_shared,
                                            const uint8_t *G, const uint8_t *F, const uint8_t *B, uint8_t *proofs_out, uint8_t *status_out,
                                            uint8_t *transcripts_out) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    const int rca = ipp_ts_host_args(c, transcripts, transcript_stride, nbatch);
    if (rca) return rca;
    return lin_create_host_call(c, n, nbatch, nullptr, 0, nullptr, transcripts, transcript_stride, rng32, C, r, a, b, b_shared, G, F, B, proofs_out, status_out,
                                transcripts_out);
}

// ============================================================================
// batched range-proof creation (rp_prover.h)
// ============================================================================
// working set of the range-proof / R1CS provers and the party / dealer calls (cleared by host_call::finish on the way out, so an
// outgrown block is clean when it is freed)
static int rpp_reserve(bpgpu_ctx *c, size_t need) {
    if (c->rpp_cap >= need) return BPGPU_OK;
    HIPCHK(c, hipDeviceSynchronize());
    if (c->rpp_buf) HIPCHK(c, hipFree(c->rpp_buf));
    c->rpp_buf = nullptr;
    c->rpp_cap = 0;
    HIPCHK(c, hipMalloc((void **)&c->rpp_buf, need + need / 8));
    c->rpp_cap = need + need / 8;
    return BPGPU_OK;
}
// the parameter checks of prove_multiple_with_rng / Party::new / Dealer::new (mod.rs:244-246, party.rs:41-53, dealer.rs:34-60) ...
static int rpp_check_nm(bpgpu_ctx *c, size_t n, size_t m) {
    if (!(n == 8 || n == 16 || n == 32 || n == 64)) return fail(c, BPGPU_ERR_INVALID_ARG, "InvalidBitsize: n must be 8, 16, 32 or 64");
    if (m == 0 || (m & (m - 1))) return fail(c, BPGPU_ERR_INVALID_ARG, "InvalidAggregation: m must be a power of two");
    return BPGPU_OK;
}
// ... and, with the context locked, those against the loaded generators, the values (host memory; nullptr: not checkable) and the sizes
static int rpp_shape_locked(bpgpu_ctx *c, size_t n, size_t m, size_t nbatch, const uint64_t *values, rpp_shape &sh) {
    if (!c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    if (c->gens_capacity < n || c->party_capacity < m) return fail(c, BPGPU_ERR_NO_GENS, "InvalidGeneratorsLength: generators too small for n=%zu m=%zu", n, m);
    if (n < 64 && values)
        for (size_t i = 0; i < nbatch * m; i++)
            if (values[i] >> n) return fail(c, BPGPU_ERR_INVALID_ARG, "value %zu does not fit %zu bits", i, n);   // (the reference would prove a false statement's bits silently; refuse)
    const size_t nm = n * m;
    size_t k = 0;
    while (((size_t)1 << k) < nm) k++;
    if (k > BP_RP_MAX_K) return fail(c, BPGPU_ERR_INVALID_ARG, "n*m > 2^%d not supported", BP_RP_MAX_K);
    sh.n = (uint32_t)n;
    sh.m = (uint32_t)m;
    sh.nm = (uint32_t)nm;
    sh.k = (uint32_t)k;
    sh.nproofs = (uint32_t)nbatch;
    sh.proof_len = (uint32_t)(32 * (9 + 2 * k));
    sh.n_gen_terms = (uint32_t)(2 * nm + 2);
    sh.rng_per_proof = (uint32_t)(64 * (m * (2 * n + 2) + 2 * m));
    const size_t nmsm1 = nbatch * (2 + m);
    const uint64_t gs_bytes = (uint64_t)nmsm1 * sh.n_gen_terms * 32;
    if (gs_bytes > (4ull << 30) || (uint64_t)nmsm1 * sh.n_gen_terms > 0x7fffffffull || (uint64_t)nbatch * nm > 0x7fffffffull / 64)
        return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large for this shape");
    return BPGPU_OK;
}
// where the chain's draws and start transcripts come from (rpp_chain)
struct rpp_source {
    const uint8_t *rng = nullptr;       // 64 bytes per draw, or
    const uint8_t *seeds = nullptr;     // 32 bytes per proof
    const uint32_t *ts_in = nullptr;    // the callers' states before rangeproof_domain_sep (nullptr: d_ts holds separated states)
    uint32_t ts_in_stride = 0;          // words between them: 0 (one for all) or BP_TS_WORDS
    bool rw = false;                    // the rewindable form (m = 1): draw 0 of the seed minus (value + 2^64 message)
    const uint32_t *messages = nullptr; // 16 bytes per proof, or nullptr (every message 0)
};
static int rpp_chain(bpgpu_ctx *c, hipStream_t s, const rpp_shape &sh, const uint64_t *d_values, const uint8_t *d_bl, rpp_source src, uint32_t *d_ts,
                     uint8_t *d_proofs, uint8_t *d_coms, const char *stage_seeds);

extern "C" int bpgpu_rangeproof_prove_batch(bpgpu_ctx *c, size_t n, size_t m, size_t nbatch, const uint64_t *values, const uint8_t *blindings,
                                            const uint8_t *label, size_t label_len, const uint8_t *shared_transcript, const uint8_t *rng,
                                            uint8_t *proofs_out, uint8_t *commitments_out, uint8_t *transcripts_out) {
    if (!c || (label_len && !label)) return BPGPU_ERR_INVALID_ARG;
    if (nbatch == 0) return BPGPU_OK;
    if (!values || !blindings || !proofs_out || !commitments_out) return BPGPU_ERR_INVALID_ARG;
    int rc = rpp_check_nm(c, n, m);
    if (rc) return rc;
    if (shared_transcript && !ts_state_ok(shared_transcript)) return fail(c, BPGPU_ERR_INVALID_ARG, "malformed transcript state");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    rpp_shape sh;
    if ((rc = rpp_shape_locked(c, n, m, nbatch, values, sh))) return rc;
    const size_t TS = BPGPU_TRANSCRIPT_BYTES, proof_len = sh.proof_len;
    hipStream_t s = c->stream;
    // ---- inputs through pinned staging into the persistent IO buffer
    host_call<bpgpu_ctx> io(c, s);
    const int r_val = io.in(nbatch * m * 8), r_bl = io.in(nbatch * m * 32), r_rng = io.in(nbatch * sh.rng_per_proof), r_ts = io.in(nbatch * TS);
    const int r_pr = io.out(nbatch * proof_len), r_cm = io.out(nbatch * m * 32), r_to = io.out(nbatch * TS);
    io.secrets(io.off[r_ts]);   // values, blindings, every random scalar
    rc = io.open();
    if (rc) return io.finish(rc);
    io.put(r_val, values, nbatch * m * 8);
    io.put(r_bl, blindings, nbatch * m * 32);
    if (rng) io.put(r_rng, rng, nbatch * sh.rng_per_proof);
    else {   // thread_rng() of prove_multiple (mod.rs:291-310): OS CSPRNG
        rc = os_random(c, io.h(r_rng), nbatch * sh.rng_per_proof);
        if (rc) return io.finish(rc);
    }
    uint8_t st_start[BPGPU_TRANSCRIPT_BYTES];
    {   // every proof's transcript after rangeproof_domain_sep(n, m) (transcript.rs:44-48)
        if (shared_transcript) memcpy(st_start, shared_transcript, TS);
        else bpgpu_transcript_new(label, label_len, st_start);
        uint32_t w[50];
        strobe t;
        ts_to_strobe(t, w, st_start);
        const uint8_t rp[13] = {'r', 'a', 'n', 'g', 'e', 'p', 'r', 'o', 'o', 'f', ' ', 'v', '1'}, ln[1] = {'n'}, lm[1] = {'m'};
        merlin_append_message(t, DOM_SEP, 7, rp, 13);
        merlin_append_u64(t, ln, 1, n);
        merlin_append_u64(t, lm, 1, m);
        uint8_t st1[BPGPU_TRANSCRIPT_BYTES];
        ts_from_strobe(st1, t);
        for (size_t p = 0; p < nbatch; p++) memcpy(io.h(r_ts) + p * TS, st1, TS);
    }
    const uint64_t *d_values = (const uint64_t *)io.d(r_val);
    const uint8_t *d_bl = (const uint8_t *)io.d(r_bl), *d_rng = (const uint8_t *)io.d(r_rng);
    uint32_t *d_ts = (uint32_t *)io.d(r_ts);
    uint8_t *d_proofs = (uint8_t *)io.d(r_pr), *d_coms = (uint8_t *)io.d(r_cm);
    if ((rc = io.upload())) return io.finish(rc);
    rpp_source src;
    src.rng = d_rng;
    rc = rpp_chain(c, s, sh, d_values, d_bl, src, d_ts, d_proofs, d_coms, nullptr);
    if (!rc && (hipMemcpyAsync(io.d(r_to), d_ts, nbatch * TS, hipMemcpyDeviceToDevice, s) != hipSuccess || io.download(0)))
        rc = fail(c, BPGPU_ERR_HIP, "D2H copy failed");
    rc = io.finish(rc);
    if (rc) return rc;
    memcpy(proofs_out, io.h(r_pr), nbatch * proof_len);
    memcpy(commitments_out, io.h(r_cm), nbatch * m * 32);
    if (transcripts_out) memcpy(transcripts_out, io.h(r_to), nbatch * TS);
    return BPGPU_OK;
}

// The prover's launch chain over device-resident inputs, enqueued on s.  The draws come from src.rng (64 bytes each, transcripts in
// d_ts already separated) or from src.seeds (32 bytes per proof, every draw computed by the lane that consumes it; the transcripts
// start at src.ts_in, before rangeproof_domain_sep).  d_ts: the working states, left as the prover leaves them (nullptr: kept in the
// working set).  stage_seeds: seeds in pinned host memory, which the chain copies into its working set and reads from there.
static int rpp_chain(bpgpu_ctx *c, hipStream_t s, const rpp_shape &sh, const uint64_t *d_values, const uint8_t *d_bl, rpp_source src, uint32_t *d_ts,
                     uint8_t *d_proofs, uint8_t *d_coms, const char *stage_seeds) {
    const size_t n = sh.n, m = sh.m, nm = sh.nm, k = sh.k, nbatch = sh.nproofs, proof_len = sh.proof_len, nmsm1 = nbatch * (2 + m);
    const uint64_t gs_bytes = (uint64_t)nmsm1 * sh.n_gen_terms * 32;
    const bool seeded = src.seeds || stage_seeds;
    int rc;
    // ---- working set
    const size_t w_gs = align_up(gs_bytes), w_mo = align_up(nmsm1 * 32), w_ms = align_up(nmsm1 + 64), w_f = align_up(RPP_FIXED * nbatch * 32),
                 w_p = align_up(RPP_PARTY_FIELDS * nbatch * m * 32), w_v = align_up(nbatch * nm * 32), w_q = align_up(nbatch * 32), w_gen = align_up(nm * 32),
                 w_seed = stage_seeds ? align_up(nbatch * 32) : 0, w_ts = d_ts ? 0 : align_up(nbatch * BPGPU_TRANSCRIPT_BYTES);
    const size_t need = w_gs + w_mo + w_ms + w_f + w_p + 10 * w_v + w_q + 2 * w_gen + w_seed + w_ts;
    if ((rc = rpp_reserve(c, need))) return rc;
    char *wb = c->rpp_buf;
    uint32_t *gsc = (uint32_t *)wb, *mo = (uint32_t *)(wb + w_gs);
    uint8_t *mst = (uint8_t *)mo + w_mo;
    uint32_t *fields = (uint32_t *)(mst + w_ms), *party = (uint32_t *)((char *)fields + w_f);
    char *vv = (char *)party + w_p;
    uint32_t *sL = (uint32_t *)vv, *sR = (uint32_t *)(vv + w_v), *l0 = (uint32_t *)(vv + 2 * w_v), *l1 = (uint32_t *)(vv + 3 * w_v), *r0 = (uint32_t *)(vv + 4 * w_v),
             *r1 = (uint32_t *)(vv + 5 * w_v), *avec = (uint32_t *)(vv + 6 * w_v), *bvec = (uint32_t *)(vv + 7 * w_v), *Gf = (uint32_t *)(vv + 8 * w_v),
             *Hf = (uint32_t *)(vv + 9 * w_v);
    uint32_t *qenc = (uint32_t *)(vv + 10 * w_v), *Genc = (uint32_t *)((char *)qenc + w_q), *Henc = (uint32_t *)((char *)Genc + w_gen);
    char *seed_slot = (char *)Henc + w_gen;
    if (!d_ts) d_ts = (uint32_t *)(seed_slot + w_seed);
    const uint32_t nb32 = (uint32_t)nbatch, nbits = (uint32_t)(nbatch * nm), n_b = (nb32 + BP_BLOCK - 1) / BP_BLOCK;
    do {
        if (stage_seeds) {   // library-drawn seeds of a device-pointer call: pinned staging -> the working set (cleared with it)
            // and wait for that one copy: the caller clears the staged seeds when this returns
            if (hipMemcpyAsync(seed_slot, stage_seeds, nbatch * 32, hipMemcpyHostToDevice, s) != hipSuccess || c->io.pin_mark(s) ||
                hipEventSynchronize(c->io.pin_ev) != hipSuccess) {
                rc = fail(c, BPGPU_ERR_HIP, "staging the seeds failed");
                break;
            }
            c->io.pin_pending = false;
            src.seeds = (const uint8_t *)seed_slot;
        }
        uint32_t *d_ids = nullptr;
        rc = gen_ids_for(c, n, m, &d_ids);
        if (rc) break;
        LAUNCH(c, s, "gather32", k_gather32, ((uint32_t)(2 * nm) + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, (uint32_t)(2 * nm), (const uint32_t *)(d_ids + 2),
               (const uint32_t *)c->d_gens, Genc);   // G(n, m) then H(n, m): Henc = Genc + nm records when w_gen is exact
        if (hipMemsetAsync(gsc, 0, gs_bytes, s) != hipSuccess || hipMemsetAsync(d_proofs, 0, nbatch * proof_len, s) != hipSuccess) {
            rc = fail(c, BPGPU_ERR_HIP, "memset failed");
            break;
        }
        // (1) V_j, A, S
        if (src.rw)
            LAUNCH(c, s, "rpp_commit1_rw", k_rpp_commit1_rw, n_b + (nbits + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, n_b, nbits, sh, d_values, d_bl, src.seeds, src.messages, gsc,
                   party, sL, sR);
        else if (seeded)
            LAUNCH(c, s, "rpp_commit1_seed", k_rpp_commit1_seed, n_b + (nbits + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, n_b, nbits, sh, d_values, d_bl, src.seeds, gsc, party,
                   sL, sR);
        else
            LAUNCH(c, s, "rpp_commit1", k_rpp_commit1, n_b + (nbits + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, n_b, nbits, sh, d_values, d_bl, src.rng, gsc, party, sL, sR);
        rc = msm_shared_dev_locked(c, n, m, nmsm1, 0, gsc, nullptr, nullptr, mo, mst, nullptr, s, false, c->prover_ct);
        if (rc) break;
        if (src.ts_in)
            LAUNCH(c, s, "rpp_chal1_sep", k_rpp_chal1_sep, (nb32 + RP_BLOCK - 1) / RP_BLOCK, RP_BLOCK, sh, (const uint32_t *)mo, src.ts_in, src.ts_in_stride, d_ts, fields,
                   d_proofs, d_coms);
        else
            LAUNCH(c, s, "rpp_chal1", k_rpp_chal1, (nb32 + RP_BLOCK - 1) / RP_BLOCK, RP_BLOCK, sh, (const uint32_t *)mo, d_ts, fields, d_proofs, d_coms);
        // (2) polynomials, T_1, T_2
        const uint32_t npar = (uint32_t)(nbatch * m);
        LAUNCH(c, s, "rpp_poly", k_rpp_poly, (npar + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, npar, sh, d_values, (const uint32_t *)fields, (const uint32_t *)sL,
               (const uint32_t *)sR, l0, l1, r0, r1, party);
        if (hipMemsetAsync(gsc, 0, (size_t)2 * nbatch * sh.n_gen_terms * 32, s) != hipSuccess) {
            rc = fail(c, BPGPU_ERR_HIP, "memset failed");
            break;
        }
        if (seeded) LAUNCH(c, s, "rpp_tcommit_seed", k_rpp_tcommit_seed, n_b, BP_BLOCK, sh, src.seeds, gsc, party);
        else LAUNCH(c, s, "rpp_tcommit", k_rpp_tcommit, n_b, BP_BLOCK, sh, src.rng, gsc, party);
        rc = msm_shared_dev_locked(c, n, m, 2 * nbatch, 0, gsc, nullptr, nullptr, mo, mst, nullptr, s, false, c->prover_ct);
        if (rc) break;
        // (3) x, t_x ..., w; Q = w B; the inner-product argument's inputs
        if (hipMemsetAsync(gsc, 0, (size_t)nbatch * sh.n_gen_terms * 32, s) != hipSuccess) {
            rc = fail(c, BPGPU_ERR_HIP, "memset failed");
            break;
        }
        LAUNCH(c, s, "rpp_chal2", k_rpp_chal2, (nb32 + RP_BLOCK - 1) / RP_BLOCK, RP_BLOCK, sh, (const uint32_t *)mo, d_ts, fields, (const uint32_t *)party, gsc,
               d_proofs);
        LAUNCH(c, s, "rpp_vectors", k_rpp_vectors, (nbits + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, nbits, sh, (const uint32_t *)fields, (const uint32_t *)l0,
               (const uint32_t *)l1, (const uint32_t *)r0, (const uint32_t *)r1, avec, bvec, Gf, Hf);
        // (4) InnerProductProof::create over G(n, m), H(n, m) with Q = w B (dealer.rs:279-293): every L_j / R_j is a generator-table
        // MSM (the Q term is (c w) on B); L, R pairs and a, b go behind the 7 fixed elements of the proof
        ippc_fixed fx;
        fx.gn = n;
        fx.gm = m;
        fx.w = fields + (size_t)RPP_W * nbatch * 8;
        fx.gen_scalars = gsc;
        rc = ippc_core(c, s, nm, k, nbatch, avec, bvec, Gf, Hf, qenc, Genc, Genc + 8 * nm, 1, d_ts, d_proofs + 224, proof_len, nullptr, &fx);
    } while (0);
    return rc;
}

// ---- the callers' own transcripts, one seed per proof (rp_prover.h: rpp_from_seed, rpp_chal1_lane<true>) ----
static int rpp_ts_args(bpgpu_ctx *c, size_t n, size_t m, size_t transcript_stride) {
    int rc = rpp_check_nm(c, n, m);
    if (rc) return rc;
    if (transcript_stride != 0 && transcript_stride != BPGPU_TRANSCRIPT_BYTES)
        return fail(c, BPGPU_ERR_INVALID_ARG, "transcript_stride must be 0 or %d", BPGPU_TRANSCRIPT_BYTES);
    return BPGPU_OK;
}

// the argument rule of the rewindable forms beyond the seeded ones': one party, and a seed that somebody holds
static int rpp_rw_args(bpgpu_ctx *c, size_t m, const void *rng32) {
    if (m != 1) return fail(c, BPGPU_ERR_INVALID_ARG, "rewindable proofs have m = 1: the parties of an aggregated proof cannot be separated");
    if (!rng32) return fail(c, BPGPU_ERR_INVALID_ARG, "rng32 missing: a rewindable proof is rewound with its seed");
    return BPGPU_OK;
}

// host pointers, the seeded form and (rw) the rewindable one: messages may be null
static int rpp_ts_host_call(bpgpu_ctx *c, size_t n, size_t m, size_t nbatch, const uint64_t *values, const uint8_t *blindings, const uint8_t *transcripts,
                            size_t transcript_stride, const uint8_t *rng32, bool rw, const uint8_t *messages, uint8_t *proofs_out, uint8_t *commitments_out,
                            uint8_t *transcripts_out) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    if (nbatch == 0) return BPGPU_OK;
    if (!values || !blindings || !proofs_out || !commitments_out) return BPGPU_ERR_INVALID_ARG;
    if (!transcripts) return fail(c, BPGPU_ERR_INVALID_ARG, "transcripts missing");
    int rc = rpp_ts_args(c, n, m, transcript_stride);
    if (rc) return rc;
    if (rw && (rc = rpp_rw_args(c, m, rng32))) return rc;
    const size_t TS = BPGPU_TRANSCRIPT_BYTES, nstates = transcript_stride ? nbatch : 1;
    for (size_t p = 0; p < nstates; p++)
        if (!ts_state_ok(transcripts + p * TS)) return fail(c, BPGPU_ERR_INVALID_ARG, "malformed transcript state %zu", p);
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    rpp_shape sh;
    if ((rc = rpp_shape_locked(c, n, m, nbatch, values, sh))) return rc;
    const size_t proof_len = sh.proof_len;
    hipStream_t s = c->stream;
    // ---- inputs through pinned staging into the persistent IO buffer: 32 bytes of randomness per proof, no draw buffer
    host_call<bpgpu_ctx> io(c, s);
    const int r_val = io.in(nbatch * m * 8), r_bl = io.in(nbatch * m * 32), r_seed = io.in(nbatch * 32), r_msg = io.in(messages ? nbatch * 16 : 0),
              r_ts = io.in(nstates * TS);
    const int r_pr = io.out(nbatch * proof_len), r_cm = io.out(nbatch * m * 32), r_to = io.out(nbatch * TS);
    io.secrets(io.off[r_ts]);   // values, blindings, the seeds, the messages
    rc = io.open();
    if (rc) return io.finish(rc);
    io.put(r_val, values, nbatch * m * 8);
    io.put(r_bl, blindings, nbatch * m * 32);
    if (rng32) io.put(r_seed, rng32, nbatch * 32);
    else if ((rc = os_random(c, io.h(r_seed), nbatch * 32)) != 0) return io.finish(rc);
    if (messages) io.put(r_msg, messages, nbatch * 16);
    io.put(r_ts, transcripts, nstates * TS);
    if ((rc = io.upload())) return io.finish(rc);
    rpp_source src;
    src.rw = rw;
    src.messages = messages ? (const uint32_t *)io.d(r_msg) : nullptr;
    src.seeds = (const uint8_t *)io.d(r_seed);
    src.ts_in = (const uint32_t *)io.d(r_ts);
    src.ts_in_stride = transcript_stride ? BP_TS_WORDS : 0;
    rc = rpp_chain(c, s, sh, (const uint64_t *)io.d(r_val), (const uint8_t *)io.d(r_bl), src, (uint32_t *)io.d(r_to), (uint8_t *)io.d(r_pr), (uint8_t *)io.d(r_cm),
                   nullptr);
    rc = io.finish(io.download(rc));
    if (rc) return rc;
    memcpy(proofs_out, io.h(r_pr), nbatch * proof_len);
    memcpy(commitments_out, io.h(r_cm), nbatch * m * 32);
    if (transcripts_out) memcpy(transcripts_out, io.h(r_to), nbatch * TS);
    return BPGPU_OK;
}
extern "C" int bpgpu_rangeproof_prove_batch_ts(bpgpu_ctx *c, size_t n, size_t m, size_t nbatch, const uint64_t *values, const uint8_t *blindings,
                                               const uint8_t *transcripts, size_t transcript_stride, const uint8_t *rng32, uint8_t *proofs_out,
                                               uint8_t *commitments_out, uint8_t *transcripts_out) {
    return rpp_ts_host_call(c, n, m, nbatch, values, blindings, transcripts, transcript_stride, rng32, false, nullptr, proofs_out, commitments_out, transcripts_out);
}
extern "C" int bpgpu_rangeproof_prove_batch_rw(bpgpu_ctx *c, size_t n, size_t m, size_t nbatch, const uint64_t *values, const uint8_t *blindings,
                                               const uint8_t *transcripts, size_t transcript_stride, const uint8_t *rng32, const uint8_t *messages,
                                               uint8_t *proofs_out, uint8_t *commitments_out, uint8_t *transcripts_out) {
    return rpp_ts_host_call(c, n, m, nbatch, values, blindings, transcripts, transcript_stride, rng32, true, messages, proofs_out, commitments_out, transcripts_out);
}

static int rpp_ts_dev_call(bpgpu_ctx *c, size_t n, size_t m, size_t nbatch, const void *d_values, const void *d_blindings, const void *d_transcripts,
                           size_t transcript_stride, const void *d_rng32, bool rw, const void *d_messages, void *d_proofs_out, void *d_commitments_out,
                           void *d_transcripts_out, void *stream) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    if (nbatch == 0) return BPGPU_OK;
    if (!d_values || !d_blindings || !d_proofs_out || !d_commitments_out) return BPGPU_ERR_INVALID_ARG;
    if (!d_transcripts) return fail(c, BPGPU_ERR_INVALID_ARG, "transcripts missing");
    int rc = rpp_ts_args(c, n, m, transcript_stride);
    if (rc) return rc;
    if (rw && (rc = rpp_rw_args(c, m, d_rng32))) return rc;
    if (((uintptr_t)d_values & 7) || (((uintptr_t)d_blindings | (uintptr_t)d_transcripts | (uintptr_t)d_rng32 | (uintptr_t)d_proofs_out | (uintptr_t)d_commitments_out |
                                       (uintptr_t)d_transcripts_out | (uintptr_t)d_messages) & 3))
        return fail(c, BPGPU_ERR_INVALID_ARG, "device buffers must be 4-byte aligned (values: 8-byte)");
    dev_scope<bpgpu_ctx> sc(c);
    if (sc.rc) return sc.rc;
    rpp_shape sh;
    if ((rc = rpp_shape_locked(c, n, m, nbatch, nullptr, sh))) return rc;
    if ((rc = sc.enter(stream))) return rc;
    hipStream_t s = sc.s;
    char *h_seeds = nullptr;
    if (!d_rng32) {   // the library's own seeds: drawn into pinned staging, copied by the chain into its working set
        rc = c->io.pin_alloc(nbatch * 32, &h_seeds);
        if (!rc) rc = os_random(c, h_seeds, nbatch * 32);
    }
    rpp_source src;
    src.rw = rw;
    src.messages = (const uint32_t *)d_messages;
    src.seeds = (const uint8_t *)d_rng32;
    src.ts_in = (const uint32_t *)d_transcripts;
    src.ts_in_stride = transcript_stride ? BP_TS_WORDS : 0;
    if (!rc) rc = rpp_chain(c, s, sh, (const uint64_t *)d_values, (const uint8_t *)d_blindings, src, (uint32_t *)d_transcripts_out, (uint8_t *)d_proofs_out,
                            (uint8_t *)d_commitments_out, h_seeds);
    // the exit of a prover (host_call::finish) without its wait: working sets and arena cleared on the stream behind the last kernel
    dev_span b[3];
    secret_spans(c, b);
    bool ok = true;
    for (const dev_span &x : b)
        if (x.p) ok = hipMemsetAsync(x.p, 0, x.bytes, s) == hipSuccess && ok;
    const int rc2 = sc.leave();
    if (h_seeds) {   // (the chain has waited until the seeds had left the staging block: the one wait of this form)
        memset(h_seeds, 0, nbatch * 32);
        c->io.last_secret_bytes = (h_seeds == c->io.pin) ? nbatch * 32 : 0;
    }
    if (!rc && !ok) rc = fail(c, BPGPU_ERR_HIP, "clearing the prover's working set failed");
    return rc ? rc : rc2;
}
extern "C" int bpgpu_rangeproof_prove_batch_ts_dev(bpgpu_ctx *c, size_t n, size_t m, size_t nbatch, const void *d_values, const void *d_blindings,
                                                   const void *d_transcripts, size_t transcript_stride, const void *d_rng32, void *d_proofs_out,
                                                   void *d_commitments_out, void *d_transcripts_out, void *stream) {
    return rpp_ts_dev_call(c, n, m, nbatch, d_values, d_blindings, d_transcripts, transcript_stride, d_rng32, false, nullptr, d_proofs_out, d_commitments_out,
                           d_transcripts_out, stream);
}
extern "C" int bpgpu_rangeproof_prove_batch_rw_dev(bpgpu_ctx *c, size_t n, size_t m, size_t nbatch, const void *d_values, const void *d_blindings,
                                                   const void *d_transcripts, size_t transcript_stride, const void *d_rng32, const void *d_messages,
                                                   void *d_proofs_out, void *d_commitments_out, void *d_transcripts_out, void *stream) {
    return rpp_ts_dev_call(c, n, m, nbatch, d_values, d_blindings, d_transcripts, transcript_stride, d_rng32, true, d_messages, d_proofs_out, d_commitments_out,
                           d_transcripts_out, stream);
}

// ============================================================================
// batches of Pedersen commitments and openings (pedersen.h): one launch, lane = row
// ============================================================================
#define PED_MAX_BATCH ((size_t)1 << 28)
// the argument rules the four entry points share; commit = false: the open forms (blindings required, no seed)
static int ped_check_args(bpgpu_ctx *c, size_t nbatch, size_t value_bytes, const void *values, const void *blindings, const void *seed, uint64_t first_draw,
                          const void *blindings_out, bool commit) {
    if (value_bytes != 8 && value_bytes != 32) return fail(c, BPGPU_ERR_INVALID_ARG, "value_bytes must be 8 (u64) or 32 (scalars)");
    if (nbatch > PED_MAX_BATCH) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large: at most 2^28 rows per call");
    if (!values) return fail(c, BPGPU_ERR_INVALID_ARG, "values missing");
    if (!commit) return blindings ? BPGPU_OK : fail(c, BPGPU_ERR_INVALID_ARG, "blindings missing");
    if (blindings && (seed || first_draw)) return fail(c, BPGPU_ERR_INVALID_ARG, "blindings given: rng_seed32 must be NULL and first_draw 0");
    if (!blindings && !seed && !blindings_out)
        return fail(c, BPGPU_ERR_INVALID_ARG, "the library draws the seed: blindings_out is required (nothing else tells the caller the openings)");
    return BPGPU_OK;
}
// enqueue the one launch on s.  d_commitments_in != nullptr: the open form (verdicts to d_verdict); else the commit form, constant-time
// under the context option "prover_constant_time" (its own small-window table, built on first use)
static int ped_launch_locked(bpgpu_ctx *c, hipStream_t s, size_t nbatch, const void *d_values, size_t value_bytes, const void *d_blindings, const void *d_seed,
                             uint64_t first_draw, const void *d_commitments_in, void *d_out, void *d_blindings_out, void *d_status) {
    uint32_t *d_ids = nullptr;
    int rc = gen_ids_for(c, 1, 1, &d_ids);   // the shared path's list: [0] = B_blinding, [1] = B
    if (rc) return rc;
    const bool ct = !d_commitments_in && c->prover_ct;
    fb_walk w;
    if ((rc = fb_walk_for(c, ct, w))) return rc;
    ped_in in;
    in.values = (const uint32_t *)d_values;
    in.value_words = (uint32_t)(value_bytes / 4);
    in.blindings = (const uint32_t *)d_blindings;
    in.seed32 = (const uint8_t *)d_seed;
    in.first_draw = first_draw;
    const uint32_t nb = (uint32_t)nbatch, grid = (nb + BP_BLOCK - 1) / BP_BLOCK;
    if (d_commitments_in)
        LAUNCH(c, s, "ped_open", k_ped_open, grid, BP_BLOCK, nb, in, (const uint32_t *)d_commitments_in, c->prm, (const uint32_t *)d_ids, (const fb_entry *)c->d_table,
               (uint8_t *)d_out);
    else
        LAUNCH_CT(c, s, ct, "ped_commit", k_ped_commit, grid, BP_BLOCK, nb, in, w.prm, (const uint32_t *)d_ids, w.table, (uint32_t *)d_out, (uint32_t *)d_blindings_out,
                  (uint8_t *)d_status);
    if (hipGetLastError() != hipSuccess) return fail(c, BPGPU_ERR_HIP, "launch failed");
    return BPGPU_OK;
}

extern "C" int bpgpu_pedersen_commit_batch(bpgpu_ctx *c, size_t nbatch, const void *values, size_t value_bytes, const uint8_t *blindings, const uint8_t *rng_seed32,
                                           uint64_t first_draw, uint8_t *commitments_out, uint8_t *blindings_out, uint8_t *status_out) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    if (nbatch == 0) return BPGPU_OK;
    int rc = ped_check_args(c, nbatch, value_bytes, values, blindings, rng_seed32, first_draw, blindings_out, true);
    if (rc) return rc;
    if (!commitments_out || !status_out) return fail(c, BPGPU_ERR_INVALID_ARG, "commitments_out and status_out are required");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    hipStream_t s = c->stream;
    // values, blindings and the seed through the provers' staging: the secret span is every input
    host_call<bpgpu_ctx> io(c, s);
    const int r_val = io.in(nbatch * value_bytes), r_bl = io.in(blindings ? nbatch * 32 : 0), r_seed = io.in(32);
    const int r_blo = io.out(blindings_out ? nbatch * 32 : 0), r_cm = io.out(nbatch * 32), r_st = io.out(nbatch);
    io.secrets(io.in_bytes());
    rc = io.open();
    if (rc) return io.finish(rc);
    io.put(r_val, values, nbatch * value_bytes);
    if (blindings) io.put(r_bl, blindings, nbatch * 32);
    else if (rng_seed32) io.put(r_seed, rng_seed32, 32);
    else if ((rc = os_random(c, io.h(r_seed), 32)) != 0) return io.finish(rc);
    if ((rc = io.upload())) return io.finish(rc);
    rc = ped_launch_locked(c, s, nbatch, io.d(r_val), value_bytes, blindings ? io.d(r_bl) : nullptr, blindings ? nullptr : io.d(r_seed), first_draw, nullptr, io.d(r_cm),
                           blindings_out ? io.d(r_blo) : nullptr, io.d(r_st));
    rc = io.finish(io.download(rc));
    if (blindings_out) {   // the staged copy of the blindings is a secret too: handed over, then cleared
        if (!rc) memcpy(blindings_out, io.h(r_blo), nbatch * 32);
        memset(io.h(r_blo), 0, nbatch * 32);
        if (io.hb == c->io.pin) c->io.last_secret_bytes = io.off[r_blo + 1];   // (the first output region: the secret span grows by it)
    }
    if (rc) return rc;
    memcpy(commitments_out, io.h(r_cm), nbatch * 32);
    memcpy(status_out, io.h(r_st), nbatch);
    return BPGPU_OK;
}

extern "C" int bpgpu_pedersen_open_batch(bpgpu_ctx *c, size_t nbatch, const uint8_t *commitments, const void *values, size_t value_bytes, const uint8_t *blindings,
                                         uint8_t *verdict_out) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    if (nbatch == 0) return BPGPU_OK;
    int rc = ped_check_args(c, nbatch, value_bytes, values, blindings, nullptr, 0, nullptr, false);
    if (rc) return rc;
    if (!commitments || !verdict_out) return fail(c, BPGPU_ERR_INVALID_ARG, "commitments and verdict_out are required");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    hipStream_t s = c->stream;
    host_call<bpgpu_ctx> io(c, s);
    const int r_val = io.in(nbatch * value_bytes), r_bl = io.in(nbatch * 32), r_cm = io.in(nbatch * 32);
    const int r_vd = io.out(nbatch);
    io.secrets(io.off[r_cm]);   // an opening is a secret of whoever made it, public only to this verifier
    rc = io.open();
    if (rc) return io.finish(rc);
    io.put(r_val, values, nbatch * value_bytes);
    io.put(r_bl, blindings, nbatch * 32);
    io.put(r_cm, commitments, nbatch * 32);
    if ((rc = io.upload())) return io.finish(rc);
    rc = ped_launch_locked(c, s, nbatch, io.d(r_val), value_bytes, io.d(r_bl), nullptr, 0, io.d(r_cm), io.d(r_vd), nullptr, nullptr);
    rc = io.finish(io.download(rc));
    if (rc) return rc;
    memcpy(verdict_out, io.h(r_vd), nbatch);
    return BPGPU_OK;
}

extern "C" int bpgpu_pedersen_commit_batch_dev(bpgpu_ctx *c, size_t nbatch, const void *d_values, size_t value_bytes, const void *d_blindings, const void *d_rng_seed32,
                                               uint64_t first_draw, void *d_commitments_out, void *d_blindings_out, void *d_status_out, void *stream) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    if (nbatch == 0) return BPGPU_OK;
    int rc = ped_check_args(c, nbatch, value_bytes, d_values, d_blindings, d_rng_seed32, first_draw, d_blindings_out, true);
    if (rc) return rc;
    if (!d_commitments_out || !d_status_out) return fail(c, BPGPU_ERR_INVALID_ARG, "commitments_out and status_out are required");
    if (((uintptr_t)d_values | (uintptr_t)d_blindings | (uintptr_t)d_rng_seed32 | (uintptr_t)d_commitments_out | (uintptr_t)d_blindings_out) & 3)
        return fail(c, BPGPU_ERR_INVALID_ARG, "device buffers must be 4-byte aligned");
    dev_scope<bpgpu_ctx> sc(c);
    if (sc.rc) return sc.rc;
    if (!c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    if ((rc = sc.enter(stream))) return rc;
    hipStream_t s = sc.s;
    char *h_seed = nullptr;
    const void *d_seed = d_rng_seed32;
    size_t slot_bytes = 256;
    do {
        if (!d_blindings && !d_rng_seed32) {   // the library's own seed: pinned staging -> a slot of the arena, cleared behind the kernel
            const bool fresh = c->arena_cap < 256;   // (an arena allocated here is cleared whole: the allocator hands out what its last owner left)
            if ((rc = arena_reserve(c, 256)) || (rc = c->io.pin_alloc(32, &h_seed)) || (rc = os_random(c, h_seed, 32))) break;
            if (fresh) slot_bytes = c->arena_cap;
            // ... and wait for that one copy, so that the staged seed can be cleared before this returns (the one wait of this form)
            if (hipMemcpyAsync(c->arena, h_seed, 32, hipMemcpyHostToDevice, s) != hipSuccess || c->io.pin_mark(s) || hipEventSynchronize(c->io.pin_ev) != hipSuccess) {
                rc = fail(c, BPGPU_ERR_HIP, "staging the seed failed");
                break;
            }
            c->io.pin_pending = false;
            d_seed = c->arena;
        }
        rc = ped_launch_locked(c, s, nbatch, d_values, value_bytes, d_blindings, d_blindings ? nullptr : d_seed, first_draw, nullptr, d_commitments_out, d_blindings_out,
                               d_status_out);
    } while (0);
    bool ok = true;
    if (h_seed) {
        if (c->arena) ok = hipMemsetAsync(c->arena, 0, slot_bytes, s) == hipSuccess;
        memset(h_seed, 0, 32);
        c->io.last_secret_bytes = (h_seed == c->io.pin) ? 32 : 0;
    }
    const int rc2 = sc.leave();
    if (!rc && !ok) rc = fail(c, BPGPU_ERR_HIP, "clearing the seed slot failed");
    return rc ? rc : rc2;
}

extern "C" int bpgpu_pedersen_open_batch_dev(bpgpu_ctx *c, size_t nbatch, const void *d_commitments, const void *d_values, size_t value_bytes, const void *d_blindings,
                                             void *d_verdict_out, void *stream) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    if (nbatch == 0) return BPGPU_OK;
    int rc = ped_check_args(c, nbatch, value_bytes, d_values, d_blindings, nullptr, 0, nullptr, false);
    if (rc) return rc;
    if (!d_commitments || !d_verdict_out) return fail(c, BPGPU_ERR_INVALID_ARG, "commitments and verdict_out are required");
    if (((uintptr_t)d_values | (uintptr_t)d_blindings | (uintptr_t)d_commitments) & 3) return fail(c, BPGPU_ERR_INVALID_ARG, "device buffers must be 4-byte aligned");
    return dev_call(
        c, stream, [&] { return c->d_table ? BPGPU_OK : fail(c, BPGPU_ERR_NO_GENS, "generators not loaded"); },
        [&](hipStream_t s) { return ped_launch_locked(c, s, nbatch, d_values, value_bytes, d_blindings, nullptr, 0, d_commitments, d_verdict_out, nullptr, nullptr); });
}

// ============================================================================
// signed sums of Pedersen commitments and the balance check (pedersen_sum.h): term launch, reduce passes, finish launch
// ============================================================================
// the argument rules the four entry points share; fills the plan (host: row_offsets never leaves it but as the plan table)
static int psum_check_args(bpgpu_ctx *c, size_t nbatch, const uint32_t *row_offsets, const void *points, const void *values, size_t value_bytes, psum_plan &pl) {
    if (nbatch > PED_MAX_BATCH) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large: at most 2^28 rows per call");
    if (!row_offsets) return fail(c, BPGPU_ERR_INVALID_ARG, "row_offsets missing");
    if (values && value_bytes != 8 && value_bytes != 32) return fail(c, BPGPU_ERR_INVALID_ARG, "value_bytes must be 8 (u64) or 32 (scalars)");
    if (row_offsets[0] != 0) return fail(c, BPGPU_ERR_INVALID_ARG, "row_offsets must start at 0");
    for (size_t r = 0; r < nbatch; r++)
        if (row_offsets[r + 1] < row_offsets[r]) return fail(c, BPGPU_ERR_INVALID_ARG, "row_offsets must not decrease");
    if (row_offsets[nbatch] > PED_MAX_BATCH) return fail(c, BPGPU_ERR_INVALID_ARG, "too many terms: at most 2^28 per call");
    if (row_offsets[nbatch] && !points) return fail(c, BPGPU_ERR_INVALID_ARG, "points missing");
    try {   // (the table has (passes + 1)(nbatch + 1) words: gigabytes at the documented limit)
        psum_make_plan(pl, (uint32_t)nbatch, row_offsets);
    } catch (const std::bad_alloc &) {
        return fail(c, BPGPU_ERR_INVALID_ARG, "out of host memory for the plan table of %zu rows", nbatch);
    }
    return BPGPU_OK;
}
// the call's working set in the arena: [plan table (the _dev forms; the host forms stage it with their inputs)][row flags][partials]
struct psum_arena {
    size_t off_tab, off_bad, off_part, total;
    psum_arena(const psum_plan &pl, bool with_table) {
        arena_plan ap;
        off_tab = ap.add(with_table ? pl.table.size() * 4 : 0);
        off_bad = ap.add(pl.nbatch);
        off_part = ap.add((size_t)pl.partials() * sizeof(ge_ext));
        total = ap.total;
    }
};
// enqueue the launches on s.  d_tab: the plan table on the device.  balance: verdicts to d_status; else sums to d_out and BPGPU_MSM_*
// bytes to d_status, the walk constant-time under the context option "prover_constant_time" (its own small-window table, built on
// first use).  Without a scalar no generator is touched.
static int psum_launch_locked(bpgpu_ctx *c, hipStream_t s, const psum_plan &pl, const psum_arena &ar, const uint32_t *d_tab, const void *d_points, const void *d_signs,
                              const void *d_values, size_t value_bytes, const void *d_blindings, bool balance, void *d_out, void *d_status) {
    const bool scalars = d_values || d_blindings;
    uint32_t *d_ids = nullptr;
    int rc;
    if (scalars && (rc = gen_ids_for(c, 1, 1, &d_ids))) return rc;   // the shared path's list: [0] = B_blinding, [1] = B
    const bool ct = scalars && !balance && c->prover_ct;
    if (ct && (rc = build_ct_table(c))) return rc;
    ped_in in;
    in.values = (const uint32_t *)d_values;
    in.value_words = (uint32_t)(value_bytes / 4);
    in.blindings = (const uint32_t *)d_blindings;
    in.seed32 = nullptr;
    in.first_draw = 0;
    const uint32_t nb = pl.nbatch, stride = nb + 1;
    uint8_t *d_bad = (uint8_t *)(c->arena + ar.off_bad);
    ge_ext *src = (ge_ext *)(c->arena + ar.off_part), *dst = src;
    HIPCHK(c, hipMemsetAsync(d_bad, 0, nb, s));
    for (uint32_t k = 0; k < pl.npasses && pl.items(0); k++) {
        const psum_pass ps = {pl.items(k), nb, d_tab + (size_t)k * stride, d_tab + (size_t)(k + 1) * stride};
        const uint32_t grid = (ps.total + PSUM_BLOCK - 1) / PSUM_BLOCK;
        if (k == 0) LAUNCH(c, s, "psum_terms", k_psum_terms, grid, PSUM_BLOCK, ps, (const uint32_t *)d_points, (const uint8_t *)d_signs, d_bad, dst);
        else LAUNCH(c, s, "psum_reduce", k_psum_reduce, grid, PSUM_BLOCK, ps, (const ge_ext *)src, dst);
        src = dst;
        dst += pl.items(k + 1);
    }
    const uint32_t *d_slot = d_tab + (size_t)pl.npasses * stride;
    const fb_params prm = scalars ? (ct ? c->prm_ct : c->prm) : fb_params();
    const fb_entry *table = scalars ? (const fb_entry *)(ct ? c->d_table_ct : c->d_table) : nullptr;
    const uint32_t grid = (nb + BP_BLOCK - 1) / BP_BLOCK;
    if (balance)
        LAUNCH(c, s, "psum_balance", k_psum_balance, grid, BP_BLOCK, nb, in, prm, (const uint32_t *)d_ids, table, d_slot, (const ge_ext *)src, (const uint8_t *)d_bad,
               (uint8_t *)d_status);
    else
        LAUNCH_CT(c, s, ct, "psum_finish", k_psum_finish, grid, BP_BLOCK, nb, in, prm, (const uint32_t *)d_ids, table, d_slot, (const ge_ext *)src, (const uint8_t *)d_bad,
                  (uint32_t *)d_out, (uint8_t *)d_status);
    if (hipGetLastError() != hipSuccess) return fail(c, BPGPU_ERR_HIP, "launch failed");
    return BPGPU_OK;
}

// the host forms: values and blindings lead the staged inputs -- the secret span of the sum form; out == nullptr: the balance form
static int psum_host(bpgpu_ctx *c, size_t nbatch, const uint32_t *row_offsets, const uint8_t *points, const uint8_t *signs, const void *values, size_t value_bytes,
                     const uint8_t *blindings, uint8_t *out, uint8_t *status) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    if (nbatch == 0) return BPGPU_OK;
    const bool balance = !out;
    psum_plan pl;
    int rc = psum_check_args(c, nbatch, row_offsets, points, values, value_bytes, pl);
    if (rc) return rc;
    if (!status) return fail(c, BPGPU_ERR_INVALID_ARG, balance ? "verdict_out is required" : "out and status_out are required");
    const size_t total = row_offsets[nbatch];
    for (size_t t = 0; signs && t < total; t++)
        if (signs[t] > 1) return fail(c, BPGPU_ERR_INVALID_ARG, "a sign byte is 0 (add) or 1 (subtract)");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if ((values || blindings) && !c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    hipStream_t s = c->stream;
    host_call<bpgpu_ctx> io(c, s);
    const int r_val = io.in(values ? nbatch * value_bytes : 0), r_bl = io.in(blindings ? nbatch * 32 : 0), r_tab = io.in(pl.table.size() * 4);
    const int r_pts = io.in(total * 32), r_sg = io.in(signs ? total : 0);
    const int r_out = io.out(balance ? 0 : nbatch * 32), r_st = io.out(nbatch);
    if (values || blindings) io.secrets(io.off[r_tab]);   // a wallet's (value, blinding), or an opening shown to this verifier alone (as bpgpu_pedersen_open_batch); the commitments are public
    rc = io.open();
    if (rc) return io.finish(rc);
    const psum_arena ar(pl, false);
    if ((rc = arena_reserve(c, ar.total))) return io.finish(rc);
    if (values) io.put(r_val, values, nbatch * value_bytes);
    if (blindings) io.put(r_bl, blindings, nbatch * 32);
    io.put(r_tab, pl.table.data(), pl.table.size() * 4);
    if (total) io.put(r_pts, points, total * 32);
    if (signs && total) io.put(r_sg, signs, total);
    if ((rc = io.upload())) return io.finish(rc);
    rc = psum_launch_locked(c, s, pl, ar, (const uint32_t *)io.d(r_tab), io.d(r_pts), signs ? io.d(r_sg) : nullptr, values ? io.d(r_val) : nullptr, value_bytes,
                            blindings ? io.d(r_bl) : nullptr, balance, balance ? nullptr : io.d(r_out), io.d(r_st));
    rc = io.finish(io.download(rc));
    if (rc) return rc;
    if (!balance) memcpy(out, io.h(r_out), nbatch * 32);
    memcpy(status, io.h(r_st), nbatch);
    return BPGPU_OK;
}
extern "C" int bpgpu_pedersen_sum_batch(bpgpu_ctx *c, size_t nbatch, const uint32_t *row_offsets, const uint8_t *points, const uint8_t *signs, const void *values,
                                        size_t value_bytes, const uint8_t *blindings, uint8_t *out, uint8_t *status_out) {
    if (c && nbatch && !out) return fail(c, BPGPU_ERR_INVALID_ARG, "out and status_out are required");
    return psum_host(c, nbatch, row_offsets, points, signs, values, value_bytes, blindings, out, status_out);
}
extern "C" int bpgpu_pedersen_balance_batch(bpgpu_ctx *c, size_t nbatch, const uint32_t *row_offsets, const uint8_t *points, const uint8_t *signs, const void *values,
                                            size_t value_bytes, const uint8_t *blindings, uint8_t *verdict_out) {
    return psum_host(c, nbatch, row_offsets, points, signs, values, value_bytes, blindings, nullptr, verdict_out);
}

// the _dev forms: row_offsets stays a host array (the launch geometry follows from it); the plan table is the only host -> device traffic
static int psum_dev(bpgpu_ctx *c, size_t nbatch, const uint32_t *row_offsets, const void *d_points, const void *d_signs, const void *d_values, size_t value_bytes,
                    const void *d_blindings, void *d_out, void *d_status, void *stream) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    if (nbatch == 0) return BPGPU_OK;
    const bool balance = !d_out;
    psum_plan pl;
    int rc = psum_check_args(c, nbatch, row_offsets, d_points, d_values, value_bytes, pl);
    if (rc) return rc;
    if (!d_status) return fail(c, BPGPU_ERR_INVALID_ARG, balance ? "verdict_out is required" : "out and status_out are required");
    if (((uintptr_t)d_points | (uintptr_t)d_values | (uintptr_t)d_blindings | (uintptr_t)d_out) & 3) return fail(c, BPGPU_ERR_INVALID_ARG, "device buffers must be 4-byte aligned");
    dev_scope<bpgpu_ctx> sc(c);
    if (sc.rc) return sc.rc;
    if ((d_values || d_blindings) && !c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    if ((rc = sc.enter(stream))) return rc;
    hipStream_t s = sc.s;
    const psum_arena ar(pl, true);
    char *h_tab = nullptr;
    const size_t tab_bytes = pl.table.size() * 4;
    do {
        if ((rc = arena_reserve(c, ar.total)) || (rc = c->io.pin_alloc(tab_bytes, &h_tab))) break;
        memcpy(h_tab, pl.table.data(), tab_bytes);
        c->io.last_secret_bytes = 0;   // (the block's leading bytes now hold this call's plan table: public)
        if (hipMemcpyAsync(c->arena + ar.off_tab, h_tab, tab_bytes, hipMemcpyHostToDevice, s) != hipSuccess || c->io.pin_mark(s)) {
            rc = fail(c, BPGPU_ERR_HIP, "staging the plan table failed");
            break;
        }
        rc = psum_launch_locked(c, s, pl, ar, (const uint32_t *)(c->arena + ar.off_tab), d_points, d_signs, d_values, value_bytes, d_blindings, balance, d_out, d_status);
    } while (0);
    // what the library itself allocated for the call -- plan table, row flags, partials -- is cleared on the stream behind the finish, as the
    // other _dev forms of this family clear theirs: nothing of a call stays in the context's working set
    bool ok = true;
    if (c->arena && c->arena_cap >= ar.total) ok = hipMemsetAsync(c->arena, 0, ar.total, s) == hipSuccess;
    const int rc2 = sc.leave();
    if (!rc && !ok) rc = fail(c, BPGPU_ERR_HIP, "clearing the working set failed");
    return rc ? rc : rc2;
}
extern "C" int bpgpu_pedersen_sum_batch_dev(bpgpu_ctx *c, size_t nbatch, const uint32_t *row_offsets, const void *d_points, const void *d_signs, const void *d_values,
                                            size_t value_bytes, const void *d_blindings, void *d_out, void *d_status_out, void *stream) {
    if (c && nbatch && !d_out) return fail(c, BPGPU_ERR_INVALID_ARG, "out and status_out are required");
    return psum_dev(c, nbatch, row_offsets, d_points, d_signs, d_values, value_bytes, d_blindings, d_out, d_status_out, stream);
}
extern "C" int bpgpu_pedersen_balance_batch_dev(bpgpu_ctx *c, size_t nbatch, const uint32_t *row_offsets, const void *d_points, const void *d_signs, const void *d_values,
                                                size_t value_bytes, const void *d_blindings, void *d_verdict_out, void *stream) {
    return psum_dev(c, nbatch, row_offsets, d_points, d_signs, d_values, value_bytes, d_blindings, nullptr, d_verdict_out, stream);
}

// ============================================================================
// the multi-party aggregation protocol: parties (mpc_party.h) and dealer (mpc_dealer.h)
// ============================================================================
static bool mpc_bitsize_ok(size_t n) { return n == 8 || n == 16 || n == 32 || n == 64; }

// the id lists of every position for bitsize n: [party_capacity][2n + 2] (mpc_fill_ids), cached like gen_ids_for's lists
static int mpc_ids_for(bpgpu_ctx *c, size_t n, uint32_t **out) {
    auto key = std::make_pair(n, (size_t)1 << 41);
    auto it = c->gen_ids_cache.find(key);
    if (it != c->gen_ids_cache.end()) {
        *out = it->second;
        return BPGPU_OK;
    }
    const size_t stride = 2 * n + 2;
    std::vector<uint32_t> ids(c->party_capacity * stride);
    for (size_t j = 0; j < c->party_capacity; j++) mpc_fill_ids(ids.data() + j * stride, (uint32_t)n, (uint32_t)j, (uint32_t)c->gens_capacity, (uint32_t)c->party_capacity);
    uint32_t *d = nullptr;
    HIPCHK(c, hipMalloc((void **)&d, ids.size() * 4));
    HIPCHK(c, hipMemcpy(d, ids.data(), ids.size() * 4, hipMemcpyHostToDevice));
    c->gen_ids_cache[key] = d;
    *out = d;
    return BPGPU_OK;
}

struct mpc_plan {
    uint32_t nslots = 0;
    std::vector<uint32_t> row_slot, slot_row, blk_pos, slot_pos;
};
static void mpc_make_plan(mpc_plan &pl, size_t nrows, const uint32_t *pos, size_t npos) {
    const size_t cap = (size_t)mpc_plan_cap(nrows, npos);
    pl.row_slot.assign(nrows, 0);
    pl.slot_row.assign(cap, MPC_NO_ROW);
    pl.blk_pos.assign(cap / MPC_WAVE, 0);
    pl.nslots = mpc_plan_slots((uint32_t)nrows, pos, (uint32_t)npos, pl.row_slot.data(), pl.slot_row.data(), pl.blk_pos.data());
    pl.slot_pos.assign(pl.nslots, MPC_NO_ROW);
    for (uint32_t s = 0; s < pl.nslots; s++)
        if (pl.slot_row[s] != MPC_NO_ROW) pl.slot_pos[s] = pos[pl.slot_row[s]];
}

// kinds * nslots multiscalar multiplications over the first n_terms generator terms of each row's POSITION (k_mpc.hip): rows
// [kind][slot] of n_terms scalars -> d_out [kinds * nslots][8 words].  Context option prover_constant_time: the constant-time walk.
static int mpc_walk(bpgpu_ctx *c, hipStream_t s, size_t n, uint32_t kinds, uint32_t nslots, uint32_t n_terms, const uint32_t *d_scalars, const uint32_t *d_blk_pos,
                    const uint32_t *d_slot_pos, uint32_t *d_out) {
    const bool ct = c->prover_ct;
    if (ct) {
        const int rcc = build_ct_table(c);
        if (rcc) return rcc;
    }
    uint32_t *d_ids = nullptr;
    int rc = mpc_ids_for(c, n, &d_ids);
    if (rc) return rc;
    const fb_params prm = ct ? c->prm_ct : c->prm;
    const uint32_t nrows = kinds * nslots, npairs = n_terms * prm.nwin;
    if ((uint64_t)npairs * nrows > 0x7fffffffull) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large for this shape");
    const uint32_t nsplit = pick_splits(c, nrows, npairs);
    arena_plan ap;
    const size_t off_status = ap.add((size_t)nrows * 4), off_digits = ap.add((size_t)npairs * nrows * sizeof(fb_digit) + 16),
                 off_partial = ap.add((size_t)2 * nsplit * nrows * sizeof(ge_ext) + 16);
    rc = arena_reserve(c, ap.total);
    if (rc) return rc;
    uint32_t *d_status = (uint32_t *)(c->arena + off_status);
    fb_digit *d_digits = (fb_digit *)(c->arena + off_digits);
    ge_ext *d_partial = (ge_ext *)(c->arena + off_partial);
    HIPCHK(c, hipMemsetAsync(d_status, 0, (size_t)nrows * 4, s));
    const uint32_t nrec = n_terms * nrows, nblk_p = nrows / FB_BLOCK, stride = (uint32_t)(2 * n + 2);
    if (ct) {
        LAUNCH(c, s, "fb_recode_ct", k_fb_recode_ct, (nrec + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, nrec, prm, nrows, n_terms, d_scalars, d_digits);
        LAUNCH(c, s, "mpc_accum_ct", k_mpc_accum_ct, nblk_p * nsplit, FB_BLOCK, prm, nrows, nslots, nsplit, npairs, (const uint32_t *)d_ids, stride, d_blk_pos, d_slot_pos,
               (const fb_digit *)d_digits, (const fb_entry *)c->d_table_ct, d_partial);
    } else {
        LAUNCH(c, s, "fb_recode", k_fb_recode, (nrec + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, nrec, prm, nrows, n_terms, d_scalars, d_digits, d_status);
        LAUNCH(c, s, "mpc_accum", k_mpc_accum, nblk_p * nsplit, FB_BLOCK, prm, nrows, nslots, nsplit, npairs, (const uint32_t *)d_ids, stride, d_blk_pos, d_slot_pos,
               (const fb_digit *)d_digits, (const fb_entry *)c->d_table, d_partial);
    }
    ge_ext *d_red = nullptr;
    uint32_t nred = 0;
    enqueue_fb_reduce(c, s, nrows, nsplit, d_partial, &d_red, &nred);
    LAUNCH(c, s, "shared_finish", k_shared_finish, (nrows + 63) / 64, 64, nrows, nred, (const ge_ext *)nullptr, 0, (const ge_ext *)d_red, (const uint32_t *)d_status, d_out,
           (uint8_t *)nullptr, (uint8_t *)nullptr);
    HIPCHK(c, hipGetLastError());
    return BPGPU_OK;
}

extern "C" size_t bpgpu_mpc_state1_bytes(size_t n) { return 4 * (size_t)MPC_ST1_WORDS(n); }
extern "C" size_t bpgpu_mpc_state2_bytes(size_t n) { return 4 * (size_t)MPC_ST2_WORDS(n); }

// the state blobs that came back through the staging block are secrets too: cleared once they have been handed to the caller
static void mpc_clear_staged_state(host_call<bpgpu_ctx> &io, int r) {
    memset(io.h(r), 0, io.width(r));
    if (io.hb == io.st.pin) io.st.last_secret_bytes = io.off[r + 1];
}

// ---- step 1: Party::new + assign_position_with_rng -------------------------------------------------------------------------
// seeded (bpgpu_mpc_party_bit_commit_seeded): the draws are keystream blocks first_draw[r] ... of ChaChaRng::from_seed(rng32[r]), computed by
// the lanes that consume them; the rng region of the staging block then holds 32 + 8 bytes per slot in place of 64 (2n + 2)
static int mpc_bit_commit(bpgpu_ctx *c, size_t n, size_t nparties, const uint32_t *party_index, const uint64_t *values, const uint8_t *blindings, bool seeded,
                          const uint8_t *rng, const uint64_t *first_draw, uint8_t *bit_commitments, uint8_t *state1) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    if (nparties == 0) return BPGPU_OK;
    if (!party_index || !values || !blindings || !bit_commitments || !state1) return BPGPU_ERR_INVALID_ARG;
    if (!mpc_bitsize_ok(n)) return fail(c, BPGPU_ERR_INVALID_ARG, "InvalidBitsize: n must be 8, 16, 32 or 64 (party.rs:41-43)");
    if (seeded && first_draw)
        for (size_t r = 0; r < nparties; r++)
            if (first_draw[r] > (uint64_t)0 - (uint64_t)(2 * n + 2))
                return fail(c, BPGPU_ERR_INVALID_ARG, "first_draw of party %zu: its 2n + 2 draws would run the block counter past 2^64 - 1", r);
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    if (c->gens_capacity < n) return fail(c, BPGPU_ERR_NO_GENS, "InvalidGeneratorsLength: generators too small for n=%zu (party.rs:44-46)", n);
    for (size_t r = 0; r < nparties; r++)
        if (party_index[r] >= c->party_capacity)
            return fail(c, BPGPU_ERR_NO_GENS, "InvalidGeneratorsLength: position %u of party %zu >= party_capacity %zu (party.rs:88-90)", party_index[r], r, c->party_capacity);
    if ((uint64_t)mpc_plan_cap(nparties, c->party_capacity) * 2 * (2 * n + 2) > 0x7fffffffull / 64) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large for this shape");
    mpc_plan pl;
    mpc_make_plan(pl, nparties, party_index, c->party_capacity);
    const size_t ns = pl.nslots, per_rng = seeded ? 32 + 8 : 64 * (2 * n + 2), st_bytes = bpgpu_mpc_state1_bytes(n);
    hipStream_t s = c->stream;
    host_call<bpgpu_ctx> io(c, s);
    const int r_sp = io.in(ns * 4), r_bp = io.in(ns / MPC_WAVE * 4), r_val = io.in(ns * 8), r_bl = io.in(ns * 32), r_rng = io.in(ns * per_rng);
    const int r_st = io.out(ns * st_bytes), r_v = io.out(ns * 32), r_as = io.out(2 * ns * 32);
    io.secrets(io.in_bytes());
    int rc = io.open();
    if (rc) return io.finish(rc);
    memset(io.h(r_sp), 0, io.in_bytes());
    io.put(r_sp, pl.slot_pos.data(), ns * 4);
    io.put(r_bp, pl.blk_pos.data(), ns / MPC_WAVE * 4);
    char *h_val = io.h(r_val), *h_bl = io.h(r_bl), *h_rng = io.h(r_rng), *h_base = h_rng + ns * 32;   // seeded: seeds [ns][32], then bases [ns]
    if (!rng) {   // Scalar::random(&mut thread_rng()): OS CSPRNG (padding slots draw too; they are never read); seeded: the seeds alone
        rc = os_random(c, h_rng, seeded ? ns * 32 : ns * per_rng);
        if (rc) return io.finish(rc);
    }
    for (size_t r = 0; r < nparties; r++) {
        const size_t sl = pl.row_slot[r];
        memcpy(h_val + sl * 8, values + r, 8);
        memcpy(h_bl + sl * 32, blindings + r * 32, 32);
        if (seeded) {   // seed and base go through the same row-to-slot map as the value (first_draw == NULL: 0, the region is pre-zeroed)
            if (rng) memcpy(h_rng + sl * 32, rng + r * 32, 32);
            if (first_draw) memcpy(h_base + sl * 8, first_draw + r, 8);
        } else if (rng) {
            memcpy(h_rng + sl * per_rng, rng + r * per_rng, per_rng);
        }
    }
    const uint32_t *d_sp = (const uint32_t *)io.d(r_sp), *d_bp = (const uint32_t *)io.d(r_bp);
    const uint64_t *d_val = (const uint64_t *)io.d(r_val);
    const uint8_t *d_bl = (const uint8_t *)io.d(r_bl), *d_rng = (const uint8_t *)io.d(r_rng);
    uint32_t *d_st = (uint32_t *)io.d(r_st), *d_v = (uint32_t *)io.d(r_v), *d_as = (uint32_t *)io.d(r_as);
    if ((rc = io.upload())) return io.finish(rc);
    const size_t row_len = 2 * n + 2, w_v = align_up(ns * 2 * 32), w_as = align_up(2 * ns * row_len * 32);
    rc = rpp_reserve(c, w_v + w_as);
    if (rc) return io.finish(rc);
    uint32_t *gsV = (uint32_t *)c->rpp_buf, *gsAS = (uint32_t *)(c->rpp_buf + w_v);
    do {
        if (hipMemsetAsync(c->rpp_buf, 0, w_v + w_as, s) != hipSuccess || hipMemsetAsync(d_st, 0, io.width(r_st), s) != hipSuccess) {
            rc = fail(c, BPGPU_ERR_HIP, "memset failed");
            break;
        }
        const uint32_t ns32 = (uint32_t)ns, nbits = (uint32_t)(ns * n), n_b = (ns32 + BP_BLOCK - 1) / BP_BLOCK;
        if (seeded)
            LAUNCH(c, s, "mpc_commit1_seeded", k_mpc_commit1_seeded, n_b + (nbits + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, n_b, nbits, (uint32_t)n, ns32, d_sp, d_val, d_bl, d_rng,
                   (const uint64_t *)(d_rng + ns * 32), gsV, gsAS, d_st);
        else
            LAUNCH(c, s, "mpc_commit1", k_mpc_commit1, n_b + (nbits + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, n_b, nbits, (uint32_t)n, ns32, d_sp, d_val, d_bl, d_rng, gsV, gsAS, d_st);
        rc = mpc_walk(c, s, n, 1, ns32, 2, gsV, d_bp, d_sp, d_v);                       // V_j = v B + v_blinding B~ (party.rs:55)
        if (rc) break;
        rc = mpc_walk(c, s, n, 2, ns32, (uint32_t)row_len, gsAS, d_bp, d_sp, d_as);     // A_j, S_j over B~, G_j(n), H_j(n) (party.rs:99-124)
    } while (0);
    rc = io.finish(io.download(rc));
    if (!rc)
        for (size_t r = 0; r < nparties; r++) {
            const size_t sl = pl.row_slot[r];
            memcpy(state1 + r * st_bytes, io.h(r_st) + sl * st_bytes, st_bytes);
            memcpy(bit_commitments + r * 96, io.h(r_v) + sl * 32, 32);
            memcpy(bit_commitments + r * 96 + 32, io.h(r_as) + sl * 32, 32);
            memcpy(bit_commitments + r * 96 + 64, io.h(r_as) + (ns + sl) * 32, 32);
        }
    mpc_clear_staged_state(io, r_st);
    return rc;
}
extern "C" int bpgpu_mpc_party_bit_commit(bpgpu_ctx *c, size_t n, size_t nparties, const uint32_t *party_index, const uint64_t *values, const uint8_t *blindings,
                                          const uint8_t *rng, uint8_t *bit_commitments, uint8_t *state1) {
    return mpc_bit_commit(c, n, nparties, party_index, values, blindings, false, rng, nullptr, bit_commitments, state1);
}
extern "C" int bpgpu_mpc_party_bit_commit_seeded(bpgpu_ctx *c, size_t n, size_t nparties, const uint32_t *party_index, const uint64_t *values,
                                                 const uint8_t *blindings, const uint8_t *rng32, const uint64_t *first_draw, uint8_t *bit_commitments,
                                                 uint8_t *state1) {
    return mpc_bit_commit(c, n, nparties, party_index, values, blindings, true, rng32, first_draw, bit_commitments, state1);
}

// validates the headers of caller-held state blobs; pos (optional): the rows' positions
static int mpc_check_states(bpgpu_ctx *c, size_t n, size_t nrows, const uint8_t *state, size_t st_bytes, uint32_t magic, uint32_t *pos) {
    for (size_t r = 0; r < nrows; r++) {
        uint32_t hd[3];
        memcpy(hd, state + r * st_bytes, 12);
        if (hd[0] != magic || hd[1] != n || hd[2] >= c->party_capacity)
            return fail(c, BPGPU_ERR_INVALID_ARG, "state blob %zu is not a state of this step for n=%zu on this generator set", r, n);
        if (pos) pos[r] = hd[2];
    }
    return BPGPU_OK;
}

// ---- step 2: PartyAwaitingBitChallenge::apply_challenge_with_rng ------------------------------------------------------------
// seeded (bpgpu_mpc_party_poly_commit_seeded): as mpc_bit_commit; first_draw == NULL: 2n + 2, one ChaChaRng carried through both steps
static int mpc_poly_commit(bpgpu_ctx *c, size_t n, size_t nparties, const uint8_t *state1, const uint8_t *bit_challenges, int challenges_shared, bool seeded,
                           const uint8_t *rng, const uint64_t *first_draw, uint8_t *poly_commitments, uint8_t *state2, uint8_t *status) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    if (nparties == 0) return BPGPU_OK;
    if (!state1 || !bit_challenges || !poly_commitments || !state2 || !status) return BPGPU_ERR_INVALID_ARG;
    if (!mpc_bitsize_ok(n)) return fail(c, BPGPU_ERR_INVALID_ARG, "InvalidBitsize: n must be 8, 16, 32 or 64 (party.rs:41-43)");
    if (seeded && first_draw)
        for (size_t r = 0; r < nparties; r++)
            if (first_draw[r] > (uint64_t)0 - 2)
                return fail(c, BPGPU_ERR_INVALID_ARG, "first_draw of party %zu: its 2 draws would run the block counter past 2^64 - 1", r);
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    if (c->gens_capacity < n) return fail(c, BPGPU_ERR_NO_GENS, "InvalidGeneratorsLength: generators too small for n=%zu", n);
    const size_t st1_bytes = bpgpu_mpc_state1_bytes(n), st2_bytes = bpgpu_mpc_state2_bytes(n);
    std::vector<uint32_t> pos(nparties);
    int rc = mpc_check_states(c, n, nparties, state1, st1_bytes, MPC_MAGIC1, pos.data());
    if (rc) return rc;
    if ((uint64_t)mpc_plan_cap(nparties, c->party_capacity) * st2_bytes > 0x7fffffffull) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large for this shape");
    mpc_plan pl;
    mpc_make_plan(pl, nparties, pos.data(), c->party_capacity);
    const size_t ns = pl.nslots, nch = challenges_shared ? 1 : ns, per_rng = seeded ? 32 + 8 : 128;
    hipStream_t s = c->stream;
    host_call<bpgpu_ctx> io(c, s);
    const int r_sp = io.in(ns * 4), r_bp = io.in(ns / MPC_WAVE * 4), r_s1 = io.in(ns * st1_bytes), r_ch = io.in(nch * 64), r_rng = io.in(ns * per_rng);
    const int r_s2 = io.out(ns * st2_bytes), r_t = io.out(2 * ns * 32), r_stat = io.out(ns * 4);
    io.secrets(io.in_bytes());
    rc = io.open();
    if (rc) return io.finish(rc);
    memset(io.h(r_sp), 0, io.in_bytes());
    io.put(r_sp, pl.slot_pos.data(), ns * 4);
    io.put(r_bp, pl.blk_pos.data(), ns / MPC_WAVE * 4);
    char *h_s1 = io.h(r_s1), *h_ch = io.h(r_ch), *h_rng = io.h(r_rng), *h_base = h_rng + ns * 32;   // seeded: seeds [ns][32], then bases [ns]
    if (!rng) {
        rc = os_random(c, h_rng, seeded ? ns * 32 : ns * per_rng);
        if (rc) return io.finish(rc);
    }
    if (challenges_shared) memcpy(h_ch, bit_challenges, 64);
    const uint64_t carried = 2 * n + 2;
    for (size_t r = 0; r < nparties; r++) {
        const size_t sl = pl.row_slot[r];
        memcpy(h_s1 + sl * st1_bytes, state1 + r * st1_bytes, st1_bytes);
        if (!challenges_shared) memcpy(h_ch + sl * 64, bit_challenges + r * 64, 64);
        if (seeded) {
            if (rng) memcpy(h_rng + sl * 32, rng + r * 32, 32);
            memcpy(h_base + sl * 8, first_draw ? first_draw + r : &carried, 8);
        } else if (rng) {
            memcpy(h_rng + sl * per_rng, rng + r * per_rng, per_rng);
        }
    }
    const uint32_t *d_sp = (const uint32_t *)io.d(r_sp), *d_bp = (const uint32_t *)io.d(r_bp), *d_s1 = (const uint32_t *)io.d(r_s1);
    const uint8_t *d_ch = (const uint8_t *)io.d(r_ch), *d_rng = (const uint8_t *)io.d(r_rng);
    uint32_t *d_s2 = (uint32_t *)io.d(r_s2), *d_t = (uint32_t *)io.d(r_t), *d_stat = (uint32_t *)io.d(r_stat);
    if ((rc = io.upload())) return io.finish(rc);
    const size_t w_t = align_up(2 * ns * 2 * 32);
    rc = rpp_reserve(c, w_t);
    if (rc) return io.finish(rc);
    uint32_t *gsT = (uint32_t *)c->rpp_buf;
    do {
        if (hipMemsetAsync(gsT, 0, w_t, s) != hipSuccess || hipMemsetAsync(d_s2, 0, io.out_bytes(), s) != hipSuccess) {
            rc = fail(c, BPGPU_ERR_HIP, "memset failed");
            break;
        }
        const uint32_t ns32 = (uint32_t)ns;
        if (seeded)
            LAUNCH(c, s, "mpc_poly_seeded", k_mpc_poly_seeded, (ns32 + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, (uint32_t)n, ns32, d_sp, d_s1, d_ch, challenges_shared ? 1u : 0u,
                   d_rng, (const uint64_t *)(d_rng + ns * 32), d_s2, gsT, d_stat);
        else
            LAUNCH(c, s, "mpc_poly", k_mpc_poly, (ns32 + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, (uint32_t)n, ns32, d_sp, d_s1, d_ch, challenges_shared ? 1u : 0u, d_rng, d_s2, gsT,
                   d_stat);
        rc = mpc_walk(c, s, n, 2, ns32, 2, gsT, d_bp, d_sp, d_t);   // T_i_j = t_i B + t_i_blinding B~ (party.rs:224-227)
    } while (0);
    rc = io.finish(io.download(rc));
    if (!rc)
        for (size_t r = 0; r < nparties; r++) {
            const size_t sl = pl.row_slot[r];
            uint32_t st;
            memcpy(&st, io.h(r_stat) + sl * 4, 4);
            status[r] = (uint8_t)st;
            memcpy(state2 + r * st2_bytes, io.h(r_s2) + sl * st2_bytes, st2_bytes);
            if (st) {
                memset(poly_commitments + r * 64, 0, 64);
            } else {
                memcpy(poly_commitments + r * 64, io.h(r_t) + sl * 32, 32);
                memcpy(poly_commitments + r * 64 + 32, io.h(r_t) + (ns + sl) * 32, 32);
            }
        }
    mpc_clear_staged_state(io, r_s2);
    return rc;
}
extern "C" int bpgpu_mpc_party_poly_commit(bpgpu_ctx *c, size_t n, size_t nparties, const uint8_t *state1, const uint8_t *bit_challenges, int challenges_shared,
                                           const uint8_t *rng, uint8_t *poly_commitments, uint8_t *state2, uint8_t *status) {
    return mpc_poly_commit(c, n, nparties, state1, bit_challenges, challenges_shared, false, rng, nullptr, poly_commitments, state2, status);
}
extern "C" int bpgpu_mpc_party_poly_commit_seeded(bpgpu_ctx *c, size_t n, size_t nparties, const uint8_t *state1, const uint8_t *bit_challenges,
                                                  int challenges_shared, const uint8_t *rng32, const uint64_t *first_draw, uint8_t *poly_commitments,
                                                  uint8_t *state2, uint8_t *status) {
    return mpc_poly_commit(c, n, nparties, state1, bit_challenges, challenges_shared, true, rng32, first_draw, poly_commitments, state2, status);
}

// ---- step 3: PartyAwaitingPolyChallenge::apply_challenge -------------------------------------------------------------------
extern "C" int bpgpu_mpc_party_proof_share(bpgpu_ctx *c, size_t n, size_t nparties, const uint8_t *state2, const uint8_t *poly_challenges, int challenges_shared,
                                           uint8_t *shares, uint8_t *status) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    if (nparties == 0) return BPGPU_OK;
    if (!state2 || !poly_challenges || !shares || !status) return BPGPU_ERR_INVALID_ARG;
    if (!mpc_bitsize_ok(n)) return fail(c, BPGPU_ERR_INVALID_ARG, "InvalidBitsize: n must be 8, 16, 32 or 64 (party.rs:41-43)");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_gens) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    const size_t st2_bytes = bpgpu_mpc_state2_bytes(n), share_len = 32 * (3 + 2 * n), nch = challenges_shared ? 1 : nparties;
    int rc = mpc_check_states(c, n, nparties, state2, st2_bytes, MPC_MAGIC2, nullptr);
    if (rc) return rc;
    if ((uint64_t)nparties * st2_bytes > 0x7fffffffull) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large for this shape");
    hipStream_t s = c->stream;
    host_call<bpgpu_ctx> io(c, s);
    const int r_s2 = io.in(nparties * st2_bytes), r_x = io.in(nch * 32), r_sh = io.out(nparties * share_len), r_stat = io.out(nparties);
    io.secrets(io.in_bytes());
    rc = io.open();
    if (rc) return io.finish(rc);
    io.put(r_s2, state2, nparties * st2_bytes);
    io.put(r_x, poly_challenges, nch * 32);
    rc = io.upload();
    if (!rc) rc = HIPRC(c, hipMemsetAsync(io.d(r_sh), 0, io.out_bytes(), s));
    if (rc) return io.finish(rc);
    const uint32_t np32 = (uint32_t)nparties;
    LAUNCH(c, s, "mpc_share", k_mpc_share, (np32 + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, np32, (uint32_t)n, (const uint32_t *)io.d(r_s2), (const uint8_t *)io.d(r_x),
           challenges_shared ? 1u : 0u, (uint32_t *)io.d(r_sh), (uint8_t *)io.d(r_stat));
    if (hipGetLastError() != hipSuccess) rc = fail(c, BPGPU_ERR_HIP, "launch failed");
    rc = io.finish(io.download(rc));
    if (rc) return rc;
    memcpy(shares, io.h(r_sh), nparties * share_len);
    memcpy(status, io.h(r_stat), nparties);
    return BPGPU_OK;
}

// ---- dealer ------------------------------------------------------------------------------------------------------------------
static int mpc_dealer_shape(bpgpu_ctx *c, size_t n, size_t m, size_t *k_out) {
    if (!mpc_bitsize_ok(n)) return fail(c, BPGPU_ERR_INVALID_ARG, "InvalidBitsize: n must be 8, 16, 32 or 64 (dealer.rs:44-46)");
    if (m == 0 || (m & (m - 1))) return fail(c, BPGPU_ERR_INVALID_ARG, "InvalidAggregation: m must be a power of two (dealer.rs:47-49)");
    size_t k = 0;
    while (((size_t)1 << k) < n * m) k++;
    if (k > BP_RP_MAX_K) return fail(c, BPGPU_ERR_INVALID_ARG, "n*m > 2^%d not supported", BP_RP_MAX_K);
    if (!c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    if (c->gens_capacity < n || c->party_capacity < m)
        return fail(c, BPGPU_ERR_NO_GENS, "InvalidGeneratorsLength: generators too small for n=%zu m=%zu (dealer.rs:50-55)", n, m);
    if (k_out) *k_out = k;
    return BPGPU_OK;
}
// nsessions x ncol point sums on the device (k_mpc_ptsum): in = nsessions x m records of `rec` bytes -> out nsessions x ncol x 32, st nsessions bytes
static int mpc_point_sums(bpgpu_ctx *c, size_t m, size_t nsessions, const uint8_t *in, uint32_t rec, uint32_t off, uint32_t ncol, uint8_t *out, uint8_t *st) {
    if ((uint64_t)nsessions * m * rec > 0x7fffffffull) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large for this shape");
    hipStream_t s = c->stream;
    host_call<bpgpu_ctx> io(c, s);
    const int r_in = io.in(nsessions * m * rec), r_o = io.out(nsessions * ncol * 32), r_st = io.out(nsessions * 4);
    int rc = io.open();
    if (rc) return rc;
    io.put(r_in, in, nsessions * m * rec);
    rc = io.upload();
    if (!rc && hipMemsetAsync(io.d(r_st), 0, io.width(r_st), s) != hipSuccess) rc = fail(c, BPGPU_ERR_HIP, "memset failed");
    const uint32_t nt = (uint32_t)(nsessions * ncol);
    if (!rc) {
        LAUNCH(c, s, "mpc_ptsum", k_mpc_ptsum, (nt + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, nt, (uint32_t)m, ncol, rec, off, (const uint8_t *)io.d(r_in), (uint32_t *)io.d(r_o),
               (uint32_t *)io.d(r_st));
        if (hipGetLastError() != hipSuccess) rc = fail(c, BPGPU_ERR_HIP, "launch failed");
    }
    rc = io.finish(io.download(rc));
    if (rc) return rc;
    memcpy(out, io.h(r_o), nsessions * ncol * 32);
    for (size_t p = 0; p < nsessions; p++) {
        uint32_t v;
        memcpy(&v, io.h(r_st) + p * 4, 4);
        st[p] = (uint8_t)v;
    }
    return BPGPU_OK;
}

// ---- step 4: Dealer::new + receive_bit_commitments ---------------------------------------------------------------------------
extern "C" int bpgpu_mpc_dealer_bit_challenge(bpgpu_ctx *c, size_t n, size_t m, size_t nsessions, const uint8_t *bit_commitments, const uint8_t *label,
                                              size_t label_len, const uint8_t *transcripts, size_t transcript_stride, uint8_t *bit_challenges,
                                              uint8_t *sums_out, uint8_t *transcripts_out, uint8_t *status) {
    if (!c || (label_len && !label)) return BPGPU_ERR_INVALID_ARG;
    if (nsessions == 0) return BPGPU_OK;
    if (!bit_commitments || !bit_challenges || !transcripts_out || !status) return BPGPU_ERR_INVALID_ARG;
    if (transcripts && transcript_stride != 0 && transcript_stride != BPGPU_TRANSCRIPT_BYTES)
        return fail(c, BPGPU_ERR_INVALID_ARG, "transcript_stride neither 0 nor BPGPU_TRANSCRIPT_BYTES");
    const size_t TS = BPGPU_TRANSCRIPT_BYTES;
    if (transcripts)
        for (size_t p = 0; p < (transcript_stride ? nsessions : 1); p++)
            if (!ts_state_ok(transcripts + p * TS)) return fail(c, BPGPU_ERR_INVALID_ARG, "malformed transcript state %zu", p);
    std::vector<uint8_t> sums(nsessions * 64), st(nsessions);
    {
        std::lock_guard<std::mutex> lk(c->mu);
        HIPCHK(c, hipSetDevice(c->device));
        int rc = mpc_dealer_shape(c, n, m, nullptr);
        if (rc) return rc;
        rc = mpc_point_sums(c, m, nsessions, bit_commitments, 96, 32, 2, sums.data(), st.data());   // A = sum A_j, S = sum S_j (dealer.rs:117-118)
        if (rc) return rc;
    }
    uint8_t st_new[BPGPU_TRANSCRIPT_BYTES];
    if (!transcripts) bpgpu_transcript_new(label, label_len, st_new);
    const uint8_t rp[13] = {'r', 'a', 'n', 'g', 'e', 'p', 'r', 'o', 'o', 'f', ' ', 'v', '1'}, ln[1] = {'n'}, lm[1] = {'m'}, lV[1] = {'V'}, lA[1] = {'A'}, lS[1] = {'S'},
                  ly[1] = {'y'}, lz[1] = {'z'};
    for (size_t p = 0; p < nsessions; p++) {
        const uint8_t *st0 = transcripts ? transcripts + (transcript_stride ? p * TS : 0) : st_new;
        status[p] = st[p];
        if (st[p]) {   // an A_j or S_j that does not decode: the session fails, its transcript stays where the caller left it
            memcpy(transcripts_out + p * TS, st0, TS);
            memset(bit_challenges + p * 64, 0, 64);
            if (sums_out) memset(sums_out + p * 64, 0, 64);
            continue;
        }
        uint32_t w[50];
        strobe t;
        ts_to_strobe(t, w, st0);
        merlin_append_message(t, DOM_SEP, 7, rp, 13);             // rangeproof_domain_sep(n, m) (dealer.rs:62)
        merlin_append_u64(t, ln, 1, n);
        merlin_append_u64(t, lm, 1, m);
        for (size_t j = 0; j < m; j++) merlin_append_message(t, lV, 1, bit_commitments + (p * m + j) * 96, 32);   // as given (dealer.rs:112-114)
        merlin_append_message(t, lA, 1, sums.data() + p * 64, 32);
        merlin_append_message(t, lS, 1, sums.data() + p * 64 + 32, 32);
        sc y, z;
        rp_challenge_scalar(t, ly, 1, y);
        rp_challenge_scalar(t, lz, 1, z);
        memcpy(bit_challenges + p * 64, y.v, 32);
        memcpy(bit_challenges + p * 64 + 32, z.v, 32);
        if (sums_out) memcpy(sums_out + p * 64, sums.data() + p * 64, 64);
        ts_from_strobe(transcripts_out + p * TS, t);
    }
    return BPGPU_OK;
}

// ---- step 5: receive_poly_commitments ----------------------------------------------------------------------------------------
extern "C" int bpgpu_mpc_dealer_poly_challenge(bpgpu_ctx *c, size_t m, size_t nsessions, const uint8_t *poly_commitments, uint8_t *transcripts,
                                               uint8_t *poly_challenges, uint8_t *sums_out, uint8_t *status) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    if (nsessions == 0) return BPGPU_OK;
    if (!poly_commitments || !transcripts || !poly_challenges || !status) return BPGPU_ERR_INVALID_ARG;
    if (m == 0 || (m & (m - 1))) return fail(c, BPGPU_ERR_INVALID_ARG, "InvalidAggregation: m must be a power of two");
    const size_t TS = BPGPU_TRANSCRIPT_BYTES;
    for (size_t p = 0; p < nsessions; p++)
        if (!ts_state_ok(transcripts + p * TS)) return fail(c, BPGPU_ERR_INVALID_ARG, "malformed transcript state %zu", p);
    std::vector<uint8_t> sums(nsessions * 64), st(nsessions);
    {
        std::lock_guard<std::mutex> lk(c->mu);
        HIPCHK(c, hipSetDevice(c->device));
        const int rc = mpc_point_sums(c, m, nsessions, poly_commitments, 64, 0, 2, sums.data(), st.data());   // T_i = sum T_i_j (dealer.rs:176-177)
        if (rc) return rc;
    }
    const uint8_t lT1[3] = {'T', '_', '1'}, lT2[3] = {'T', '_', '2'}, lx[1] = {'x'};
    for (size_t p = 0; p < nsessions; p++) {
        status[p] = st[p];
        if (st[p]) {
            memset(poly_challenges + p * 32, 0, 32);
            if (sums_out) memset(sums_out + p * 64, 0, 64);
            continue;
        }
        uint32_t w[50];
        strobe t;
        ts_to_strobe(t, w, transcripts + p * TS);
        merlin_append_message(t, lT1, 3, sums.data() + p * 64, 32);
        merlin_append_message(t, lT2, 3, sums.data() + p * 64 + 32, 32);
        sc x;
        rp_challenge_scalar(t, lx, 1, x);
        memcpy(poly_challenges + p * 32, x.v, 32);
        if (sums_out) memcpy(sums_out + p * 64, sums.data() + p * 64, 64);
        ts_from_strobe(transcripts + p * TS, t);
    }
    return BPGPU_OK;
}

// ---- step 6: assemble_shares, receive_shares_with_rng / receive_trusted_shares -----------------------------------------------
// the assembling half, under the context's mutex: sums and w on the host, vectors and the inner-product argument on the device.
// skip[p] (in/out): sessions that are void (non-canonical scalars on the way in; undecodable commitments on the way out).
static int mpc_assemble_locked(bpgpu_ctx *c, size_t n, size_t m, size_t k, size_t nsessions, const uint8_t *shares, const uint8_t *bit_commitments,
                               const uint8_t *poly_commitments, const uint8_t *challenges, uint8_t *transcripts, std::vector<uint8_t> &skip, uint8_t *status,
                               uint8_t *proofs_out) {
    const size_t nm = n * m, proof_len = 32 * (9 + 2 * k), TS = BPGPU_TRANSCRIPT_BYTES, share_len = 32 * (3 + 2 * n);
    if ((uint64_t)nsessions * 2 * (2 * nm + 2) > 0x7fffffffull / 64 || (uint64_t)nsessions * m * share_len > 0x7fffffffull)
        return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large for this shape");
    std::vector<uint8_t> sums(nsessions * 128), pst(2 * nsessions);
    int rc = mpc_point_sums(c, m, nsessions, bit_commitments, 96, 32, 2, sums.data(), pst.data());
    if (rc) return rc;
    {
        std::vector<uint8_t> tsum(nsessions * 64);
        rc = mpc_point_sums(c, m, nsessions, poly_commitments, 64, 0, 2, tsum.data(), pst.data() + nsessions);
        if (rc) return rc;
        for (size_t p = nsessions; p-- > 0;) {   // -> A, S, T_1, T_2 per session
            memmove(sums.data() + p * 128, sums.data() + p * 64, 64);
            memcpy(sums.data() + p * 128 + 64, tsum.data() + p * 64, 64);
        }
    }
    hipStream_t s = c->stream;
    host_call<bpgpu_ctx> io(c, s);
    const int r_sh = io.in(nsessions * m * share_len), r_yinv = io.in(nsessions * 32), r_w = io.in(nsessions * 32), r_sk = io.in(nsessions), r_ts = io.in(nsessions * TS);
    const int r_pr = io.out(nsessions * proof_len), r_stb = io.out(nsessions);
    io.secrets(io.off[r_yinv]);   // the shares
    rc = io.open();
    if (rc) return io.finish(rc);
    memset(io.h(r_sh), 0, io.in_bytes());
    io.put(r_sh, shares, nsessions * m * share_len);
    char *h_yinv = io.h(r_yinv), *h_w = io.h(r_w), *h_sk = io.h(r_sk), *h_ts = io.h(r_ts);
    std::vector<uint8_t> fixed(nsessions * 96);   // t_x, t_x_blinding, e_blinding
    const uint8_t ltx[3] = {'t', '_', 'x'}, ltxb[12] = {'t', '_', 'x', '_', 'b', 'l', 'i', 'n', 'd', 'i', 'n', 'g'},
                  leb[10] = {'e', '_', 'b', 'l', 'i', 'n', 'd', 'i', 'n', 'g'}, lw[1] = {'w'}, lipp[6] = {'i', 'p', 'p', ' ', 'v', '1'}, ln[1] = {'n'};
    for (size_t p = 0; p < nsessions; p++) {
        sc y;
        memcpy(y.v, challenges + p * 96, 32);
        if (pst[p] || pst[nsessions + p]) {
            skip[p] = 1;
            status[p] = (uint8_t)MPC_ST_BAD_POINT;
        }
        if (!sc_is_canonical_sc(y)) {
            skip[p] = 1;
            status[p] = (uint8_t)MPC_ST_BAD_SCALAR;
        }
        h_sk[p] = (char)skip[p];
        if (skip[p]) {
            memcpy(h_ts + p * TS, transcripts + p * TS, TS);
            continue;
        }
        sc t_x, t_x_bl, e_bl, wch, yinv;
        mpc_sum_shares((uint32_t)n, (uint32_t)m, shares + p * m * share_len, t_x, t_x_bl, e_bl, nullptr);
        memcpy(fixed.data() + p * 96, t_x.v, 32);
        memcpy(fixed.data() + p * 96 + 32, t_x_bl.v, 32);
        memcpy(fixed.data() + p * 96 + 64, e_bl.v, 32);
        uint32_t w[50];
        strobe t;
        ts_to_strobe(t, w, transcripts + p * TS);
        merlin_append_words8(t, ltx, 3, t_x.v);                   // (dealer.rs:268-270)
        merlin_append_words8(t, ltxb, 12, t_x_bl.v);
        merlin_append_words8(t, leb, 10, e_bl.v);
        rp_challenge_scalar(t, lw, 1, wch);                       // Q = w B (dealer.rs:273-274)
        merlin_append_message(t, DOM_SEP, 7, lipp, 6);            // InnerProductProof::create: innerproduct_domain_sep(nm)
        merlin_append_u64(t, ln, 1, nm);
        ts_from_strobe((uint8_t *)h_ts + p * TS, t);
        sc_invert_safegcd(yinv, y);
        memcpy(h_yinv + p * 32, yinv.v, 32);
        memcpy(h_w + p * 32, wch.v, 32);
    }
    char *d = io.d(r_sh), *d_yinv = io.d(r_yinv), *d_w = io.d(r_w), *d_sk = io.d(r_sk), *d_ts = io.d(r_ts), *d_pr = io.d(r_pr), *d_stb = io.d(r_stb);
    rc = io.upload();
    if (!rc) rc = HIPRC(c, hipMemsetAsync(d_pr, 0, io.out_bytes(), s));
    if (rc) return io.finish(rc);
    const size_t w_v = align_up(nsessions * nm * 32), w_gs = align_up(2 * nsessions * (2 * nm + 2) * 32);
    rc = rpp_reserve(c, 4 * w_v + w_gs);
    if (rc) return io.finish(rc);
    uint32_t *avec = (uint32_t *)c->rpp_buf, *bvec = (uint32_t *)(c->rpp_buf + w_v), *Gf = (uint32_t *)(c->rpp_buf + 2 * w_v), *Hf = (uint32_t *)(c->rpp_buf + 3 * w_v),
             *gsc = (uint32_t *)(c->rpp_buf + 4 * w_v);
    do {
        const uint32_t nt = (uint32_t)(nsessions * nm);
        LAUNCH(c, s, "mpc_vectors", k_mpc_vectors, (nt + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, nt, (uint32_t)n, (uint32_t)m, (const uint8_t *)d, (const uint32_t *)d_yinv,
               (const uint8_t *)d_sk, avec, bvec, Gf, Hf);
        ippc_fixed fx;
        fx.gn = n;
        fx.gm = m;
        fx.w = (const uint32_t *)d_w;
        fx.gen_scalars = gsc;
        rc = ippc_core(c, s, nm, k, nsessions, avec, bvec, Gf, Hf, nullptr, nullptr, nullptr, 1, (uint32_t *)d_ts, (uint8_t *)d_pr + 224, proof_len, (uint8_t *)d_stb, &fx);
    } while (0);
    if (!rc && (io.download(0) || hipMemcpyAsync(h_ts, d_ts, nsessions * TS, hipMemcpyDeviceToHost, s) != hipSuccess))
        rc = fail(c, BPGPU_ERR_HIP, "D2H copy failed");
    rc = io.finish(rc);
    if (rc) return rc;
    const char *h_out = io.h(r_pr);
    for (size_t p = 0; p < nsessions; p++) {
        uint8_t *pr = proofs_out + p * proof_len;
        if (!skip[p] && io.h(r_stb)[p]) {   // (the inner-product rounds refused the session's vectors)
            skip[p] = 1;
            status[p] = (uint8_t)MPC_ST_BAD_SCALAR;
        }
        if (skip[p]) {
            memset(pr, 0, proof_len);
            continue;
        }
        memcpy(pr, sums.data() + p * 128, 128);
        memcpy(pr + 128, fixed.data() + p * 96, 96);
        memcpy(pr + 224, h_out + p * proof_len + 224, proof_len - 224);
        memcpy(transcripts + p * TS, h_ts + p * TS, TS);
    }
    return BPGPU_OK;
}

extern "C" int bpgpu_mpc_dealer_assemble(bpgpu_ctx *c, size_t n, size_t m, size_t nsessions, const uint8_t *shares, const uint8_t *bit_commitments,
                                         const uint8_t *poly_commitments, const uint8_t *challenges, uint8_t *transcripts, const uint8_t *initial_label,
                                         size_t initial_label_len, const uint8_t *initial_transcripts, size_t initial_stride, const uint8_t *rng64, int trusted,
                                         uint8_t *proofs_out, uint8_t *bad_shares, uint8_t *status) {
    if (!c || (initial_label_len && !initial_label)) return BPGPU_ERR_INVALID_ARG;
    if (nsessions == 0) return BPGPU_OK;
    if (!shares || !bit_commitments || !poly_commitments || !challenges || !transcripts || !proofs_out || !bad_shares || !status) return BPGPU_ERR_INVALID_ARG;
    if (initial_transcripts && initial_stride != 0 && initial_stride != BPGPU_TRANSCRIPT_BYTES)
        return fail(c, BPGPU_ERR_INVALID_ARG, "initial_stride neither 0 nor BPGPU_TRANSCRIPT_BYTES");
    const size_t TS = BPGPU_TRANSCRIPT_BYTES, share_len = 32 * (3 + 2 * n);
    for (size_t p = 0; p < nsessions; p++)
        if (!ts_state_ok(transcripts + p * TS)) return fail(c, BPGPU_ERR_INVALID_ARG, "malformed transcript state %zu", p);
    size_t k = 0;
    std::vector<uint8_t> skip(nsessions, 0);
    memset(status, 0, nsessions);
    memset(bad_shares, 0, nsessions * m);
    {
        std::lock_guard<std::mutex> lk(c->mu);
        HIPCHK(c, hipSetDevice(c->device));
        int rc = mpc_dealer_shape(c, n, m, &k);
        if (rc) return rc;
        for (size_t p = 0; p < nsessions; p++) {   // upstream the share fields are Scalars by type: a non-canonical one names its party
            sc a, b, d;
            if (!mpc_sum_shares((uint32_t)n, (uint32_t)m, shares + p * m * share_len, a, b, d, bad_shares + p * m)) {
                skip[p] = 1;
                status[p] = (uint8_t)MPC_ST_MALFORMED_SHARES;
            }
        }
        rc = mpc_assemble_locked(c, n, m, k, nsessions, shares, bit_commitments, poly_commitments, challenges, transcripts, skip, status, proofs_out);
        if (rc) return rc;
    }
    if (trusted) return BPGPU_OK;
    // receive_shares_with_rng (dealer.rs:303-335): verify every assembled proof on the transcript Dealer::new cloned; audit the shares of the
    // sessions that fail.  Both through the public entry points (each under the context's mutex).
    const size_t proof_len = 32 * (9 + 2 * k);
    std::vector<size_t> cand;
    for (size_t p = 0; p < nsessions; p++)
        if (!skip[p]) cand.push_back(p);
    std::vector<size_t> blame;
    for (size_t p = 0; p < nsessions; p++)
        if (skip[p] && status[p] == MPC_ST_MALFORMED_SHARES) blame.push_back(p);
    if (!cand.empty()) {
        const size_t nc = cand.size();
        std::vector<uint8_t> pr(nc * proof_len), cm(nc * m * 32), rg(rng64 ? nc * 64 : 0), ts(initial_transcripts && initial_stride ? nc * TS : 0), verdict(nc);
        for (size_t q = 0; q < nc; q++) {
            const size_t p = cand[q];
            memcpy(pr.data() + q * proof_len, proofs_out + p * proof_len, proof_len);
            for (size_t j = 0; j < m; j++) memcpy(cm.data() + (q * m + j) * 32, bit_commitments + (p * m + j) * 96, 32);
            if (rng64) memcpy(rg.data() + q * 64, rng64 + p * 64, 64);
            if (!ts.empty()) memcpy(ts.data() + q * TS, initial_transcripts + p * TS, TS);
        }
        int rc;
        if (!initial_transcripts)
            rc = bpgpu_rangeproof_verify_batch(c, n, m, nc, pr.data(), proof_len, cm.data(), initial_label, initial_label_len, rng64 ? rg.data() : nullptr, verdict.data(),
                                               nullptr);
        else
            rc = bpgpu_rangeproof_verify_batch_ts(c, n, m, nc, pr.data(), proof_len, cm.data(), ts.empty() ? initial_transcripts : ts.data(), ts.empty() ? 0 : TS,
                                                  rng64 ? rg.data() : nullptr, verdict.data(), nullptr, nullptr);
        if (rc) return rc;
        for (size_t q = 0; q < nc; q++)
            if (verdict[q] != BPGPU_VERDICT_OK) blame.push_back(cand[q]);
    }
    if (!blame.empty()) {
        const size_t nbl = blame.size(), nsh = nbl * m;
        std::vector<uint32_t> pi(nsh);
        std::vector<uint8_t> sh(nsh * share_len), bc(nsh * 96), pc(nsh * 64), ch(nsh * 96), verdict(nsh);
        for (size_t q = 0; q < nbl; q++) {
            const size_t p = blame[q];
            memcpy(sh.data() + q * m * share_len, shares + p * m * share_len, m * share_len);
            memcpy(bc.data() + q * m * 96, bit_commitments + p * m * 96, m * 96);
            memcpy(pc.data() + q * m * 64, poly_commitments + p * m * 64, m * 64);
            for (size_t j = 0; j < m; j++) {
                pi[q * m + j] = (uint32_t)j;
                memcpy(ch.data() + (q * m + j) * 96, challenges + p * 96, 96);
            }
        }
        const int rc = bpgpu_rangeproof_audit_shares(c, n, nsh, pi.data(), sh.data(), bc.data(), pc.data(), ch.data(), 0, verdict.data(), nullptr);
        if (rc) return rc;
        for (size_t q = 0; q < nbl; q++) {
            const size_t p = blame[q];
            status[p] = (uint8_t)MPC_ST_MALFORMED_SHARES;   // MPCError::MalformedProofShares { bad_shares }
            memset(proofs_out + p * proof_len, 0, proof_len);
            for (size_t j = 0; j < m; j++) bad_shares[p * m + j] = verdict[q * m + j] != BPGPU_VERDICT_OK ? 1 : bad_shares[p * m + j];
        }
    }
    return BPGPU_OK;
}

// ============================================================================
// R1CS constraint-system proofs (r1cs.h): the circuit is a host object; its per-variable lists are uploaded to a device on
// first use and kept there until bpgpu_r1cs_circuit_destroy
// ============================================================================
struct bpgpu_r1cs_circuit {
    uint32_t m = 0, n1 = 0, n = 0, pn = 1, k = 0, two_phase = 0, nch = 0, Q = 0;
    std::vector<uint32_t> col_ptr;   // 3n + m + 2 entries: columns L_i, R_i, O_i (3i, 3i+1, 3i+2), V_j (3n + j), ONE (3n + m)
    std::vector<r1cs_ent> ents;
    std::vector<uint32_t> lbl_off;   // nch + 1
    std::vector<uint8_t> lbl;
    size_t off_ents = 0, off_lbl_off = 0, off_lbl = 0, dev_bytes = 0;
    std::mutex mu;
    std::map<int, char *> dev;       // device ordinal -> [col_ptr][ents][lbl_off][lbl]
    // the row form of the witness check (r1cs_check.h): built at the first check, uploaded to a device at the first check there
    bool rows_built = false;
    r1c_rows rows;
    size_t off_rterms = 0, off_rlongs = 0, rows_bytes = 0;
    std::map<int, char *> dev_rows;  // device ordinal -> [units][terms][longs]
};

extern "C" int bpgpu_r1cs_circuit_create(size_t m, size_t n1, size_t n2, int two_phase, size_t n_challenges, const uint8_t *labels,
                                         const uint32_t *label_lens, size_t n_constraints, const uint32_t *row_ptr, size_t n_terms,
                                         const uint8_t *term_kind, const uint32_t *term_index, const uint32_t *term_challenge,
                                         const uint32_t *term_power, const uint8_t *term_coeff, bpgpu_r1cs_circuit **out) {
    if (!out) return BPGPU_ERR_INVALID_ARG;
    *out = nullptr;
    const size_t n = n1 + n2;
    if (m > BPGPU_R1CS_MAX_VARS || n1 > BPGPU_R1CS_MAX_VARS || n2 > BPGPU_R1CS_MAX_VARS || n > BPGPU_R1CS_MAX_VARS ||
        n_constraints > BPGPU_R1CS_MAX_CONSTRAINTS || n_terms > BPGPU_R1CS_MAX_TERMS || n_challenges > BPGPU_R1CS_MAX_CHALLENGES)
        return BPGPU_ERR_INVALID_ARG;
    if (two_phase != 0 && two_phase != 1) return BPGPU_ERR_INVALID_ARG;
    if (!two_phase && (n2 != 0 || n_challenges != 0)) return BPGPU_ERR_INVALID_ARG;   // no randomized callback: no phase 2
    if (n_challenges && (!label_lens || !labels)) return BPGPU_ERR_INVALID_ARG;
    if (!row_ptr || (n_terms && (!term_kind || !term_index || !term_challenge || !term_power || !term_coeff))) return BPGPU_ERR_INVALID_ARG;
    if (row_ptr[0] != 0 || row_ptr[n_constraints] != n_terms) return BPGPU_ERR_INVALID_ARG;
    for (size_t q = 0; q < n_constraints; q++)
        if (row_ptr[q + 1] < row_ptr[q]) return BPGPU_ERR_INVALID_ARG;
    auto *ci = new bpgpu_r1cs_circuit();
    ci->m = (uint32_t)m, ci->n1 = (uint32_t)n1, ci->n = (uint32_t)n, ci->two_phase = (uint32_t)two_phase, ci->nch = (uint32_t)n_challenges;
    ci->Q = (uint32_t)n_constraints;
    while (ci->pn < n) ci->pn <<= 1, ci->k++;   // next_power_of_two (0 -> 1)
    ci->lbl_off.push_back(0);
    for (size_t j = 0; j < n_challenges; j++) {
        if (label_lens[j] > BPGPU_R1CS_MAX_LABEL) {
            delete ci;
            return BPGPU_ERR_INVALID_ARG;
        }
        ci->lbl_off.push_back(ci->lbl_off.back() + label_lens[j]);
    }
    ci->lbl.assign(labels ? labels : (const uint8_t *)"", (labels ? labels : (const uint8_t *)"") + ci->lbl_off.back());
    for (size_t t = 0; t < n_terms; t++) {
        const uint32_t kind = term_kind[t], idx = term_index[t], ch = term_challenge[t], pw = term_power[t];
        bool ok = true;
        switch (kind) {
        case BPGPU_R1CS_L: case BPGPU_R1CS_R: case BPGPU_R1CS_O: ok = idx < n; break;
        case BPGPU_R1CS_V: ok = idx < m; break;
        case BPGPU_R1CS_ONE: ok = idx == 0; break;
        default: ok = false;
        }
        if (ch == BPGPU_R1CS_NO_CHALLENGE) ok = ok && pw == 0;
        else ok = ok && ch < n_challenges && pw >= 1 && pw <= BPGPU_R1CS_MAX_POWER;
        sc cf;
        memcpy(cf.v, term_coeff + (size_t)t * 32, 32);
        ok = ok && sc_is_canonical_sc(cf);
        if (!ok) {
            delete ci;
            return BPGPU_ERR_INVALID_ARG;
        }
    }
    r1cs_build_lists(m, n, n_constraints, row_ptr, n_terms, term_kind, term_index, term_challenge, term_power, term_coeff, ci->col_ptr, ci->ents);
    ci->off_ents = align_up(ci->col_ptr.size() * 4);
    ci->off_lbl_off = ci->off_ents + align_up(ci->ents.size() * sizeof(r1cs_ent));
    ci->off_lbl = ci->off_lbl_off + align_up(ci->lbl_off.size() * 4);
    ci->dev_bytes = ci->off_lbl + align_up(ci->lbl.size() + 1);
    *out = ci;
    return BPGPU_OK;
}

extern "C" void bpgpu_r1cs_circuit_destroy(bpgpu_r1cs_circuit *ci) {
    if (!ci) return;
    for (auto &kv : ci->dev) {
        (void)hipSetDevice(kv.first);
        (void)hipFree(kv.second);
    }
    for (auto &kv : ci->dev_rows) {
        (void)hipSetDevice(kv.first);
        (void)hipFree(kv.second);
    }
    delete ci;
}

extern "C" int bpgpu_r1cs_circuit_shape(const bpgpu_r1cs_circuit *ci, size_t *padded_n, size_t *n_unique) {
    if (!ci) return BPGPU_ERR_INVALID_ARG;
    if (padded_n) *padded_n = ci->pn;
    if (n_unique) *n_unique = 11 + ci->m + 2 * ci->k;
    return BPGPU_OK;
}

// the circuit's lists on c's device (uploaded once per device; the caller holds c->mu and has set the device)
static int r1cs_circuit_on(bpgpu_ctx *c, const bpgpu_r1cs_circuit *cci, char **d_out) {
    auto *ci = const_cast<bpgpu_r1cs_circuit *>(cci);
    std::lock_guard<std::mutex> lk(ci->mu);
    auto it = ci->dev.find(c->device);
    if (it != ci->dev.end()) {
        *d_out = it->second;
        return BPGPU_OK;
    }
    std::vector<char> img(ci->dev_bytes, 0);
    memcpy(img.data(), ci->col_ptr.data(), ci->col_ptr.size() * 4);
    if (!ci->ents.empty()) memcpy(img.data() + ci->off_ents, ci->ents.data(), ci->ents.size() * sizeof(r1cs_ent));
    memcpy(img.data() + ci->off_lbl_off, ci->lbl_off.data(), ci->lbl_off.size() * 4);
    if (!ci->lbl.empty()) memcpy(img.data() + ci->off_lbl, ci->lbl.data(), ci->lbl.size());
    char *d = nullptr;
    if (hipMalloc((void **)&d, ci->dev_bytes) != hipSuccess) return fail(c, BPGPU_ERR_HIP, "out of device memory (circuit)");
    if (hipMemcpy(d, img.data(), ci->dev_bytes, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        return fail(c, BPGPU_ERR_HIP, "circuit upload failed");
    }
    ci->dev[c->device] = d;
    *d_out = d;
    return BPGPU_OK;
}

// the circuit's row form on c's device (r1cs_check.h; the caller holds c->mu and has set the device)
static int r1cs_rows_on(bpgpu_ctx *c, const bpgpu_r1cs_circuit *cci, char **d_out) {
    auto *ci = const_cast<bpgpu_r1cs_circuit *>(cci);
    std::lock_guard<std::mutex> lk(ci->mu);
    if (!ci->rows_built) {
        r1c_build_rows(ci->m, ci->n, ci->Q, ci->col_ptr, ci->ents, ci->rows);
        ci->off_rterms = align_up(ci->rows.units.size() * sizeof(r1c_unit) + 4);
        ci->off_rlongs = ci->off_rterms + align_up(ci->rows.terms.size() * sizeof(r1p_term) + 4);
        ci->rows_bytes = ci->off_rlongs + align_up(ci->rows.longs.size() * sizeof(r1c_long) + 4);
        ci->rows_built = true;
    }
    auto it = ci->dev_rows.find(c->device);
    if (it != ci->dev_rows.end()) {
        *d_out = it->second;
        return BPGPU_OK;
    }
    std::vector<char> img(ci->rows_bytes, 0);
    if (!ci->rows.units.empty()) memcpy(img.data(), ci->rows.units.data(), ci->rows.units.size() * sizeof(r1c_unit));
    if (!ci->rows.terms.empty()) memcpy(img.data() + ci->off_rterms, ci->rows.terms.data(), ci->rows.terms.size() * sizeof(r1p_term));
    if (!ci->rows.longs.empty()) memcpy(img.data() + ci->off_rlongs, ci->rows.longs.data(), ci->rows.longs.size() * sizeof(r1c_long));
    char *d = nullptr;
    if (hipMalloc((void **)&d, ci->rows_bytes) != hipSuccess) return fail(c, BPGPU_ERR_HIP, "out of device memory (circuit rows)");
    if (hipMemcpy(d, img.data(), ci->rows_bytes, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        return fail(c, BPGPU_ERR_HIP, "circuit row upload failed");
    }
    ci->dev_rows[c->device] = d;
    *d_out = d;
    return BPGPU_OK;
}

// what launches 1-3 of a batch leave in c->ipp_buf for its mega-checks: generator rows (nbatch x (2 pn + 2)), per-proof scalars and
// points (nbatch x U), status words; then room for the MSM's status bytes and outputs
struct r1cs_staged {
    r1cs_shape sh;
    char *gen, *usc, *upt, *stat, *mst, *out;
    size_t sz_mo;   // bytes of mst + out
};

// launches 1-3 of one batch against one circuit (k_r1cs_front, k_r1cs_flatten, k_r1cs_finish): everything before the mega-check
static int r1cs_front_dev_locked(bpgpu_ctx *c, const bpgpu_r1cs_circuit *ci, size_t nbatch, const void *d_proofs, size_t proof_stride,
                                 const void *d_lens, const void *d_coms, const uint8_t *shared_ts, const void *d_ts, const void *d_rng32,
                                 void *d_ts_out, hipStream_t s, r1cs_staged &stg) {
    if (shared_ts && !ts_state_ok(shared_ts)) return fail(c, BPGPU_ERR_INVALID_ARG, "malformed transcript state");
    if (!c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    if (proof_stride > 0xffffffu || nbatch > 0x7fffffffu / 64) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large");
    char *dc = nullptr;
    int rc = r1cs_circuit_on(c, ci, &dc);
    if (rc) return rc;
    r1cs_shape sh{};
    r1cs_shape_of(sh, ci->m, ci->n1, ci->n, ci->pn, ci->k, ci->two_phase, ci->nch, ci->Q, ci->col_ptr[3 * ci->n + ci->m + 1] - ci->col_ptr[3 * ci->n + ci->m],
                  proof_stride, nbatch, c->gens_capacity);
    const uint64_t ncol = (uint64_t)sh.pn + sh.m + sh.one_chunks;
    if (ncol * nbatch > 0x7fffffffull || (uint64_t)nbatch * (2 * sh.pn + 2 + sh.U) > 0x7fffffffull / 64)
        return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large for this circuit");
    if (!d_rng32) {
        sh.seeded = 1;
        if (c->test_seed_set) memcpy(sh.seed, c->test_seed, 32);
        else if (!bp::fast_random((uint8_t *)sh.seed, 32)) return fail(c, BPGPU_ERR_HIP, "getrandom failed");
    }
    const size_t ngen = 2 * (size_t)sh.pn + 2;
    const size_t sz_f = align_up((size_t)sh.nfields * nbatch * 40), sz_g = align_up(nbatch * ngen * 32), sz_u = align_up(nbatch * sh.U * 32),
                 sz_d = align_up(((size_t)sh.pn + sh.one_chunks) * nbatch * 32), sz_st = align_up(nbatch * 4), sz_b = align_up(nbatch + 64), sz_o = align_up(nbatch * 32 + 64);
    rc = ipp_reserve(c, sz_g + 2 * sz_u + sz_st + sz_f + sz_d + sz_b + sz_o);
    if (rc) return rc;
    char *d_gen = c->ipp_buf, *d_usc = d_gen + sz_g, *d_upt = d_usc + sz_u, *d_stat = d_upt + sz_u, *d_f = d_stat + sz_st, *d_dt = d_f + sz_f,
         *d_mst = d_dt + sz_d, *d_out = d_mst + sz_b;
    HIPCHK(c, hipMemsetAsync(d_gen, 0, sz_g + 2 * sz_u + sz_st, s));   // generator rows, per-proof rows, status
    rp_strobe_init init;
    memset(&init, 0, sizeof init);
    if (shared_ts) strobe_init_from_state(init, shared_ts);
    const uint32_t nb32 = (uint32_t)nbatch;
    LAUNCH(c, s, "r1cs_front", k_r1cs_front, (nb32 + RP_BLOCK - 1) / RP_BLOCK, RP_BLOCK, sh, init, (const uint8_t *)d_proofs, (const uint32_t *)d_lens,
           (const uint8_t *)d_coms, shared_ts ? (const uint32_t *)nullptr : (const uint32_t *)d_ts, (const uint8_t *)d_rng32,
           (const uint32_t *)(dc + ci->off_lbl_off), (const uint8_t *)(dc + ci->off_lbl), (uint32_t *)d_f, (uint32_t *)d_usc, (uint32_t *)d_upt,
           (uint32_t *)d_ts_out, (uint32_t *)d_stat);
    if (!sh.gens_short) {   // (gens_short: every proof stopped in launch 1 or earlier)
        const uint32_t nt = (uint32_t)(ncol * nbatch);
        LAUNCH(c, s, "r1cs_flatten", k_r1cs_flatten, (nt + 63) / 64, 64, nt, sh, (const uint32_t *)dc, (const r1cs_ent *)(dc + ci->off_ents),
               (const uint32_t *)d_stat, (uint32_t *)d_f, (uint32_t *)d_gen, (uint32_t *)d_usc, (uint32_t *)d_dt);
        LAUNCH(c, s, "r1cs_finish", k_r1cs_finish, nb32, 64, sh, (const uint32_t *)d_stat, (const uint32_t *)d_dt, (const uint32_t *)d_f, (uint32_t *)d_gen);
    }
    stg.sh = sh;
    stg.gen = d_gen, stg.usc = d_usc, stg.upt = d_upt, stg.stat = d_stat, stg.mst = d_mst, stg.out = d_out;
    stg.sz_mo = sz_b + sz_o;
    return BPGPU_OK;
}

// the per-proof mega-checks of a staged batch and its verdicts
static int r1cs_tail_dev_locked(bpgpu_ctx *c, const r1cs_staged &stg, size_t nbatch, void *d_verdict, void *d_msm_out, hipStream_t s) {
    if (stg.sh.gens_short) {   // every proof stopped in launch 1 (or earlier): nothing to multiply
        HIPCHK(c, hipMemsetAsync(stg.mst, 0, stg.sz_mo, s));
    } else {
        const int rc = msm_shared_dev_locked(c, stg.sh.pn, 1, nbatch, stg.sh.U, stg.gen, stg.usc, stg.upt, stg.out, stg.mst, nullptr, s);
        if (rc) return rc;
    }
    const uint32_t nb32 = (uint32_t)nbatch;
    LAUNCH(c, s, "r1cs_verdict", k_ipp_verdict, (nb32 + 63) / 64, 64, nb32, (const uint32_t *)stg.stat, (const uint8_t *)stg.mst, (const uint32_t *)stg.out,
           (uint8_t *)d_verdict);
    if (d_msm_out) HIPCHK(c, hipMemcpyAsync(d_msm_out, stg.out, nbatch * 32, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipGetLastError());
    return BPGPU_OK;
}

static int r1cs_verify_dev_locked(bpgpu_ctx *c, const bpgpu_r1cs_circuit *ci, size_t nbatch, const void *d_proofs, size_t proof_stride,
                                  const void *d_lens, const void *d_coms, const uint8_t *shared_ts, const void *d_ts, const void *d_rng32,
                                  void *d_verdict, void *d_msm_out, void *d_ts_out, hipStream_t s) {
    r1cs_staged stg;
    const int rc = r1cs_front_dev_locked(c, ci, nbatch, d_proofs, proof_stride, d_lens, d_coms, shared_ts, d_ts, d_rng32, d_ts_out, s, stg);
    return rc ? rc : r1cs_tail_dev_locked(c, stg, nbatch, d_verdict, d_msm_out, s);
}

extern "C" int bpgpu_r1cs_verify_batch_ts_dev(bpgpu_ctx *c, const bpgpu_r1cs_circuit *circuit, size_t nbatch, const void *d_proofs, size_t proof_stride,
                                              const void *d_proof_lens, const void *d_commitments, const uint8_t *shared_transcript,
                                              const void *d_transcripts, const void *d_rng32, void *d_verdict, void *d_msm_out,
                                              void *d_transcripts_out, void *stream) {
    if (!c || !circuit) return BPGPU_ERR_INVALID_ARG;
    if (nbatch == 0) return BPGPU_OK;
    if (!d_proofs || !d_proof_lens || !d_verdict || (circuit->m && !d_commitments) || (!shared_transcript == !d_transcripts)) return BPGPU_ERR_INVALID_ARG;
    if (((uintptr_t)d_proof_lens | (uintptr_t)d_transcripts | (uintptr_t)d_transcripts_out) & 3)
        return fail(c, BPGPU_ERR_INVALID_ARG, "device buffers must be 4-byte aligned");
    return dev_call(c, stream, [&](hipStream_t s) {
        return r1cs_verify_dev_locked(c, circuit, nbatch, d_proofs, proof_stride, d_proof_lens, d_commitments, shared_transcript, d_transcripts, d_rng32,
                                    d_verdict, d_msm_out, d_transcripts_out, s);
    });
}

extern "C" int bpgpu_r1cs_verify_batch_ts(bpgpu_ctx *c, const bpgpu_r1cs_circuit *circuit, size_t nbatch, const uint8_t *proofs, size_t proof_stride,
                                          const uint32_t *proof_lens, const uint8_t *commitments, const uint8_t *transcripts, size_t transcript_stride,
                                          const uint8_t *rng32, uint8_t *verdict, uint8_t *msm_out, uint8_t *transcripts_out) {
    if (!c || !circuit) return BPGPU_ERR_INVALID_ARG;
    if (nbatch == 0) return BPGPU_OK;
    if (!proofs || !proof_lens || !verdict || !transcripts || (circuit->m && !commitments)) return BPGPU_ERR_INVALID_ARG;
    if (transcript_stride != 0 && transcript_stride != BPGPU_TRANSCRIPT_BYTES)
        return fail(c, BPGPU_ERR_INVALID_ARG, "transcript_stride neither 0 nor BPGPU_TRANSCRIPT_BYTES");
    const bool per_proof = transcript_stride != 0;
    for (size_t b = 0; b < (per_proof ? nbatch : 1); b++)
        if (!ts_state_ok(transcripts + b * BPGPU_TRANSCRIPT_BYTES)) return fail(c, BPGPU_ERR_INVALID_ARG, "malformed transcript state %zu", b);
    const size_t TS = BPGPU_TRANSCRIPT_BYTES, m = circuit->m;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    host_call<bpgpu_ctx> io(c, s);
    const int r_pr = io.in(nbatch * proof_stride + 64), r_l = io.in(nbatch * 4), r_c = io.in(nbatch * m * 32 + 64), r_t = io.in(per_proof ? nbatch * TS : 0),
              r_r = io.in(rng32 ? nbatch * 32 : 0);
    const int r_v = io.out(nbatch), r_o = io.out(nbatch * 32), r_to = io.out(transcripts_out ? nbatch * TS : 0);
    int rc = io.open();
    if (rc) return rc;
    io.put(r_pr, proofs, nbatch * proof_stride);
    io.put(r_l, proof_lens, nbatch * 4);
    if (m) io.put(r_c, commitments, nbatch * m * 32);
    if (per_proof) io.put(r_t, transcripts, nbatch * TS);
    if (rng32) io.put(r_r, rng32, nbatch * 32);
    rc = io.upload();
    if (!rc)
        rc = r1cs_verify_dev_locked(c, circuit, nbatch, io.d(r_pr), proof_stride, io.d(r_l), io.d(r_c), per_proof ? nullptr : transcripts, per_proof ? io.d(r_t) : nullptr,
                                    rng32 ? io.d(r_r) : nullptr, io.d(r_v), io.d(r_o), transcripts_out ? io.d(r_to) : nullptr, s);
    rc = io.finish(io.download(rc));
    if (rc) return rc;
    memcpy(verdict, io.h(r_v), nbatch);
    if (msm_out) memcpy(msm_out, io.h(r_o), nbatch * 32);
    if (transcripts_out) memcpy(transcripts_out, io.h(r_to), nbatch * TS);
    return BPGPU_OK;
}

// ---- batch-combined R1CS verification (r1cs_rlc.h; an ADDITIONAL entry point, as bpgpu_rangeproof_verify_rlc) --------------
// the buffer the combined checks share (R1CS here, linear proofs and mixed range proofs below): each lays it out with an arena_plan
static int comb_reserve(bpgpu_ctx *c, size_t need) {
    if (c->comb_cap >= need) return BPGPU_OK;
    HIPCHK(c, hipDeviceSynchronize());
    if (c->comb_buf) HIPCHK(c, hipFree(c->comb_buf));
    c->comb_buf = nullptr;
    c->comb_cap = 0;
    if (hipMalloc((void **)&c->comb_buf, need + need / 4) != hipSuccess) return fail(c, BPGPU_ERR_HIP, "out of device memory (%zu bytes of combined list)", need + need / 4);
    c->comb_cap = need + need / 4;
    return BPGPU_OK;
}

// the weights of a combined check, lane = proof of the call: from the caller's 64 bytes each, or drawn under a per-call key and the
// family's domain
static int comb_rho_locked(bpgpu_ctx *c, hipStream_t s, const char *label, uint32_t n, const void *d_weights64, uint32_t dom, char *d_rho) {
    rlc_key key;
    memset(&key, 0, sizeof key);
    if (!d_weights64 && !bp::fast_random((uint8_t *)key.w, 32)) return fail(c, BPGPU_ERR_HIP, "getrandom failed");   // (never the test seed: weights stay unpredictable)
    LAUNCH(c, s, label, k_rlc_comb_rho, (n + 63) / 64, 64, n, (const uint8_t *)d_weights64, key, dom, (uint32_t *)d_rho);
    return BPGPU_OK;
}

// How every combined check lays out the shared buffer: the combined scalars and points (`list` bytes each), the limb sums, the reduced row, the
// weights, 64 bytes of result (compress(R), its status byte at + 32).  A multi-group check add()s its own regions behind these before reserve().
struct comb_layout {
    arena_plan ap;
    size_t off[6];
    char *base = nullptr, *d_csc = nullptr, *d_cpt = nullptr, *d_acc = nullptr, *d_row = nullptr, *d_rho = nullptr, *d_res = nullptr;
    comb_layout(size_t list, size_t acc, size_t row, size_t rho) {
        const size_t bytes[6] = {list, list, acc, row, rho, 64};
        for (int i = 0; i < 6; i++) off[i] = ap.add(bytes[i]);
    }
    size_t add(size_t bytes) { return ap.add(bytes); }
    // d_batch (the one-list checks): a caller that wants no batch result has it written to the result slot
    int reserve(bpgpu_ctx *c, uint8_t **d_batch = nullptr) {
        const int rc = comb_reserve(c, ap.total);
        if (rc) return rc;
        base = c->comb_buf;
        d_csc = base + off[0], d_cpt = base + off[1], d_acc = base + off[2], d_row = base + off[3], d_rho = base + off[4], d_res = base + off[5];
        if (d_batch && !*d_batch) *d_batch = (uint8_t *)d_res;
        return BPGPU_OK;
    }
};

// The tail of a one-list combined check behind its front end: comb_begin_locked, the family's weigh launch(es), then comb_finish_locked
// (generator tables) or the family's own reduce into the head of the list, msm_batch_dev_locked over it and comb_verdict_locked.

// the verdicts (undecided where R is not the identity) from the front end's status words and the multiplication's result
static int comb_verdict_locked(bpgpu_ctx *c, hipStream_t s, const char *label, uint32_t nproofs, const front_staged &stg, uint8_t *d_verdict, uint8_t *d_batch) {
    LAUNCH(c, s, label, k_rlc_comb_verdict, (nproofs + 63) / 64, 64, nproofs, (const uint32_t *)stg.d_stat, (const uint32_t *)stg.d_out,
           (const uint8_t *)stg.d_mst, d_verdict, d_batch);
    HIPCHK(c, hipGetLastError());
    return BPGPU_OK;
}
// the weights (nrho of them) and the limb sums of `rows` rows zeroed
static int comb_begin_locked(bpgpu_ctx *c, hipStream_t s, const char *label, const comb_layout &lay, uint32_t nrho, const void *d_weights64, uint32_t dom, size_t rows) {
    const int rc = comb_rho_locked(c, s, label, nrho, d_weights64, dom, lay.d_rho);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(lay.d_acc, 0, rows * 80, s));
    return BPGPU_OK;
}
// the limb sums reduced into the generator-table row, ONE multiplication over the tables of (gn, gm) and the list's nterms terms, the verdicts
static int comb_finish_locked(bpgpu_ctx *c, hipStream_t s, const char *reduce, const char *verdict, const comb_layout &lay, const front_staged &stg, size_t rows,
                              size_t gn, size_t gm, bool g_only, size_t nterms, uint32_t nproofs, uint8_t *d_verdict, uint8_t *d_batch) {
    LAUNCH(c, s, reduce, k_rlc_comb_reduce, (uint32_t)((rows + 63) / 64), 64, (uint32_t)rows, (const unsigned long long *)lay.d_acc, (uint32_t *)lay.d_row);
    const int rc = msm_shared_dev_locked(c, gn, gm, 1, nterms, lay.d_row, lay.d_csc, lay.d_cpt, stg.d_out, stg.d_mst, nullptr, s, g_only);
    return rc ? rc : comb_verdict_locked(c, s, verdict, nproofs, stg, d_verdict, d_batch);
}

// one group's inputs on the device; its proof i is proof gp0 + i of the call
struct r1cs_rlc_group {
    const bpgpu_r1cs_circuit *ci;
    size_t nbatch, proof_stride, gp0;
    const char *d_proofs, *d_lens, *d_coms, *d_ts;   // d_ts: nbatch transcript states, or null with shared_ts (a host pointer)
    const uint8_t *shared_ts;
};

// R = sum_i rho_i MegaCheck_i over every group: per slice of a group launches 1-3 (r1cs_front_dev_locked) and the weigh launch, per
// combination of at most r1cs_rlc_max_terms unique terms the reduction and ONE shared-generator MSM over PN = max padded_n, then the sum
// of the combinations and the verdicts (undecided where R is not the identity).  d_rng32: every proof's 32 bytes (the caller's or drawn).
static int r1cs_rlc_dev_locked(bpgpu_ctx *c, const std::vector<r1cs_rlc_group> &gr, size_t total, const char *d_rng32, const void *d_weights64,
                               uint8_t *d_verdict, uint8_t *d_batch, char *d_ts_out, hipStream_t s) {
    if (!c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    const size_t TS = BPGPU_TRANSCRIPT_BYTES;
    const size_t cap = c->r1cs_rlc_max_terms ? c->r1cs_rlc_max_terms : R1_RLC_MAX_TERMS;
    uint32_t PN = 1;   // (a group whose padded_n exceeds the generators stops in launch 1 and adds no generator term)
    for (const auto &g : gr)
        if (g.ci->pn <= c->gens_capacity && g.ci->pn > PN) PN = g.ci->pn;
    // the plan: slices in call order, each inside one combination (a new combination where the next slice would pass `cap`)
    struct slice_plan {
        size_t grp, first, count, comb, u0;
    };
    std::vector<slice_plan> plan;
    std::vector<size_t> comb_terms;
    for (size_t gi = 0; gi < gr.size(); gi++) {
        const size_t U = 11 + gr[gi].ci->m + 2 * (size_t)gr[gi].ci->k;
        const size_t per = std::max<size_t>(1, std::min<size_t>(R1_RLC_SLICE, cap / U));
        for (size_t f = 0; f < gr[gi].nbatch; f += per) {
            const size_t cnt = std::min(per, gr[gi].nbatch - f);
            if (comb_terms.empty() || (comb_terms.back() && comb_terms.back() + cnt * U > cap)) comb_terms.push_back(0);
            plan.push_back({gi, f, cnt, comb_terms.size() - 1, comb_terms.back()});
            comb_terms.back() += cnt * U;
        }
    }
    size_t list_max = 1;
    for (size_t t : comb_terms) list_max = std::max(list_max, t);
    const size_t ncomb = comb_terms.size(), nrows = 2 * (size_t)PN + 2;
    comb_layout lay(list_max * 32, nrows * 80, nrows * 32, total * 32);
    const size_t off_gst = lay.add(total * 4), off_parts = lay.add(ncomb * 32), off_pst = lay.add(ncomb + 64);
    int rc = lay.reserve(c);
    if (rc) return rc;
    char *d_csc = lay.d_csc, *d_cpt = lay.d_cpt, *d_acc = lay.d_acc, *d_gen = lay.d_row, *d_rho = lay.d_rho, *d_res = lay.d_res, *d_gst = lay.base + off_gst,
         *d_parts = lay.base + off_parts, *d_pst = lay.base + off_pst;
    const uint32_t n32 = (uint32_t)total;
    rc = comb_rho_locked(c, s, "r1cs_rlc_rho", n32, d_weights64, R1_RLC_WEIGHT_DOMAIN, d_rho);
    if (rc) return rc;
    for (size_t i = 0; i < plan.size(); i++) {
        const slice_plan &sp = plan[i];
        const r1cs_rlc_group &g = gr[sp.grp];
        if (i == 0 || plan[i - 1].comb != sp.comb) HIPCHK(c, hipMemsetAsync(d_acc, 0, nrows * 80, s));
        const size_t gp0 = g.gp0 + sp.first;
        r1cs_staged stg;
        rc = r1cs_front_dev_locked(c, g.ci, sp.count, g.d_proofs + sp.first * g.proof_stride, g.proof_stride, g.d_lens + sp.first * 4,
                                   g.d_coms ? g.d_coms + sp.first * g.ci->m * 32 : nullptr, g.shared_ts, g.d_ts ? g.d_ts + sp.first * TS : nullptr,
                                   d_rng32 + gp0 * 32, d_ts_out ? d_ts_out + gp0 * TS : nullptr, s, stg);
        if (rc) return rc;
        // a slice whose padded_n exceeds the generators stopped in launch 1 and has no generator terms (its pn may exceed PN: no row of it)
        r1_rlc_slice sl;
        sl.nproofs = (uint32_t)sp.count, sl.nstride = (uint32_t)((sp.count + 63) / 64 * 64), sl.U = stg.sh.U;
        sl.ngen = stg.sh.gens_short ? 0u : 2 * stg.sh.pn + 2, sl.pn = stg.sh.pn, sl.PN = PN, sl.gp0 = (uint32_t)gp0, sl.u0 = (uint32_t)sp.u0;
        if (sl.ngen && sl.pn > PN) return fail(c, BPGPU_ERR_INVALID_ARG, "padded_n %u above the combination's %u", sl.pn, PN);   // (PN covers every such group)
        const uint64_t nt = (uint64_t)sl.nstride * (sl.U + sl.ngen);   // (a multiple of 64: whole wavefronts)
        if (nt > 0x7fffffffull) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large for this circuit");
        LAUNCH(c, s, "r1cs_rlc_weigh", k_r1cs_rlc_weigh, (uint32_t)(nt / 64), 64, sl, (const uint32_t *)stg.stat, (const uint32_t *)d_rho, (const uint32_t *)stg.gen,
               (const uint32_t *)stg.usc, (const uint32_t *)stg.upt, (uint32_t *)d_csc, (uint32_t *)d_cpt, (uint32_t *)d_gst, (unsigned long long *)d_acc);
        if (i + 1 == plan.size() || plan[i + 1].comb != sp.comb) {   // the combination is complete: its generator row, then its MSM
            LAUNCH(c, s, "r1cs_rlc_reduce", k_rlc_comb_reduce, (uint32_t)((nrows + 63) / 64), 64, (uint32_t)nrows, (const unsigned long long *)d_acc,
                   (uint32_t *)d_gen);
            rc = msm_shared_dev_locked(c, PN, 1, 1, comb_terms[sp.comb], d_gen, d_csc, d_cpt, d_parts + 32 * sp.comb, d_pst + sp.comb, nullptr, s);
            if (rc) return rc;
        }
    }
    LAUNCH(c, s, "r1cs_rlc_sum", k_r1cs_rlc_sum, 1, 64, (uint32_t)ncomb, (const uint32_t *)d_parts, (const uint8_t *)d_pst, (uint32_t *)d_res, (uint8_t *)(d_res + 32));
    LAUNCH(c, s, "r1cs_rlc_verdict", k_rlc_comb_verdict, (n32 + 63) / 64, 64, n32, (const uint32_t *)d_gst, (const uint32_t *)d_res, (const uint8_t *)(d_res + 32),
           d_verdict, d_batch);
    HIPCHK(c, hipGetLastError());
    return BPGPU_OK;
}

extern "C" int bpgpu_r1cs_verify_rlc(bpgpu_ctx *c, size_t ngroups, const bpgpu_r1cs_circuit *const *circuits, const size_t *nbatch,
                                     const uint8_t *const *proofs, const size_t *proof_stride, const uint32_t *const *proof_lens,
                                     const uint8_t *const *commitments, const uint8_t *const *transcripts, const size_t *transcript_stride,
                                     const uint8_t *rng32, const uint8_t *weights64, uint8_t *verdict, uint8_t *batch_out, uint8_t *transcripts_out) {
    if (!c || ngroups == 0 || !circuits || !nbatch || !proofs || !proof_stride || !proof_lens || !commitments || !transcripts || !transcript_stride)
        return BPGPU_ERR_INVALID_ARG;
    const size_t TS = BPGPU_TRANSCRIPT_BYTES;
    size_t total = 0;
    for (size_t g = 0; g < ngroups; g++) {
        if (!circuits[g]) return BPGPU_ERR_INVALID_ARG;
        if (nbatch[g] == 0) continue;
        if (!proofs[g] || !proof_lens[g] || !transcripts[g] || (circuits[g]->m && !commitments[g])) return BPGPU_ERR_INVALID_ARG;
        if (transcript_stride[g] != 0 && transcript_stride[g] != TS)
            return fail(c, BPGPU_ERR_INVALID_ARG, "transcript_stride of group %zu neither 0 nor BPGPU_TRANSCRIPT_BYTES", g);
        if (proof_stride[g] > 0xffffffu || nbatch[g] > 0x7fffffffu / 64) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large");
        for (size_t b = 0; b < (transcript_stride[g] ? nbatch[g] : 1); b++)
            if (!ts_state_ok(transcripts[g] + b * TS)) return fail(c, BPGPU_ERR_INVALID_ARG, "malformed transcript state %zu of group %zu", b, g);
        total += nbatch[g];
    }
    if (total == 0) {
        if (batch_out) memset(batch_out, 0, 33);
        return BPGPU_OK;
    }
    if (!verdict) return BPGPU_ERR_INVALID_ARG;
    if (total > (1u << 24)) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    // staging: per group proofs, lengths, commitments, per-proof transcripts; then every proof's rng bytes and weights; then the outputs
    std::vector<size_t> off(ngroups * 4 + 1, 0);
    size_t in = 0;
    for (size_t g = 0; g < ngroups; g++) {
        const size_t nb = nbatch[g];
        off[4 * g] = in, in += nb ? align_up(nb * proof_stride[g] + 64) : 0;
        off[4 * g + 1] = in, in += nb ? align_up(nb * 4) : 0;
        off[4 * g + 2] = in, in += nb ? align_up(nb * circuits[g]->m * 32 + 64) : 0;
        off[4 * g + 3] = in, in += (nb && transcript_stride[g]) ? align_up(nb * TS) : 0;
    }
    hipStream_t s = c->stream;
    host_call<bpgpu_ctx> io(c, s);
    const int r_g = io.in(in), r_r = io.in(total * 32), r_w = io.in(weights64 ? total * 64 : 0);   // (the groups' pieces: off[] inside r_g)
    const int r_v = io.out(total), r_b = io.out(64), r_to = io.out(transcripts_out ? total * TS : 0);
    int rc = io.open();
    if (rc) return rc;
    char *h = io.h(r_g), *d = io.d(r_g);
    std::vector<r1cs_rlc_group> gr;
    size_t gp = 0;
    for (size_t g = 0; g < ngroups; g++) {
        const size_t nb = nbatch[g], m = circuits[g]->m;
        if (nb == 0) continue;
        memcpy(h + off[4 * g], proofs[g], nb * proof_stride[g]);
        memcpy(h + off[4 * g + 1], proof_lens[g], nb * 4);
        if (m) memcpy(h + off[4 * g + 2], commitments[g], nb * m * 32);
        if (transcript_stride[g]) memcpy(h + off[4 * g + 3], transcripts[g], nb * TS);
        gr.push_back({circuits[g], nb, proof_stride[g], gp, d + off[4 * g], d + off[4 * g + 1], m ? d + off[4 * g + 2] : nullptr,
                      transcript_stride[g] ? d + off[4 * g + 3] : nullptr, transcript_stride[g] ? nullptr : transcripts[g]});
        gp += nb;
    }
    if (rng32) {
        io.put(r_r, rng32, total * 32);
    } else {   // drawn once, as the per-proof path's seeded mode draws them (R1_RNG_DOMAIN), for the combination and any fallback alike
        uint32_t seed[8];
        if (c->test_seed_set) memcpy(seed, c->test_seed, 32);
        else if (!bp::fast_random((uint8_t *)seed, 32)) return io.finish(fail(c, BPGPU_ERR_HIP, "getrandom failed"));
        for (size_t p = 0; p < total; p++) {
            uint32_t kw[16];
            chacha20_block(seed, (uint64_t)p, R1_RNG_DOMAIN, 0u, kw);
            memcpy(io.h(r_r) + 32 * p, kw, 32);   // (little-endian words: the bytes k_r1cs_front takes from them)
        }
    }
    if (weights64) io.put(r_w, weights64, total * 64);
    char *d_r = io.d(r_r), *d_v = io.d(r_v);
    rc = io.upload();
    if (!rc)
        rc = r1cs_rlc_dev_locked(c, gr, total, d_r, weights64 ? io.d(r_w) : nullptr, (uint8_t *)d_v, (uint8_t *)io.d(r_b), transcripts_out ? io.d(r_to) : nullptr, s);
    rc = io.finish(io.download(rc));
    if (rc) return rc;
    // where R is not the identity, or a point did not decode: every group again through the per-proof chain, with the same rng bytes
    // (inputs are still on the device; the transcripts it leaves are the ones already copied out)
    return io.deliver_combined(r_v, verdict, total, r_b, batch_out, r_to, transcripts_out, total * TS, [&] {
        int rcg = BPGPU_OK;
        for (const auto &g : gr)   // (in slices of R1_RLC_SLICE proofs, as above: the staging stays bounded)
            for (size_t f = 0; f < g.nbatch && !rcg; f += R1_RLC_SLICE) {
                const size_t cnt = std::min<size_t>(R1_RLC_SLICE, g.nbatch - f);
                rcg = r1cs_verify_dev_locked(c, g.ci, cnt, g.d_proofs + f * g.proof_stride, g.proof_stride, g.d_lens + f * 4,
                                             g.d_coms ? g.d_coms + f * g.ci->m * 32 : nullptr, g.shared_ts, g.d_ts ? g.d_ts + f * TS : nullptr,
                                             d_r + 32 * (g.gp0 + f), d_v + g.gp0 + f, nullptr, nullptr, s);
            }
        return rcg;
    });
}

// ---- batch-combined LinearProof verification (linear_rlc.h; an ADDITIONAL entry point, as bpgpu_r1cs_verify_rlc) ------------
// R = sum_p rho_p Check_p: the front end of the per-proof path (lin_front_dev_locked), the weights, the weigh launch, the reduction of the
// n + 2 base rows and ONE multiscalar multiplication -- the shared-generator MSM with nbatch U unique terms in generator-table mode, one
// variable-base MSM of (n + 2) + nbatch U terms with the caller's bases -- then the verdicts (undecided where R is not the identity).
// The combined list and the accumulators live in the combined checks' buffer (c->comb_buf), beside the front end's staging.
static int lin_rlc_dev_locked(bpgpu_ctx *c, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len, const uint8_t *label,
                              size_t label_len, const uint8_t *shared_ts, const void *d_C, const void *d_G, const void *d_F, const void *d_B,
                              const void *d_b, int b_shared, const void *d_weights64, uint8_t *d_verdict, uint8_t *d_batch, void *d_ts_out,
                              hipStream_t s, const ipp_ts *ts = nullptr) {
    if (nbatch > LIN_RLC_MAX_PROOFS) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large: more than 2^24 proofs in one combination");
    lin_staged stg;
    int rc = lin_front_dev_locked(c, n, nbatch, d_proofs, proof_len, label, label_len, shared_ts, d_C, d_G, d_F, d_B, d_b, b_shared, d_ts_out, s, stg, ts);
    if (rc) return rc;
    if (stg.fmt) {   // every proof is a FormatError: the empty sum
        HIPCHK(c, hipMemsetAsync(d_verdict, BPGPU_VERDICT_FORMAT_ERROR, nbatch, s));
        if (d_batch) HIPCHK(c, hipMemsetAsync(d_batch, 0, 33, s));
        return BPGPU_OK;
    }
    const lin_shape &sh = stg.sh;
    const size_t U = 2 * (size_t)sh.k + 2, nrows = (size_t)sh.n + 2, head = stg.fixed ? 0 : nrows, nterms = head + nbatch * U;
    if (nbatch * U > LIN_RLC_MAX_TERMS) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large: more than 2^24 proof-specific terms in one combination");
    comb_layout lay(nterms * 32 + 64, nrows * 80, nrows * 32 + 64, nbatch * 32);
    rc = lay.reserve(c, &d_batch);
    if (rc) return rc;
    const uint32_t nb32 = (uint32_t)nbatch;
    if (sh.shape_verdict) {   // n != 2^k: every proof already carries its code and nothing enters R
        HIPCHK(c, hipMemsetAsync(stg.d_mst, 0, stg.sz_b + stg.sz_o, s));
        return comb_verdict_locked(c, s, "lin_rlc_verdict", nb32, stg, d_verdict, d_batch);
    }
    rc = comb_rho_locked(c, s, "lin_rlc_rho", nb32, d_weights64, LIN_RLC_WEIGHT_DOMAIN, lay.d_rho);
    if (rc) return rc;
    lin_rlc_shape ws;
    ws.nproofs = nb32, ws.nstride = (uint32_t)((nbatch + 63) / 64 * 64), ws.n = sh.n, ws.k = sh.k, ws.U = (uint32_t)U, ws.fixed = stg.fixed ? 1u : 0u,
    ws.u0 = (uint32_t)head;
    const uint64_t nt = (uint64_t)ws.nstride * (U + nrows);   // (a multiple of 64: whole wavefronts)
    if (nt > 0x7fffffffull) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large for this shape");
    HIPCHK(c, hipMemsetAsync(lay.d_acc, 0, nrows * 80, s));
    LAUNCH(c, s, "lin_rlc_weigh", k_lin_rlc_weigh, (uint32_t)(nt / 64), 64, ws, (const uint32_t *)stg.d_stat, (const uint32_t *)lay.d_rho, (const uint32_t *)stg.d_gen,
           (const uint32_t *)stg.d_sc, (const uint32_t *)stg.d_pt, (uint32_t *)lay.d_csc, (uint32_t *)lay.d_cpt, (unsigned long long *)lay.d_acc);
    // the combined coefficients of (B, F, G_0..): the generator-table row, or the head of the list with the caller's encodings
    if (stg.fixed) return comb_finish_locked(c, s, "lin_rlc_reduce", "lin_rlc_verdict", lay, stg, nrows, sh.n, 1, true, nbatch * U, nb32, d_verdict, d_batch);
    LAUNCH(c, s, "lin_rlc_reduce", k_lin_rlc_reduce, (uint32_t)((nrows + 63) / 64), 64, (uint32_t)nrows, (const unsigned long long *)lay.d_acc,
           (const uint8_t *)stg.d_B, (const uint8_t *)stg.d_F, (const uint8_t *)stg.d_G, (uint32_t *)lay.d_csc, (uint32_t *)lay.d_cpt);
    const uint32_t nt1 = (uint32_t)nterms;
    rc = msm_batch_dev_locked(c, 1, &nt1, lay.d_csc, lay.d_cpt, stg.d_out, stg.d_mst, s);
    return rc ? rc : comb_verdict_locked(c, s, "lin_rlc_verdict", nb32, stg, d_verdict, d_batch);
}

extern "C" int bpgpu_linear_verify_rlc_dev(bpgpu_ctx *c, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len, const uint8_t *label,
                                           size_t label_len, const uint8_t *shared_transcript, const void *d_C, const void *d_G, const void *d_F,
                                           const void *d_B, const void *d_b, int b_shared, const void *d_weights64, void *d_verdict,
                                           void *d_batch_out, void *d_transcripts_out, void *stream) {
    if (!c || (label_len && !label)) return BPGPU_ERR_INVALID_ARG;
    if (nbatch == 0) return BPGPU_OK;
    const bool from_gens = !d_G && !d_F && !d_B;
    if (!d_proofs || !d_verdict || !d_C || (n && !d_b) || (!from_gens && (!d_F || !d_B || (n && !d_G)))) return BPGPU_ERR_INVALID_ARG;
    if (((uintptr_t)d_proofs | (uintptr_t)d_C | (uintptr_t)d_G | (uintptr_t)d_F | (uintptr_t)d_B | (uintptr_t)d_b | (uintptr_t)d_transcripts_out) & 3)
        return fail(c, BPGPU_ERR_INVALID_ARG, "device buffers must be 4-byte aligned");
    return dev_call(c, stream, [&](hipStream_t s) {
        return lin_rlc_dev_locked(c, n, nbatch, d_proofs, proof_len, label, label_len, shared_transcript, d_C, d_G, d_F, d_B, d_b, b_shared, d_weights64,
                                (uint8_t *)d_verdict, (uint8_t *)d_batch_out, d_transcripts_out, s);
    });
}

// host pointers.  ts_host (with ts_stride 0 or BPGPU_TRANSCRIPT_BYTES): the callers' own transcripts, checked by the caller, in place of label /
// shared_transcript; the per-proof fallback starts again from them
static int lin_rlc_host_call(bpgpu_ctx *c, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len, const uint8_t *label, size_t label_len,
                             const uint8_t *shared_transcript, const uint8_t *ts_host, size_t ts_stride, const uint8_t *C, const uint8_t *G,
                             const uint8_t *F, const uint8_t *B, const uint8_t *b, int b_shared, const uint8_t *weights64, uint8_t *verdict,
                             uint8_t *batch_out, uint8_t *transcripts_out) {
    if (nbatch == 0) {
        if (batch_out) memset(batch_out, 0, 33);
        return BPGPU_OK;
    }
    const bool from_gens = !G && !F && !B;
    if (!proofs || !verdict || !C || (n && !b) || (!from_gens && (!F || !B || (n && !G)))) return BPGPU_ERR_INVALID_ARG;
    if (nbatch > LIN_RLC_MAX_PROOFS) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large: more than 2^24 proofs in one combination");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nb_b = b_shared ? 1 : nbatch;
    hipStream_t s = c->stream;
    host_call<bpgpu_ctx> io(c, s);
    const int r_pr = io.in(nbatch * proof_len + 64), r_c = io.in(nbatch * 32 + 64), r_g = io.in(n * 32 + 64), r_fb = io.in(64 + 64), r_bv = io.in(nb_b * n * 32 + 64),
              r_w = io.in(weights64 ? nbatch * 64 : 0), r_ti = io.in((!ts_host ? 0 : ts_stride ? nbatch : 1) * BPGPU_TRANSCRIPT_BYTES);
    const int r_v = io.out(nbatch), r_bo = io.out(64), r_t = io.out(transcripts_out ? nbatch * BPGPU_TRANSCRIPT_BYTES : 0);
    int rc = io.open();
    if (rc) return rc;
    io.put(r_pr, proofs, nbatch * proof_len);
    io.put(r_c, C, nbatch * 32);
    if (n) {
        if (!from_gens) io.put(r_g, G, n * 32);
        io.put(r_bv, b, nb_b * n * 32);
    }
    if (!from_gens) {
        memcpy(io.h(r_fb), F, 32);
        memcpy(io.h(r_fb) + 32, B, 32);
    }
    if (weights64) io.put(r_w, weights64, nbatch * 64);
    const void *a_g = from_gens ? nullptr : io.d(r_g), *a_f = from_gens ? nullptr : io.d(r_fb), *a_b = from_gens ? nullptr : io.d(r_fb) + 32;
    ipp_ts ts;
    if (ts_host) {
        io.put(r_ti, ts_host, (ts_stride ? nbatch : 1) * BPGPU_TRANSCRIPT_BYTES);
        ts.d_in = io.d(r_ti);
        ts.stride = ts_stride ? BP_TS_WORDS : 0;
    }
    const ipp_ts *a_ts = ts_host ? &ts : nullptr;
    rc = io.upload();
    if (!rc)
        rc = lin_rlc_dev_locked(c, n, nbatch, io.d(r_pr), proof_len, label, label_len, shared_transcript, io.d(r_c), a_g, a_f, a_b, io.d(r_bv), b_shared,
                                weights64 ? io.d(r_w) : nullptr, (uint8_t *)io.d(r_v), (uint8_t *)io.d(r_bo), transcripts_out ? io.d(r_t) : nullptr, s, a_ts);
    rc = io.finish(io.download(rc));
    if (rc) return rc;
    // where R is not the identity, or a point of the combined MSM did not decode: the batch again through the per-proof path (inputs are
    // still on the device; the transcripts it leaves are the ones already copied out)
    return io.deliver_combined(r_v, verdict, nbatch, r_bo, batch_out, r_t, transcripts_out, nbatch * BPGPU_TRANSCRIPT_BYTES, [&] {
        return lin_verify_dev_locked(c, n, nbatch, io.d(r_pr), proof_len, label, label_len, shared_transcript, io.d(r_c), a_g, a_f, a_b, io.d(r_bv), b_shared,
                                     io.d(r_v), nullptr, nullptr, s, a_ts);
    });
}

extern "C" int bpgpu_linear_verify_rlc(bpgpu_ctx *c, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len, const uint8_t *label,
                                       size_t label_len, const uint8_t *shared_transcript, const uint8_t *C, const uint8_t *G, const uint8_t *F,
                                       const uint8_t *B, const uint8_t *b, int b_shared, const uint8_t *weights64, uint8_t *verdict,
                                       uint8_t *batch_out, uint8_t *transcripts_out) {
    if (!c || (label_len && !label)) return BPGPU_ERR_INVALID_ARG;
    return lin_rlc_host_call(c, n, nbatch, proofs, proof_len, label, label_len, shared_transcript, nullptr, 0, C, G, F, B, b, b_shared, weights64, verdict,
                             batch_out, transcripts_out);
}

// ---- the combined check on the callers' own transcripts ----
extern "C" int bpgpu_linear_verify_rlc_ts(bpgpu_ctx *c, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len, const uint8_t *transcripts,
                                          size_t transcript_stride, const uint8_t *C, const uint8_t *G, const uint8_t *F, const uint8_t *B,
                                          const uint8_t *b, int b_shared, const uint8_t *weights64, uint8_t *verdict, uint8_t *batch_out,
                                          uint8_t *transcripts_out) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    const int rca = ipp_ts_host_args(c, transcripts, transcript_stride, nbatch);
    if (rca) return rca;
    return lin_rlc_host_call(c, n, nbatch, proofs, proof_len, nullptr, 0, nullptr, transcripts, transcript_stride, C, G, F, B, b, b_shared, weights64, verdict,
                             batch_out, transcripts_out);
}

extern "C" int bpgpu_linear_verify_rlc_ts_dev(bpgpu_ctx *c, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len, const uint8_t *shared_transcript,
                                              const void *d_transcripts, const void *d_C, const void *d_G, const void *d_F, const void *d_B,
                                              const void *d_b, int b_shared, const void *d_weights64, void *d_verdict, void *d_batch_out,
                                              void *d_transcripts_out, void *stream) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    ipp_ts ts;
    const int rca = ipp_ts_dev_args(c, shared_transcript, d_transcripts, d_transcripts_out, ts);
    if (rca) return rca;
    if (nbatch == 0) return BPGPU_OK;
    const bool from_gens = !d_G && !d_F && !d_B;
    if (!d_proofs || !d_verdict || !d_C || (n && !d_b) || (!from_gens && (!d_F || !d_B || (n && !d_G)))) return BPGPU_ERR_INVALID_ARG;
    if (((uintptr_t)d_proofs | (uintptr_t)d_C | (uintptr_t)d_G | (uintptr_t)d_F | (uintptr_t)d_B | (uintptr_t)d_b) & 3)
        return fail(c, BPGPU_ERR_INVALID_ARG, "device buffers must be 4-byte aligned");
    return dev_call(c, stream, [&](hipStream_t s) {
        return lin_rlc_dev_locked(c, n, nbatch, d_proofs, proof_len, nullptr, 0, nullptr, d_C, d_G, d_F, d_B, d_b, b_shared, d_weights64, (uint8_t *)d_verdict,
                                (uint8_t *)d_batch_out, d_transcripts_out, s, &ts);
    });
}

// ---- batch-combined InnerProductProof verification (ipp_rlc.h; an ADDITIONAL entry point, as bpgpu_linear_verify_rlc) ---------
// generator-table mode: gens_m >= 1 divides n and the context holds G(n / gens_m, gens_m), H(n / gens_m, gens_m)
static int ipp_rlc_gens_ok(bpgpu_ctx *c, size_t n, size_t gens_m) {
    if (gens_m == 0 || n % gens_m != 0) return fail(c, BPGPU_ERR_INVALID_ARG, "gens_m=%zu does not divide n=%zu", gens_m, n);
    if (!c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    if (n / gens_m > c->gens_capacity || gens_m > c->party_capacity)
        return fail(c, BPGPU_ERR_NO_GENS, "InvalidGeneratorsLength: generators too small for n=%zu m=%zu", n / gens_m, gens_m);
    return BPGPU_OK;
}

// R = sum_p rho_p Check_p for bases shared by the batch: the front end of bpgpu_ipp_verification_scalars (k_ipp_vs_front: status, u_j^2,
// u_j^-2 and the table (u_j, u_j^-1) per proof), the weights, the unique terms, the weigh launch over the 2n rows (G_0.., H_0..), their
// reduction and ONE multiscalar multiplication -- the shared-generator MSM with nbatch U unique terms in generator-table mode
// (d_G == d_H == NULL), one variable-base MSM of 2n + nbatch U terms with the caller's bases -- then the verdicts (undecided where R is
// not the identity).  The staging lives in c->ipp_buf, the combined list and the accumulators in c->comb_buf; neither grows with
// nbatch x n.
static int ipp_rlc_dev_locked(bpgpu_ctx *c, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len, const uint8_t *label,
                              size_t label_len, const uint8_t *shared_ts, const void *d_Gf, const void *d_Hf, const void *d_P, const void *d_Q,
                              const void *d_G, const void *d_H, size_t gens_m, const void *d_weights64, uint8_t *d_verdict, uint8_t *d_batch,
                              hipStream_t s, const ipp_ts *ts = nullptr) {
    if (nbatch > IPP_RLC_MAX_PROOFS) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large: more than 2^24 proofs in one combination");
    if (!ts && shared_ts && !ts_state_ok(shared_ts)) return fail(c, BPGPU_ERR_INVALID_ARG, "malformed transcript state");
    rp_strobe_init init;
    if (ts) ipp_ts_init(init, *ts);
    const bool fixed = d_G == nullptr && d_H == nullptr;
    if (fixed) {
        const int rcg = ipp_rlc_gens_ok(c, n, gens_m);
        if (rcg) return rcg;
    }
    // InnerProductProof::from_bytes, length part (ipp.rs:374-388)
    size_t k = 0;
    bool fmt = proof_len % 32 != 0;
    if (!fmt) {
        const size_t ne = proof_len / 32;
        if (ne < 2 || (ne - 2) % 2 != 0) fmt = true;
        else {
            k = (ne - 2) / 2;
            if (k >= 32) fmt = true;
        }
    }
    if (fmt) {   // every proof is a FormatError: the empty sum
        HIPCHK(c, hipMemsetAsync(d_verdict, BPGPU_VERDICT_FORMAT_ERROR, nbatch, s));
        if (d_batch) HIPCHK(c, hipMemsetAsync(d_batch, 0, 33, s));
        if (ts && ts->d_out)
            LAUNCH(c, s, "ipp_ts_input", k_ipp_ts_input, ((uint32_t)nbatch + 63) / 64, 64, (uint32_t)nbatch, init, (const uint32_t *)ts->d_in, ts->stride, (uint32_t *)ts->d_out);
        return BPGPU_OK;
    }
    const bool shape_bad = n != ((size_t)1 << k);   // ipp.rs:203-211
    if (!shape_bad && k > BP_RP_MAX_K) return fail(c, BPGPU_ERR_INVALID_ARG, "n > 2^%d not supported", BP_RP_MAX_K);
    ipp_shape sh;
    sh.n = shape_bad ? 0u : (uint32_t)n;
    sh.k = (uint32_t)k;
    sh.N = 0;
    sh.proof_len = (uint32_t)proof_len;
    sh.nproofs = (uint32_t)nbatch;
    sh.shape_verdict = shape_bad ? BPGPU_VERDICT_VERIFICATION_ERROR : 0;
    sh.bases_shared = 1;
    const size_t U = 2 * k + 2, nrows = 2 * n + (fixed ? 2 : 0), head = fixed ? 0 : 2 * n, nterms = head + nbatch * U, kk = k ? k : 1;
    if (nbatch * U > IPP_RLC_MAX_TERMS) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large: more than 2^24 proof-specific terms in one combination");
    const uint32_t nb32 = (uint32_t)nbatch, nstride = (uint32_t)((nbatch + 63) / 64 * 64);
    // rows per weigh lane (n = 2^k: a divisor of n): a Gray-code walk where the launch stays wide enough without the lanes it folds
    const size_t wB = (uint64_t)nstride * 2 * n < IPP_RLC_BLOCK_MIN_PAIRS ? 1 : (n < IPP_RLC_BLOCK ? n : IPP_RLC_BLOCK);
    const uint64_t nt = shape_bad ? 0 : (uint64_t)nstride * (2 * n / wB);   // (a multiple of 64: whole wavefronts)
    if (nt > 0x7fffffffull) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large for this shape");
    // staging: front-end status, u_j^2, u_j^-2 (zeroed: a proof that stops writes none), the tables, rho a / rho b, MSM status / result
    const size_t sz_st = align_up(nbatch * 4), sz_u = align_up(nbatch * kk * 32), sz_tab = align_up(nbatch * kk * 80), sz_ab = align_up(nbatch * 80),
                 sz_b = align_up(64), sz_o = align_up(64);
    int rc = ipp_reserve(c, sz_st + 2 * sz_u + sz_tab + sz_ab + sz_b + sz_o);
    if (rc) return rc;
    char *d_stat = c->ipp_buf, *d_us = d_stat + sz_st, *d_ui = d_us + sz_u, *d_tab = d_ui + sz_u, *d_ab = d_tab + sz_tab, *d_mst = d_ab + sz_ab,
         *d_out = d_mst + sz_b;
    front_staged stg;   // (what the tail reads of it)
    stg.d_stat = d_stat, stg.d_mst = d_mst, stg.d_out = d_out;
    comb_layout lay(nterms * 32 + 64, nrows * 80, nrows * 32 + 64, nbatch * 32);
    rc = lay.reserve(c, &d_batch);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(d_stat, 0, sz_st + 2 * sz_u, s));
    if (ts) {
        LAUNCH(c, s, "ipp_rlc_front_ts", k_ipp_vs_front_ts, (nb32 + RP_BLOCK - 1) / RP_BLOCK, RP_BLOCK, sh, init, (const uint8_t *)d_proofs, (const uint32_t *)ts->d_in,
               ts->stride, (uint32_t *)d_us, (uint32_t *)d_ui, (uint32_t *)d_tab, (uint32_t *)ts->d_out, (uint32_t *)d_stat);
    } else {
        uint8_t st0[BPGPU_TRANSCRIPT_BYTES];
        ipp_domain_sep_state(st0, label, label_len, shared_ts, n, &init);
        LAUNCH(c, s, "ipp_rlc_front", k_ipp_vs_front, (nb32 + RP_BLOCK - 1) / RP_BLOCK, RP_BLOCK, sh, init, (const uint8_t *)d_proofs, (const uint32_t *)nullptr,
               (uint32_t *)d_us, (uint32_t *)d_ui, (uint32_t *)d_tab, (uint32_t *)nullptr, (uint32_t *)d_stat);
    }
    if (shape_bad) {   // n != 2^k: every proof already carries its code and nothing enters R
        HIPCHK(c, hipMemsetAsync(d_mst, 0, sz_b + sz_o, s));
        return comb_verdict_locked(c, s, "ipp_rlc_verdict", nb32, stg, d_verdict, d_batch);
    }
    ipp_rlc_shape ws;
    ws.nproofs = nb32, ws.nstride = nstride, ws.n = (uint32_t)n, ws.k = (uint32_t)k, ws.U = (uint32_t)U, ws.proof_len = (uint32_t)proof_len,
    ws.row0 = fixed ? 2u : 0u, ws.u0 = (uint32_t)head, ws.B = (uint32_t)wB;
    rc = comb_begin_locked(c, s, "ipp_rlc_rho", lay, nb32, d_weights64, IPP_RLC_WEIGHT_DOMAIN, nrows);
    if (rc) return rc;
    LAUNCH(c, s, "ipp_rlc_uniq", k_ipp_rlc_uniq, (nb32 + 63) / 64, 64, ws, (const uint32_t *)d_stat, (const uint32_t *)lay.d_rho, (const uint8_t *)d_proofs,
           (const uint8_t *)d_P, (const uint8_t *)d_Q, (const uint32_t *)d_us, (const uint32_t *)d_ui, (uint32_t *)d_ab, (uint32_t *)lay.d_csc, (uint32_t *)lay.d_cpt);
    LAUNCH(c, s, "ipp_rlc_weigh", k_ipp_rlc_weigh, (uint32_t)(nt / 64), 64, ws, (const uint32_t *)d_stat, (const uint32_t *)d_ab, (const uint32_t *)d_tab,
           (const uint8_t *)d_Gf, (const uint8_t *)d_Hf, (unsigned long long *)lay.d_acc);
    // the combined coefficients of (G_0.., H_0..): the generator-table row behind B_blinding = B = 0, or the head of the list with the
    // caller's encodings
    if (fixed) return comb_finish_locked(c, s, "ipp_rlc_reduce", "ipp_rlc_verdict", lay, stg, nrows, n / gens_m, gens_m, false, nbatch * U, nb32, d_verdict, d_batch);
    LAUNCH(c, s, "ipp_rlc_reduce", k_ipp_rlc_reduce, (uint32_t)((nrows + 63) / 64), 64, (uint32_t)nrows, (uint32_t)n, (const unsigned long long *)lay.d_acc,
           (const uint8_t *)d_G, (const uint8_t *)d_H, (uint32_t *)lay.d_csc, (uint32_t *)lay.d_cpt);
    const uint32_t nt1 = (uint32_t)nterms;
    rc = msm_batch_dev_locked(c, 1, &nt1, lay.d_csc, lay.d_cpt, d_out, d_mst, s);
    return rc ? rc : comb_verdict_locked(c, s, "ipp_rlc_verdict", nb32, stg, d_verdict, d_batch);
}

extern "C" int bpgpu_ipp_verify_rlc_dev(bpgpu_ctx *c, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len, const uint8_t *label,
                                        size_t label_len, const uint8_t *shared_transcript, const void *d_G_factors, const void *d_H_factors,
                                        const void *d_P, const void *d_Q, const void *d_G, const void *d_H, size_t gens_m, const void *d_weights64,
                                        void *d_verdict, void *d_batch_out, void *stream) {
    if (!c || (label_len && !label)) return BPGPU_ERR_INVALID_ARG;
    if (nbatch == 0) return BPGPU_OK;
    if (!d_proofs || !d_verdict || !d_P || !d_Q || (n && (!d_G_factors || !d_H_factors)) || (d_G == nullptr) != (d_H == nullptr)) return BPGPU_ERR_INVALID_ARG;
    if (((uintptr_t)d_proofs | (uintptr_t)d_G_factors | (uintptr_t)d_H_factors | (uintptr_t)d_P | (uintptr_t)d_Q | (uintptr_t)d_G | (uintptr_t)d_H) & 3)
        return fail(c, BPGPU_ERR_INVALID_ARG, "device buffers must be 4-byte aligned");
    return dev_call(c, stream, [&](hipStream_t s) {
        return ipp_rlc_dev_locked(c, n, nbatch, d_proofs, proof_len, label, label_len, shared_transcript, d_G_factors, d_H_factors, d_P, d_Q, d_G, d_H, gens_m,
                                d_weights64, (uint8_t *)d_verdict, (uint8_t *)d_batch_out, s);
    });
}

// host pointers.  ts_host (with ts_stride 0 or BPGPU_TRANSCRIPT_BYTES): the callers' own transcripts, checked by the caller, in place of label /
// shared_transcript, and ts_out_host (optional) what they are left as; the per-proof fallback starts again from the input states
static int ipp_rlc_host_call(bpgpu_ctx *c, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len, const uint8_t *label, size_t label_len,
                             const uint8_t *shared_transcript, const uint8_t *ts_host, size_t ts_stride, const uint8_t *G_factors,
                             const uint8_t *H_factors, const uint8_t *P, const uint8_t *Q, const uint8_t *G, const uint8_t *H, size_t gens_m,
                             const uint8_t *weights64, uint8_t *verdict, uint8_t *batch_out, uint8_t *ts_out_host) {
    if (nbatch == 0) {
        if (batch_out) memset(batch_out, 0, 33);
        return BPGPU_OK;
    }
    if (!proofs || !verdict || !P || !Q || (n && (!G_factors || !H_factors)) || (G == nullptr) != (H == nullptr)) return BPGPU_ERR_INVALID_ARG;
    if (nbatch > IPP_RLC_MAX_PROOFS) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large: more than 2^24 proofs in one combination");
    const bool from_gens = !G && !H;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (from_gens) {   // (before anything is staged: the fallback gathers 2n encodings of the context's generators)
        const int rcg = ipp_rlc_gens_ok(c, n, gens_m);
        if (rcg) return rcg;
    }
    hipStream_t s = c->stream;
    host_call<bpgpu_ctx> io(c, s);
    const size_t b_f = nbatch * n * 32 + 64, b_pq = nbatch * 32 + 64, b_g = n * 32 + 64;
    const int r_pr = io.in(nbatch * proof_len + 64), r_gf = io.in(b_f), r_hf = io.in(b_f), r_p = io.in(b_pq), r_q = io.in(b_pq),
              r_g = io.in(from_gens ? 0 : b_g), r_h = io.in(from_gens ? 0 : b_g), r_w = io.in(weights64 ? nbatch * 64 : 0),
              r_ti = io.in((!ts_host ? 0 : ts_stride ? nbatch : 1) * BPGPU_TRANSCRIPT_BYTES);
    const int r_v = io.out(nbatch), r_bo = io.out(64), r_to = io.out(ts_out_host ? nbatch * BPGPU_TRANSCRIPT_BYTES : 0);
    const int r_gen = io.dev(from_gens ? 2 * n * 32 + 64 : 0);   // the generators' encodings, for the per-proof fallback
    int rc = io.open();
    if (rc) return rc;
    io.put(r_pr, proofs, nbatch * proof_len);
    if (n) {
        io.put(r_gf, G_factors, nbatch * n * 32);
        io.put(r_hf, H_factors, nbatch * n * 32);
        if (!from_gens) {
            io.put(r_g, G, n * 32);
            io.put(r_h, H, n * 32);
        }
    }
    io.put(r_p, P, nbatch * 32);
    io.put(r_q, Q, nbatch * 32);
    if (weights64) io.put(r_w, weights64, nbatch * 64);
    const void *a_g = from_gens ? nullptr : io.d(r_g), *a_h = from_gens ? nullptr : io.d(r_h);
    ipp_ts ts;
    if (ts_host) {
        io.put(r_ti, ts_host, (ts_stride ? nbatch : 1) * BPGPU_TRANSCRIPT_BYTES);
        ts.d_in = io.d(r_ti);
        ts.stride = ts_stride ? BP_TS_WORDS : 0;
        ts.d_out = ts_out_host ? io.d(r_to) : nullptr;
    }
    rc = io.upload();
    if (!rc)
        rc = ipp_rlc_dev_locked(c, n, nbatch, io.d(r_pr), proof_len, label, label_len, shared_transcript, io.d(r_gf), io.d(r_hf), io.d(r_p), io.d(r_q), a_g, a_h,
                                gens_m, weights64 ? io.d(r_w) : nullptr, (uint8_t *)io.d(r_v), (uint8_t *)io.d(r_bo), s, ts_host ? &ts : nullptr);
    rc = io.finish(io.download(rc));
    if (rc) return rc;
    // where R is not the identity, or a point of the combined MSM did not decode: the batch again through the per-proof path with the
    // bases given once (inputs are still on the device; in generator-table mode G(n / gens_m, gens_m), H(..) are gathered first)
    return io.deliver_combined(r_v, verdict, nbatch, r_bo, batch_out, r_to, ts_out_host, nbatch * BPGPU_TRANSCRIPT_BYTES, [&]() -> int {
        ts.d_out = nullptr;   // (the fallback's transcripts are the ones already copied out)
        const void *f_g = a_g, *f_h = a_h;
        if (from_gens && n) {
            uint32_t *d_ids = nullptr;
            const int rci = gen_ids_for(c, n / gens_m, gens_m, &d_ids);
            if (rci) return rci;
            LAUNCH(c, s, "gather32", k_gather32, ((uint32_t)(2 * n) + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, (uint32_t)(2 * n), (const uint32_t *)(d_ids + 2),
                   (const uint32_t *)c->d_gens, (uint32_t *)io.d(r_gen));
            f_g = io.d(r_gen), f_h = io.d(r_gen) + n * 32;
        } else if (from_gens) {
            f_g = f_h = io.d(r_gen);
        }
        return ipp_verify_dev_locked(c, n, nbatch, io.d(r_pr), proof_len, label, label_len, shared_transcript, io.d(r_gf), io.d(r_hf), io.d(r_p), io.d(r_q),
                                     f_g, f_h, 1, io.d(r_v), nullptr, s, ts_host ? &ts : nullptr);
    });
}

extern "C" int bpgpu_ipp_verify_rlc(bpgpu_ctx *c, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len, const uint8_t *label,
                                    size_t label_len, const uint8_t *shared_transcript, const uint8_t *G_factors, const uint8_t *H_factors,
                                    const uint8_t *P, const uint8_t *Q, const uint8_t *G, const uint8_t *H, size_t gens_m, const uint8_t *weights64,
                                    uint8_t *verdict, uint8_t *batch_out) {
    if (!c || (label_len && !label)) return BPGPU_ERR_INVALID_ARG;
    return ipp_rlc_host_call(c, n, nbatch, proofs, proof_len, label, label_len, shared_transcript, nullptr, 0, G_factors, H_factors, P, Q, G, H, gens_m, weights64,
                             verdict, batch_out, nullptr);
}

// ---- the combined check on the callers' own transcripts (ipp.h: ipp_vs_front_lane<true>) ----
extern "C" int bpgpu_ipp_verify_rlc_ts(bpgpu_ctx *c, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len, const uint8_t *transcripts,
                                       size_t transcript_stride, const uint8_t *G_factors, const uint8_t *H_factors, const uint8_t *P, const uint8_t *Q,
                                       const uint8_t *G, const uint8_t *H, size_t gens_m, const uint8_t *weights64, uint8_t *verdict, uint8_t *batch_out,
                                       uint8_t *transcripts_out) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    const int rca = ipp_ts_host_args(c, transcripts, transcript_stride, nbatch);
    if (rca) return rca;
    return ipp_rlc_host_call(c, n, nbatch, proofs, proof_len, nullptr, 0, nullptr, transcripts, transcript_stride, G_factors, H_factors, P, Q, G, H, gens_m,
                             weights64, verdict, batch_out, transcripts_out);
}

extern "C" int bpgpu_ipp_verify_rlc_ts_dev(bpgpu_ctx *c, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len, const uint8_t *shared_transcript,
                                           const void *d_transcripts, const void *d_G_factors, const void *d_H_factors, const void *d_P, const void *d_Q,
                                           const void *d_G, const void *d_H, size_t gens_m, const void *d_weights64, void *d_verdict, void *d_batch_out,
                                           void *d_transcripts_out, void *stream) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    ipp_ts ts;
    const int rca = ipp_ts_dev_args(c, shared_transcript, d_transcripts, d_transcripts_out, ts);
    if (rca) return rca;
    ts.d_out = d_transcripts_out;
    if (nbatch == 0) return BPGPU_OK;
    if (!d_proofs || !d_verdict || !d_P || !d_Q || (n && (!d_G_factors || !d_H_factors)) || (d_G == nullptr) != (d_H == nullptr)) return BPGPU_ERR_INVALID_ARG;
    if (((uintptr_t)d_proofs | (uintptr_t)d_G_factors | (uintptr_t)d_H_factors | (uintptr_t)d_P | (uintptr_t)d_Q | (uintptr_t)d_G | (uintptr_t)d_H) & 3)
        return fail(c, BPGPU_ERR_INVALID_ARG, "device buffers must be 4-byte aligned");
    return dev_call(c, stream, [&](hipStream_t s) {
        return ipp_rlc_dev_locked(c, n, nbatch, d_proofs, proof_len, nullptr, 0, nullptr, d_G_factors, d_H_factors, d_P, d_Q, d_G, d_H, gens_m, d_weights64,
                                (uint8_t *)d_verdict, (uint8_t *)d_batch_out, s, &ts);
    });
}

// ============================================================================
// R1CS proof creation (r1cs_prover.h): the witness program is a host object beside the circuit, uploaded to a device on
// first use and kept there until bpgpu_r1cs_witness_destroy
// ============================================================================
struct bpgpu_r1cs_witness {
    uint32_t m = 0, n1 = 0, n = 0, nch = 0, nfree = 0, nrows = 0;
    std::vector<uint32_t> src;       // 2n entries: src_left, then src_right
    std::vector<uint32_t> row_ptr;   // nrows + 1
    std::vector<r1p_term> terms;
    size_t off_row = 0, off_terms = 0, dev_bytes = 0;
    std::mutex mu;
    std::map<int, char *> dev;       // device ordinal -> [src][row_ptr][terms]
};

extern "C" int bpgpu_r1cs_witness_create(const bpgpu_r1cs_circuit *ci, size_t n_free, const uint32_t *src_left, const uint32_t *src_right, size_t n_rows,
                                         const uint32_t *row_ptr, size_t n_terms, const uint8_t *term_kind, const uint32_t *term_index,
                                         const uint32_t *term_challenge, const uint32_t *term_power, const uint8_t *term_coeff, bpgpu_r1cs_witness **out) {
    if (!out) return BPGPU_ERR_INVALID_ARG;
    *out = nullptr;
    if (!ci) return BPGPU_ERR_INVALID_ARG;
    const size_t n = ci->n;
    if (n_free > 2 * n || n_rows > BPGPU_R1CS_MAX_CONSTRAINTS || n_terms > BPGPU_R1CS_MAX_TERMS) return BPGPU_ERR_INVALID_ARG;
    if ((n && (!src_left || !src_right)) || !row_ptr || (n_terms && (!term_kind || !term_index || !term_challenge || !term_power || !term_coeff)))
        return BPGPU_ERR_INVALID_ARG;
    if (row_ptr[0] != 0 || row_ptr[n_rows] != n_terms) return BPGPU_ERR_INVALID_ARG;
    for (size_t r = 0; r < n_rows; r++)
        if (row_ptr[r + 1] < row_ptr[r]) return BPGPU_ERR_INVALID_ARG;
    // every term as bpgpu_r1cs_circuit_create checks it
    for (size_t t = 0; t < n_terms; t++) {
        const uint32_t kind = term_kind[t], idx = term_index[t], ch = term_challenge[t], pw = term_power[t];
        bool ok = true;
        switch (kind) {
        case BPGPU_R1CS_L: case BPGPU_R1CS_R: case BPGPU_R1CS_O: ok = idx < n; break;
        case BPGPU_R1CS_V: ok = idx < ci->m; break;
        case BPGPU_R1CS_ONE: ok = idx == 0; break;
        default: ok = false;
        }
        if (ch == BPGPU_R1CS_NO_CHALLENGE) ok = ok && pw == 0;
        else ok = ok && ch < ci->nch && pw >= 1 && pw <= BPGPU_R1CS_MAX_POWER;
        sc cf;
        memcpy(cf.v, term_coeff + t * 32, 32);
        if (!ok || !sc_is_canonical_sc(cf)) return BPGPU_ERR_INVALID_ARG;
    }
    // the sources of multiplier i: a free input (each used once), a row over earlier multipliers only (no challenge in phase 1), or zero
    std::vector<uint32_t> used(n_free, 0);
    for (size_t i = 0; i < n; i++)
        for (int side = 0; side < 2; side++) {
            const uint32_t s = side ? src_right[i] : src_left[i];
            if (s == BPGPU_R1CS_SRC_ZERO) continue;
            if (s & BPGPU_R1CS_SRC_FREE) {
                const uint32_t j = s & ~BPGPU_R1CS_SRC_FREE;
                if (j >= n_free || used[j]++) return BPGPU_ERR_INVALID_ARG;
                continue;
            }
            if (s >= n_rows) return BPGPU_ERR_INVALID_ARG;
            for (uint32_t t = row_ptr[s]; t < row_ptr[s + 1]; t++) {
                if (term_kind[t] <= BPGPU_R1CS_O && term_index[t] >= i) return BPGPU_ERR_INVALID_ARG;
                if (i < ci->n1 && term_challenge[t] != BPGPU_R1CS_NO_CHALLENGE) return BPGPU_ERR_INVALID_ARG;
            }
        }
    for (size_t j = 0; j < n_free; j++)
        if (used[j] != 1) return BPGPU_ERR_INVALID_ARG;
    auto *w = new bpgpu_r1cs_witness();
    w->m = ci->m, w->n1 = ci->n1, w->n = ci->n, w->nch = ci->nch, w->nfree = (uint32_t)n_free, w->nrows = (uint32_t)n_rows;
    w->src.assign(src_left, src_left + n);
    w->src.insert(w->src.end(), src_right, src_right + n);
    w->row_ptr.assign(row_ptr, row_ptr + n_rows + 1);
    w->terms.resize(n_terms);
    for (size_t t = 0; t < n_terms; t++) {
        r1p_term &e = w->terms[t];
        e.kind = term_kind[t];
        e.index = term_index[t];
        e.chal = term_challenge[t] == BPGPU_R1CS_NO_CHALLENGE ? R1_NO_CHAL : (term_challenge[t] | (term_power[t] << 16));
        sc cf;
        sc28 cm;
        memcpy(cf.v, term_coeff + t * 32, 32);
        sc_to_mont28(cm, cf);
        memcpy(e.coeff, cm.v, 40);
    }
    w->off_row = align_up(w->src.size() * 4 + 4);
    w->off_terms = w->off_row + align_up(w->row_ptr.size() * 4);
    w->dev_bytes = w->off_terms + align_up(w->terms.size() * sizeof(r1p_term) + 4);
    *out = w;
    return BPGPU_OK;
}

extern "C" void bpgpu_r1cs_witness_destroy(bpgpu_r1cs_witness *w) {
    if (!w) return;
    for (auto &kv : w->dev) {
        (void)hipSetDevice(kv.first);
        (void)hipFree(kv.second);
    }
    delete w;
}

// the witness program on c's device (the caller holds c->mu and has set the device)
static int r1cs_witness_on(bpgpu_ctx *c, const bpgpu_r1cs_witness *cw, char **d_out) {
    auto *w = const_cast<bpgpu_r1cs_witness *>(cw);
    std::lock_guard<std::mutex> lk(w->mu);
    auto it = w->dev.find(c->device);
    if (it != w->dev.end()) {
        *d_out = it->second;
        return BPGPU_OK;
    }
    std::vector<char> img(w->dev_bytes, 0);
    if (!w->src.empty()) memcpy(img.data(), w->src.data(), w->src.size() * 4);
    memcpy(img.data() + w->off_row, w->row_ptr.data(), w->row_ptr.size() * 4);
    if (!w->terms.empty()) memcpy(img.data() + w->off_terms, w->terms.data(), w->terms.size() * sizeof(r1p_term));
    char *d = nullptr;
    if (hipMalloc((void **)&d, w->dev_bytes) != hipSuccess) return fail(c, BPGPU_ERR_HIP, "out of device memory (witness program)");
    if (hipMemcpy(d, img.data(), w->dev_bytes, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        return fail(c, BPGPU_ERR_HIP, "witness program upload failed");
    }
    w->dev[c->device] = d;
    *d_out = d;
    return BPGPU_OK;
}

// The witness check's launches over one batch (r1cs_check.h): a_L, a_R, a_O in aw, the challenges in fields and v on the device, as the
// prover's witness launches take and leave them.  first is pre-set to R1C_SATISFIED, count and map (optional) are zeroed; partial holds
// rows.nslots x per x 32 bytes.  The batch goes in slices of `per` proofs (r1c_slice).
static void r1cs_check_launch_locked(bpgpu_ctx *c, const bpgpu_r1cs_circuit *ci, const char *drows, const r1p_shape &sh, size_t nbatch, size_t per,
                                     const uint8_t *d_v, const uint32_t *aw, const uint32_t *fields, const uint32_t *d_stat, uint32_t mapw, uint32_t *partial,
                                     uint32_t *d_first, uint32_t *d_count, uint32_t *d_map, hipStream_t s) {
    const r1c_rows &rw = ci->rows;
    const r1c_unit *units = (const r1c_unit *)drows;
    const r1p_term *rterms = (const r1p_term *)(drows + ci->off_rterms);
    const r1c_long *longs = (const r1c_long *)(drows + ci->off_rlongs);
    if (rw.units.empty()) return;
    for (size_t p0 = 0; p0 < nbatch; p0 += per) {
        const uint32_t cnt = (uint32_t)std::min(per, nbatch - p0), nt = (uint32_t)(rw.units.size() * cnt);
        LAUNCH(c, s, "r1c_units", k_r1c_units, (nt + 63) / 64, 64, nt, sh, (uint32_t)p0, cnt, units, rterms, aw, d_v, fields, d_stat, mapw, partial, d_first,
               d_count, d_map);
        if (!rw.longs.empty()) {   // (circuits with rows of more than R1C_CHUNK terms only)
            const uint32_t nl = (uint32_t)(rw.longs.size() * cnt);
            LAUNCH(c, s, "r1c_long", k_r1c_long, (nl + 63) / 64, 64, nl, (uint32_t)p0, cnt, longs, (const uint32_t *)partial, d_stat, mapw, d_first, d_count,
                   d_map);
        }
    }
}

// bpgpu_r1cs_prove_batch and bpgpu_r1cs_prove_batch_checked: one launch chain, the check (on the proof's own phase-2 challenges, between
// the last witness launch and r1p_poly) on or off
static int r1cs_prove_impl(bpgpu_ctx *c, const bpgpu_r1cs_circuit *ci, const bpgpu_r1cs_witness *wi, size_t nbatch, const uint8_t *v,
                           const uint8_t *v_blinding, const uint8_t *free_inputs, const uint8_t *transcripts, size_t transcript_stride,
                           const uint8_t *rng32, uint8_t *proofs_out, size_t proof_stride, uint32_t *proof_lens_out, uint8_t *commitments_out,
                           uint8_t *status_out, uint8_t *transcripts_out, bool check, uint32_t *unsat_first_out) {
    if (!c || !ci || !wi || (check && !unsat_first_out)) return BPGPU_ERR_INVALID_ARG;
    if (wi->m != ci->m || wi->n1 != ci->n1 || wi->n != ci->n || wi->nch != ci->nch) return fail(c, BPGPU_ERR_INVALID_ARG, "witness program of another circuit");
    if (nbatch == 0) return BPGPU_OK;
    const size_t TS = BPGPU_TRANSCRIPT_BYTES, m = ci->m, n = ci->n, n1 = ci->n1, n2 = n - n1, pn = ci->pn, k = ci->k, nf = wi->nfree;
    if ((m && (!v || !v_blinding || !commitments_out)) || (nf && !free_inputs) || !transcripts || !proofs_out || !proof_lens_out || !status_out)
        return BPGPU_ERR_INVALID_ARG;
    if (transcript_stride != 0 && transcript_stride != TS) return fail(c, BPGPU_ERR_INVALID_ARG, "transcript_stride must be 0 or %zu", TS);
    for (size_t p = 0; p < (transcript_stride ? nbatch : 1); p++)
        if (!ts_state_ok(transcripts + p * transcript_stride)) return fail(c, BPGPU_ERR_INVALID_ARG, "malformed transcript state");
    const size_t ipp_len = 32 * (2 * k + 2), max_len = 1 + 32 * (n2 ? 14 : 11) + ipp_len;
    if (proof_stride < max_len) return fail(c, BPGPU_ERR_INVALID_ARG, "proof_stride %zu < %zu", proof_stride, max_len);
    const size_t ncol = 2 * pn + 2, nrow = std::max(std::max(n, m), (size_t)1);
    const size_t n_gsc = std::max(std::max(3 * nbatch * ncol, 3 * nbatch * m), 15 * nbatch);
    if ((uint64_t)n_gsc * 32 > (4ull << 30) || (uint64_t)n_gsc > 0x7fffffffull / 8 || (uint64_t)nbatch * (n + m + nf + pn) > 0x7fffffffull / 64 ||
        (uint64_t)nbatch * 7 * nrow > 0x7fffffffull / 64)
        return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large for this circuit");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    if (pn > c->gens_capacity) return fail(c, BPGPU_ERR_NO_GENS, "InvalidGeneratorsLength: padded_n=%zu > gens_capacity=%zu", pn, (size_t)c->gens_capacity);
    r1p_shape sh{};
    sh.c.m = (uint32_t)m, sh.c.n1 = (uint32_t)n1, sh.c.n = (uint32_t)n, sh.c.pn = (uint32_t)pn, sh.c.k = (uint32_t)k;
    sh.c.two_phase = ci->two_phase, sh.c.nch = ci->nch, sh.c.Q = ci->Q;
    sh.c.nzhi = (ci->Q >> 6) + 1;
    sh.c.nyhi = (uint32_t)(((pn - 1) >> 6) + 1);
    sh.c.f_zlo = R1P_FIXED;
    sh.c.f_zhi = sh.c.f_zlo + 64;
    sh.c.f_ylo = sh.c.f_zhi + sh.c.nzhi;
    sh.c.f_yhi = sh.c.f_ylo + 64;
    sh.f_yplo = sh.c.f_yhi + sh.c.nyhi;
    sh.f_yphi = sh.f_yplo + 64;
    sh.c.f_ch = sh.f_yphi + sh.c.nyhi;
    sh.c.nfields = sh.c.f_ch + sh.c.nch;
    sh.c.nproofs = (uint32_t)nbatch;
    sh.nfree = (uint32_t)nf;
    // the draw order of prove (prover.rs:416-418, 528-541, 583)
    sh.o_sl1 = 3;
    sh.o_sr1 = sh.o_sl1 + (uint32_t)n1;
    sh.o_b2 = sh.o_sr1 + (uint32_t)n1;
    sh.o_sl2 = sh.o_b2 + (n2 ? 3u : 0u);
    sh.o_sr2 = sh.o_sl2 + (uint32_t)n2;
    sh.o_tb = sh.o_sr2 + (uint32_t)n2;
    sh.nrand = sh.o_tb + 5;
    char *dc = nullptr, *dw = nullptr;
    int rc = r1cs_circuit_on(c, ci, &dc);
    if (rc) return rc;
    rc = r1cs_witness_on(c, wi, &dw);
    if (rc) return rc;
    char *drows = nullptr;
    size_t chk_per = 0;
    if (check) {
        rc = r1cs_rows_on(c, ci, &drows);
        if (rc) return rc;
        chk_per = r1c_slice(ci->rows, nbatch);
    }
    hipStream_t s = c->stream;
    // ---- inputs through pinned staging into the persistent IO buffer
    host_call<bpgpu_ctx> io(c, s);
    const int r_v = io.in(nbatch * m * 32 + 64), r_vb = io.in(nbatch * m * 32 + 64), r_free = io.in(nbatch * nf * 32 + 64), r_rng = io.in(nbatch * 32), r_ts = io.in(nbatch * TS);
    const int r_rec = io.out(nbatch * R1P_NREC * 32), r_ipp = io.out(nbatch * ipp_len), r_vout = io.out(nbatch * m * 32 + 64), r_stat = io.out(nbatch * 4),
              r_stb = io.out(nbatch + 64), r_to = io.out(nbatch * TS), r_first = io.out(check ? nbatch * 4 : 0);
    io.secrets(io.off[r_ts]);   // values, blindings, free inputs, the rng seeds
    rc = io.open();
    if (rc) return io.finish(rc);
    if (m) {
        io.put(r_v, v, nbatch * m * 32);
        io.put(r_vb, v_blinding, nbatch * m * 32);
    }
    if (nf) io.put(r_free, free_inputs, nbatch * nf * 32);
    if (rng32) io.put(r_rng, rng32, nbatch * 32);
    else if ((rc = os_random(c, io.h(r_rng), nbatch * 32)) != 0) return io.finish(rc);   // finalize(&mut thread_rng())
    for (size_t p = 0; p < nbatch; p++) memcpy(io.h(r_ts) + p * TS, transcripts + p * transcript_stride, TS);
    const uint8_t *d_v = (const uint8_t *)io.d(r_v), *d_vb = (const uint8_t *)io.d(r_vb), *d_free = (const uint8_t *)io.d(r_free), *d_rng = (const uint8_t *)io.d(r_rng);
    uint32_t *d_ts = (uint32_t *)io.d(r_ts);
    uint32_t *d_rec = (uint32_t *)io.d(r_rec), *d_vout = (uint32_t *)io.d(r_vout), *d_stat = (uint32_t *)io.d(r_stat);
    uint8_t *d_ipp = (uint8_t *)io.d(r_ipp), *d_stb = (uint8_t *)io.d(r_stb);
    rc = io.upload();
    if (!rc) rc = HIPRC(c, hipMemsetAsync(io.d(r_rec), 0, io.out_bytes(), s));
    if (!rc && check) rc = HIPRC(c, hipMemsetAsync(io.d(r_first), 0xff, nbatch * 4, s));   // R1C_SATISFIED
    if (rc) return io.finish(rc);
    // ---- working set
    const size_t w_gs = align_up(n_gsc * 32), w_mo = align_up(5 * nbatch * 32 + 64), w_ms = align_up(std::max(nbatch * m, 5 * nbatch) + 64),
                 w_rnd = align_up((size_t)sh.nrand * nbatch * 40), w_aw = align_up(3 * std::max(n, (size_t)1) * nbatch * 40),
                 w_f = align_up((size_t)sh.c.nfields * nbatch * 40), w_vec = align_up(6 * std::max(n, (size_t)1) * nbatch * 40),
                 w_t = align_up(7 * nrow * nbatch * 40), w_iv = align_up(nbatch * pn * 32), w_w = align_up(nbatch * 32),
                 w_part = check ? align_up((size_t)ci->rows.nslots * chk_per * 32) : 0;
    const size_t need = w_gs + w_mo + w_ms + w_rnd + w_aw + w_f + w_vec + w_t + 4 * w_iv + w_w + w_part;
    if ((rc = rpp_reserve(c, need))) return io.finish(rc);
    char *wb = c->rpp_buf;
    uint32_t *gsc = (uint32_t *)wb, *mo = (uint32_t *)(wb + w_gs);
    uint8_t *mst = (uint8_t *)mo + w_mo;
    uint32_t *rnd = (uint32_t *)(mst + w_ms), *aw = (uint32_t *)((char *)rnd + w_rnd), *fields = (uint32_t *)((char *)aw + w_aw),
             *vecs = (uint32_t *)((char *)fields + w_f), *terms = (uint32_t *)((char *)vecs + w_vec), *lv = (uint32_t *)((char *)terms + w_t),
             *rv = (uint32_t *)((char *)lv + w_iv), *gf = (uint32_t *)((char *)rv + w_iv), *hf = (uint32_t *)((char *)gf + w_iv),
             *wv = (uint32_t *)((char *)hf + w_iv), *part = (uint32_t *)((char *)wv + w_w);
    const uint32_t nb32 = (uint32_t)nbatch, n_pb = (nb32 + 63) / 64;
    const uint32_t *src_l = (const uint32_t *)dw, *src_r = src_l + n, *row_ptr = (const uint32_t *)(dw + wi->off_row);
    const r1p_term *wterms = (const r1p_term *)(dw + wi->off_terms);
    const bool ct = c->prover_ct;
    do {
        // (1) V_j = v_j B + v~_j B~: rows (B~, B, G_0) of the generator walk, m per proof
        if (hipMemsetAsync(gsc, 0, std::max(nbatch * m, (size_t)1) * 3 * 32, s) != hipSuccess) { rc = fail(c, BPGPU_ERR_HIP, "memset failed"); break; }
        const uint32_t nin = (uint32_t)(nbatch * (m + nf));
        if (nin) LAUNCH(c, s, "r1p_inputs", k_r1p_inputs, (nin + 63) / 64, 64, nin, sh, d_v, d_vb, d_free, gsc, d_stat);
        if (m) {
            rc = msm_shared_dev_locked(c, 1, 1, nbatch * m, 0, gsc, nullptr, nullptr, d_vout, mst, nullptr, s, true, ct);
            if (rc) break;
        }
        // (2) Prover::new, the V appends, "m"; the TranscriptRng and every random scalar (32 lanes per proof)
        LAUNCH(c, s, "r1p_rng", k_r1p_rng, (nb32 + 1) / 2, 64, sh, d_ts, (const uint32_t *)d_vout, d_vb, d_rng, rnd);
        // (3) phase 1: witness, A_I1, A_O1, S1, the phase-2 challenges
        for (int ph = 1; ph <= 2 && !rc; ph++) {
            const size_t cnt = ph == 1 ? n1 : n2;
            if (ph == 2 && !n2) {
                LAUNCH(c, s, "r1p_chal2", k_r1p_chal2, (nb32 + RP_BLOCK - 1) / RP_BLOCK, RP_BLOCK, sh, (const uint32_t *)nullptr, d_ts, fields, d_rec);
                break;
            }
            sh.i0 = ph == 1 ? 0u : (uint32_t)n1;
            sh.i1 = ph == 1 ? (uint32_t)n1 : (uint32_t)n;
            if (cnt) LAUNCH(c, s, "r1p_witness", k_r1p_witness, n_pb, 64, sh, src_l, src_r, row_ptr, wterms, d_v, d_free, (const uint32_t *)fields, aw);
            if (hipMemsetAsync(gsc, 0, 3 * nbatch * ncol * 32, s) != hipSuccess) { rc = fail(c, BPGPU_ERR_HIP, "memset failed"); break; }
            const uint32_t nr = (uint32_t)(nbatch * std::max(cnt, (size_t)1));
            LAUNCH(c, s, "r1p_rows", k_r1p_rows, (nr + 63) / 64, 64, nr, sh, (uint32_t)cnt, ph == 1 ? 0u : sh.o_b2, (const uint32_t *)aw, (const uint32_t *)rnd, gsc);
            rc = msm_shared_dev_locked(c, pn, 1, 3 * nbatch, 0, gsc, nullptr, nullptr, mo, mst, nullptr, s, false, ct);
            if (rc) break;
            if (ph == 1)
                LAUNCH(c, s, "r1p_chal1", k_r1p_chal1, (nb32 + RP_BLOCK - 1) / RP_BLOCK, RP_BLOCK, sh, (const uint32_t *)mo, (const uint32_t *)(dc + ci->off_lbl_off),
                       (const uint8_t *)(dc + ci->off_lbl), d_ts, fields, d_rec);
            else
                LAUNCH(c, s, "r1p_chal2", k_r1p_chal2, (nb32 + RP_BLOCK - 1) / RP_BLOCK, RP_BLOCK, sh, (const uint32_t *)mo, d_ts, fields, d_rec);
        }
        if (rc) break;
        if (check)   // every constraint row over the finished witness and the proof's own challenges
            r1cs_check_launch_locked(c, ci, drows, sh, nbatch, chk_per, d_v, (const uint32_t *)aw, (const uint32_t *)fields, (const uint32_t *)d_stat, 0, part,
                                     (uint32_t *)io.d(r_first), nullptr, nullptr, s);
        // (4) wL, wR, wO, wV; l, r and the t polynomial; T_1, T_3..T_6
        const uint32_t npoly = (uint32_t)((n + m) * nbatch);
        if (hipMemsetAsync(terms, 0, w_t, s) != hipSuccess || hipMemsetAsync(gsc, 0, 15 * nbatch * 32, s) != hipSuccess) { rc = fail(c, BPGPU_ERR_HIP, "memset failed"); break; }
        if (npoly)
            LAUNCH(c, s, "r1p_poly", k_r1p_poly, (npoly + 63) / 64, 64, npoly, sh, (const uint32_t *)dc, (const r1cs_ent *)(dc + ci->off_ents), (const uint32_t *)aw,
                   (const uint32_t *)rnd, d_vb, (const uint32_t *)fields, (uint32_t)nrow, vecs, terms);
        LAUNCH(c, s, "r1p_tsum", k_r1p_tsum, nb32, 64, sh, (uint32_t)nrow, (const uint32_t *)terms, (const uint32_t *)rnd, fields, gsc);
        rc = msm_shared_dev_locked(c, 1, 1, 5 * nbatch, 0, gsc, nullptr, nullptr, mo, mst, nullptr, s, true, ct);
        if (rc) break;
        // (5) u, x, t_x, t_x_blinding, e_blinding, w; the IPP over G(padded_n), H(padded_n) with Q = w B
        LAUNCH(c, s, "r1p_chal3", k_r1p_chal3, (nb32 + RP_BLOCK - 1) / RP_BLOCK, RP_BLOCK, sh, (const uint32_t *)mo, (const uint32_t *)rnd, d_ts, fields, d_rec, wv);
        const uint32_t nvec = (uint32_t)(nbatch * pn);
        LAUNCH(c, s, "r1p_vecs", k_r1p_vecs, (nvec + 63) / 64, 64, nvec, sh, (const uint32_t *)fields, (const uint32_t *)vecs, lv, rv, gf, hf);
        if (hipGetLastError() != hipSuccess) { rc = fail(c, BPGPU_ERR_HIP, "launch failed"); break; }
        ippc_fixed fx;
        fx.gn = pn;
        fx.gm = 1;
        fx.w = wv;
        fx.gen_scalars = gsc;
        rc = ippc_core(c, s, pn, k, nbatch, lv, rv, gf, hf, nullptr, nullptr, nullptr, 1, d_ts, d_ipp, ipp_len, d_stb, &fx);
    } while (0);
    if (!rc && (hipMemcpyAsync(io.d(r_to), d_ts, nbatch * TS, hipMemcpyDeviceToDevice, s) != hipSuccess || io.download(0))) rc = fail(c, BPGPU_ERR_HIP, "D2H copy failed");
    rc = io.finish(rc);
    if (rc) return rc;
    // R1CSProof::to_bytes (proof.rs:83-108): version 0 exactly when A_I2, A_O2, S2 are all the identity
    const uint8_t *h_rec = (const uint8_t *)io.h(r_rec), *h_ipp = (const uint8_t *)io.h(r_ipp), *h_v = (const uint8_t *)io.h(r_vout),
                  *h_st = (const uint8_t *)io.h(r_stat), *h_stb = (const uint8_t *)io.h(r_stb), *h_ts = (const uint8_t *)io.h(r_to);
    for (size_t p = 0; p < nbatch; p++) {
        const uint8_t *rec = h_rec + p * R1P_NREC * 32;
        bool one_phase = true;
        for (size_t b = 32 * R1P_AI2; b < 32 * (R1P_S2 + 1); b++) one_phase = one_phase && rec[b] == 0;
        uint8_t *o = proofs_out + p * proof_stride;
        size_t len = 0;
        o[len++] = one_phase ? 0 : 1;
        for (uint32_t e = 0; e < R1P_NREC; e++) {
            if (one_phase && e >= R1P_AI2 && e <= R1P_S2) continue;
            memcpy(o + len, rec + 32 * e, 32);
            len += 32;
        }
        memcpy(o + len, h_ipp + p * ipp_len, ipp_len);
        len += ipp_len;
        memset(o + len, 0, proof_stride - len);
        proof_lens_out[p] = (uint32_t)len;
        uint32_t st;
        memcpy(&st, h_st + 4 * p, 4);
        status_out[p] = (uint8_t)std::max(st, (uint32_t)h_stb[p]);
    }
    if (m) memcpy(commitments_out, h_v, nbatch * m * 32);
    if (transcripts_out) memcpy(transcripts_out, h_ts, nbatch * TS);
    if (check) {   // a proof whose witness fails is void: no proof bytes, its transcript as it came (a non-canonical input outranks it)
        memcpy(unsat_first_out, io.h(r_first), nbatch * 4);
        for (size_t p = 0; p < nbatch; p++) {
            if (status_out[p] != 0) unsat_first_out[p] = BPGPU_R1CS_SATISFIED;
            if (unsat_first_out[p] == BPGPU_R1CS_SATISFIED) continue;
            status_out[p] = BPGPU_R1CS_UNSATISFIED;
            memset(proofs_out + p * proof_stride, 0, proof_stride);
            proof_lens_out[p] = 0;
            if (transcripts_out) memcpy(transcripts_out + p * TS, transcripts + p * transcript_stride, TS);
        }
    }
    return BPGPU_OK;
}

extern "C" int bpgpu_r1cs_prove_batch(bpgpu_ctx *c, const bpgpu_r1cs_circuit *ci, const bpgpu_r1cs_witness *wi, size_t nbatch, const uint8_t *v,
                                      const uint8_t *v_blinding, const uint8_t *free_inputs, const uint8_t *transcripts, size_t transcript_stride,
                                      const uint8_t *rng32, uint8_t *proofs_out, size_t proof_stride, uint32_t *proof_lens_out, uint8_t *commitments_out,
                                      uint8_t *status_out, uint8_t *transcripts_out) {
    return r1cs_prove_impl(c, ci, wi, nbatch, v, v_blinding, free_inputs, transcripts, transcript_stride, rng32, proofs_out, proof_stride, proof_lens_out,
                           commitments_out, status_out, transcripts_out, false, nullptr);
}

extern "C" int bpgpu_r1cs_prove_batch_checked(bpgpu_ctx *c, const bpgpu_r1cs_circuit *ci, const bpgpu_r1cs_witness *wi, size_t nbatch, const uint8_t *v,
                                              const uint8_t *v_blinding, const uint8_t *free_inputs, const uint8_t *transcripts, size_t transcript_stride,
                                              const uint8_t *rng32, uint8_t *proofs_out, size_t proof_stride, uint32_t *proof_lens_out,
                                              uint8_t *commitments_out, uint8_t *status_out, uint8_t *transcripts_out, uint32_t *unsat_first_out) {
    return r1cs_prove_impl(c, ci, wi, nbatch, v, v_blinding, free_inputs, transcripts, transcript_stride, rng32, proofs_out, proof_stride, proof_lens_out,
                           commitments_out, status_out, transcripts_out, true, unsat_first_out);
}

// The stand-alone check: the challenges loaded from the caller's values, then the prover's own input and witness launches (no V rows,
// no blindings, no transcript, no generators) and the check launches.
extern "C" int bpgpu_r1cs_witness_check(bpgpu_ctx *c, const bpgpu_r1cs_circuit *ci, const bpgpu_r1cs_witness *wi, size_t nbatch, const uint8_t *v,
                                        const uint8_t *free_inputs, const uint8_t *challenges, uint32_t *first_out, uint32_t *count_out, uint8_t *map_out,
                                        size_t map_stride, uint8_t *status_out) {
    if (!ci || !wi) return BPGPU_ERR_INVALID_ARG;
    if (wi->m != ci->m || wi->n1 != ci->n1 || wi->n != ci->n || wi->nch != ci->nch) return fail(c, BPGPU_ERR_INVALID_ARG, "witness program of another circuit");
    const size_t m = ci->m, n = ci->n, nf = wi->nfree, nch = ci->nch, Q = ci->Q, map_bytes = (Q + 7) / 8, mapw = map_out ? (Q + 31) / 32 : 0;
    if (nch && !challenges) return fail(c, BPGPU_ERR_INVALID_ARG, "the circuit has %zu challenges: their values are needed", nch);
    if (map_out && map_stride < map_bytes) return fail(c, BPGPU_ERR_INVALID_ARG, "map_stride %zu < %zu", map_stride, map_bytes);
    if (!c) return BPGPU_ERR_INVALID_ARG;
    if (nbatch == 0) return BPGPU_OK;
    if ((m && !v) || (nf && !free_inputs) || !first_out || !status_out) return BPGPU_ERR_INVALID_ARG;
    if ((uint64_t)nbatch * (m + nf + nch + 1) > 0x7fffffffull / 64 || (uint64_t)nbatch * std::max(3 * n + nch, (size_t)1) * 40 > (4ull << 30) ||
        (uint64_t)nbatch * std::max(mapw, (size_t)1) * 4 > (1ull << 30))
        return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large for this circuit");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    r1p_shape sh{};
    sh.c.m = (uint32_t)m, sh.c.n1 = ci->n1, sh.c.n = (uint32_t)n, sh.c.pn = ci->pn, sh.c.k = ci->k;
    sh.c.two_phase = ci->two_phase, sh.c.nch = ci->nch, sh.c.Q = ci->Q;
    sh.c.f_ch = 0;                       // the only fields: the challenges
    sh.c.nfields = (uint32_t)nch;
    sh.c.nproofs = (uint32_t)nbatch;
    sh.nfree = (uint32_t)nf;
    sh.i0 = 0, sh.i1 = (uint32_t)n;      // every challenge is known: one witness launch over both phases
    char *dw = nullptr, *drows = nullptr;
    int rc = r1cs_witness_on(c, wi, &dw);
    if (rc) return rc;
    rc = r1cs_rows_on(c, ci, &drows);
    if (rc) return rc;
    const size_t per = r1c_slice(ci->rows, nbatch);
    hipStream_t s = c->stream;
    host_call<bpgpu_ctx> io(c, s);
    const int r_v = io.in(nbatch * m * 32 + 64), r_free = io.in(nbatch * nf * 32 + 64), r_ch = io.in(nbatch * nch * 32 + 64);
    const int r_first = io.out(nbatch * 4), r_cnt = io.out(nbatch * 4), r_stat = io.out(nbatch * 4), r_map = io.out(nbatch * mapw * 4);
    io.secrets(io.in_bytes());   // values and free inputs (the challenges ride along)
    rc = io.open();
    if (rc) return io.finish(rc);
    if (m) io.put(r_v, v, nbatch * m * 32);
    if (nf) io.put(r_free, free_inputs, nbatch * nf * 32);
    if (nch) io.put(r_ch, challenges, nbatch * nch * 32);
    const uint8_t *d_v = (const uint8_t *)io.d(r_v), *d_free = (const uint8_t *)io.d(r_free), *d_ch = (const uint8_t *)io.d(r_ch);
    uint32_t *d_first = (uint32_t *)io.d(r_first), *d_cnt = (uint32_t *)io.d(r_cnt), *d_stat = (uint32_t *)io.d(r_stat),
             *d_map = map_out ? (uint32_t *)io.d(r_map) : nullptr;
    rc = io.upload();
    if (!rc) rc = HIPRC(c, hipMemsetAsync(io.d(r_first), 0, io.out_bytes(), s));
    if (!rc) rc = HIPRC(c, hipMemsetAsync(d_first, 0xff, nbatch * 4, s));   // R1C_SATISFIED
    if (rc) return io.finish(rc);
    const size_t w_aw = align_up(3 * std::max(n, (size_t)1) * nbatch * 40), w_f = align_up(std::max(nch, (size_t)1) * nbatch * 40),
                 w_part = align_up((size_t)ci->rows.nslots * per * 32);
    if ((rc = rpp_reserve(c, w_aw + w_f + w_part))) return io.finish(rc);
    uint32_t *aw = (uint32_t *)c->rpp_buf, *fields = (uint32_t *)(c->rpp_buf + w_aw), *part = (uint32_t *)(c->rpp_buf + w_aw + w_f);
    const uint32_t *src_l = (const uint32_t *)dw, *src_r = src_l + n, *row_ptr = (const uint32_t *)(dw + wi->off_row);
    const r1p_term *wterms = (const r1p_term *)(dw + wi->off_terms);
    const uint32_t nb32 = (uint32_t)nbatch, nchal = (uint32_t)(nbatch * nch), nin = (uint32_t)(nbatch * (m + nf));
    if (nchal) LAUNCH(c, s, "r1c_chal", k_r1c_chal, (nchal + 63) / 64, 64, nchal, sh, d_ch, fields, d_stat);
    if (nin) LAUNCH(c, s, "r1p_inputs", k_r1p_inputs, (nin + 63) / 64, 64, nin, sh, d_v, (const uint8_t *)nullptr, d_free, (uint32_t *)nullptr, d_stat);
    if (n) LAUNCH(c, s, "r1p_witness", k_r1p_witness, (nb32 + 63) / 64, 64, sh, src_l, src_r, row_ptr, wterms, d_v, d_free, (const uint32_t *)fields, aw);
    r1cs_check_launch_locked(c, ci, drows, sh, nbatch, per, d_v, (const uint32_t *)aw, (const uint32_t *)fields, (const uint32_t *)d_stat, (uint32_t)mapw, part,
                             d_first, d_cnt, d_map, s);
    if (hipGetLastError() != hipSuccess) rc = fail(c, BPGPU_ERR_HIP, "launch failed");
    rc = io.finish(io.download(rc));
    if (rc) return rc;
    memcpy(first_out, io.h(r_first), nbatch * 4);
    if (count_out) memcpy(count_out, io.h(r_cnt), nbatch * 4);
    for (size_t p = 0; p < nbatch; p++) {
        uint32_t st;
        memcpy(&st, io.h(r_stat) + 4 * p, 4);
        status_out[p] = (uint8_t)st;
        if (map_out) {   // (little-endian words: bit q % 8 of byte q / 8)
            memcpy(map_out + p * map_stride, io.h(r_map) + p * mapw * 4, map_bytes);
            memset(map_out + p * map_stride + map_bytes, 0, map_stride - map_bytes);
        }
    }
    return BPGPU_OK;
}

// ---- batches of transcripts (ts_batch.h, k_ts_batch.hip) -------------------------------------------------------------------
// What the kernel reads besides the rows' data: the ops (tsb_op, device pointers inside), then the label bytes, then -- where the
// start is Transcript::new(label) -- that one state, computed here once and shared by the rows.
struct tsb_plan {
    size_t nops = 0, off_labels = 0, off_st0 = 0, bytes = 0;
    uint32_t out_len[BPGPU_TS_MAX_OPS];   // bytes a row of op o writes (0: an append)
};

// the checks both forms share (lens is device memory in one of them: the host form checks it as it stages the rows)
static int tsb_check(bpgpu_ctx *c, size_t nbatch, const uint8_t *new_label, size_t new_label_len, const void *states_in, size_t stride_in,
                     const bpgpu_ts_op *ops, size_t nops, const void *states_out, tsb_plan &pl) {
    if ((new_label != nullptr) == (states_in != nullptr)) return fail(c, BPGPU_ERR_INVALID_ARG, "exactly one of new_label and states_in is needed");
    if (new_label && new_label_len > BPGPU_TS_MAX_LABEL) return fail(c, BPGPU_ERR_INVALID_ARG, "new_label_len %zu > %d", new_label_len, BPGPU_TS_MAX_LABEL);
    if (states_in && stride_in != 0 && stride_in != BPGPU_TRANSCRIPT_BYTES)
        return fail(c, BPGPU_ERR_INVALID_ARG, "stride_in neither 0 nor BPGPU_TRANSCRIPT_BYTES");
    if (nops > BPGPU_TS_MAX_OPS || (nops && !ops)) return fail(c, BPGPU_ERR_INVALID_ARG, "nops %zu > %d, or ops missing", nops, BPGPU_TS_MAX_OPS);
    if (nbatch > 0x7fffffffu / 64) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large");
    size_t labels = 0;
    for (size_t o = 0; o < nops; o++) {
        const bpgpu_ts_op &op = ops[o];
        if (op.label_len > BPGPU_TS_MAX_LABEL || (op.label_len && !op.label))
            return fail(c, BPGPU_ERR_INVALID_ARG, "op %zu: label_len %zu > %d, or label missing", o, op.label_len, BPGPU_TS_MAX_LABEL);
        labels += op.label_len;
        pl.out_len[o] = 0;
        size_t need = 0;   // bytes of `data` a row takes
        switch (op.kind) {
        case BPGPU_TS_APPEND:
            if (op.len > BPGPU_TS_MAX_LEN) return fail(c, BPGPU_ERR_INVALID_ARG, "op %zu: len %zu > %d", o, op.len, BPGPU_TS_MAX_LEN);
            need = op.len;
            break;
        case BPGPU_TS_APPEND_U64:
            if (op.stride != 0 && op.stride != 8) return fail(c, BPGPU_ERR_INVALID_ARG, "op %zu: the stride of uint64 values is 8, or 0 for one value", o);
            need = 8;
            break;
        case BPGPU_TS_CHALLENGE:
            if (op.len > BPGPU_TS_MAX_CHALLENGE) return fail(c, BPGPU_ERR_INVALID_ARG, "op %zu: challenge of %zu > %d bytes", o, op.len, BPGPU_TS_MAX_CHALLENGE);
            need = op.len;
            pl.out_len[o] = (uint32_t)op.len;
            break;
        case BPGPU_TS_CHALLENGE_SCALAR:
            need = 32;
            pl.out_len[o] = 32;
            break;
        default:
            return fail(c, BPGPU_ERR_INVALID_ARG, "op %zu: unknown kind %u", o, op.kind);
        }
        const bool output = op.kind == BPGPU_TS_CHALLENGE || op.kind == BPGPU_TS_CHALLENGE_SCALAR;
        if (output && (op.stride == 0 || op.stride < need)) return fail(c, BPGPU_ERR_INVALID_ARG, "op %zu: an output needs a stride of at least %zu bytes per row", o, need);
        if (op.lens && op.kind != BPGPU_TS_APPEND) return fail(c, BPGPU_ERR_INVALID_ARG, "op %zu: lens goes with BPGPU_TS_APPEND only", o);
        if (nbatch && need && !op.data) return fail(c, BPGPU_ERR_INVALID_ARG, "op %zu: data missing", o);
    }
    if (nbatch && !states_out) return fail(c, BPGPU_ERR_INVALID_ARG, "states_out missing");
    pl.nops = nops;
    pl.off_labels = nops * sizeof(tsb_op);
    pl.off_st0 = (pl.off_labels + labels + 7) & ~(size_t)7;
    pl.bytes = pl.off_st0 + (new_label ? BPGPU_TRANSCRIPT_BYTES : 0);
    return BPGPU_OK;
}

// the ops and labels into `blob` (host memory that is then copied to the device); data_of(o) / lens_of(o): where op o's rows are on the device
template <class D, class Ln>
static void tsb_fill(char *blob, const tsb_plan &pl, const bpgpu_ts_op *ops, const uint8_t *new_label, size_t new_label_len, D data_of, Ln lens_of) {
    tsb_op *dst = (tsb_op *)blob;
    uint32_t loff = 0;
    for (size_t o = 0; o < pl.nops; o++) {
        const bpgpu_ts_op &op = ops[o];
        tsb_op &d = dst[o];
        d.kind = op.kind == BPGPU_TS_CHALLENGE ? TSB_CHALLENGE : op.kind == BPGPU_TS_CHALLENGE_SCALAR ? TSB_CHALLENGE_SCALAR : TSB_APPEND;
        d.label_off = loff;
        d.label_len = (uint32_t)op.label_len;
        d.len = op.kind == BPGPU_TS_APPEND_U64 ? 8u : op.kind == BPGPU_TS_CHALLENGE_SCALAR ? 64u : (uint32_t)op.len;
        d.data = (uint8_t *)data_of(o, &d.stride);
        d.lens = (const uint32_t *)lens_of(o);
        if (op.label_len) memcpy(blob + pl.off_labels + loff, op.label, op.label_len);
        loff += (uint32_t)op.label_len;
    }
    if (new_label) bpgpu_transcript_new(new_label, new_label_len, (uint8_t *)blob + pl.off_st0);
}

static void tsb_launch(bpgpu_ctx *c, hipStream_t s, size_t nbatch, const tsb_plan &pl, const char *d_blob, const void *d_states_in, size_t stride_in,
                       void *d_states_out) {
    const uint32_t nb32 = (uint32_t)nbatch;
    LAUNCH(c, s, "ts_batch", k_ts_batch, (nb32 + TSB_BLOCK - 1) / TSB_BLOCK, TSB_BLOCK, nb32, (const uint32_t *)d_states_in, (uint32_t)(stride_in / 4),
           (uint32_t *)d_states_out, (const tsb_op *)d_blob, (uint32_t)pl.nops, (const uint8_t *)d_blob + pl.off_labels);
}

extern "C" int bpgpu_transcript_batch(bpgpu_ctx *c, size_t nbatch, const uint8_t *new_label, size_t new_label_len, const uint8_t *states_in, size_t stride_in,
                                      const bpgpu_ts_op *ops, size_t nops, uint8_t *states_out) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    tsb_plan pl;
    int rc = tsb_check(c, nbatch, new_label, new_label_len, states_in, stride_in, ops, nops, states_out, pl);
    if (rc) return rc;
    if (nbatch == 0) return BPGPU_OK;
    const size_t TS = BPGPU_TRANSCRIPT_BYTES, nstates = !states_in ? 0 : stride_in ? nbatch : 1;
    for (size_t r = 0; r < nstates; r++)
        if (!ts_state_ok(states_in + r * TS)) return fail(c, BPGPU_ERR_INVALID_ARG, "malformed transcript state %zu", r);
    // one input region: the script, the start states, then op after op its rows (packed at the stride len) and its lens;
    // one output region: the states, then op after op its challenges (packed at their own length)
    size_t off_in[BPGPU_TS_MAX_OPS], off_lens[BPGPU_TS_MAX_OPS], off_out[BPGPU_TS_MAX_OPS];
    const size_t off_states = (pl.bytes + 7) & ~(size_t)7;
    size_t in_bytes = off_states + nstates * TS, out_bytes = nbatch * TS;
    for (size_t o = 0; o < nops; o++) {
        const bpgpu_ts_op &op = ops[o];
        off_in[o] = off_lens[o] = off_out[o] = 0;
        if (pl.out_len[o]) {
            off_out[o] = out_bytes;
            out_bytes += (nbatch * pl.out_len[o] + 7) & ~(size_t)7;
            continue;
        }
        const size_t len = op.kind == BPGPU_TS_APPEND_U64 ? 8 : op.len;
        off_in[o] = in_bytes;
        in_bytes += ((op.stride ? nbatch : 1) * len + 7) & ~(size_t)7;
        if (op.lens) {
            off_lens[o] = in_bytes;
            in_bytes += (nbatch * 4 + 7) & ~(size_t)7;
        }
        if (in_bytes > ((size_t)1 << 31)) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large: more than 2 GiB of messages");
    }
    if (out_bytes > ((size_t)1 << 31)) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large: more than 2 GiB of challenges");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    host_call<bpgpu_ctx> io(c, s);
    const int r_in = io.in(in_bytes), r_out = io.out(out_bytes);
    io.secrets(io.in_bytes());   // the messages may be secret, and nothing tells the script from them
    rc = io.open();
    if (rc) return io.finish(rc);
    char *h = io.h(r_in), *d = io.d(r_in);
    tsb_fill(h, pl, ops, new_label, new_label_len,
             [&](size_t o, uint64_t *stride) -> char * {
                 if (pl.out_len[o]) {
                     *stride = pl.out_len[o];
                     return io.d(r_out) + off_out[o];
                 }
                 *stride = !ops[o].stride ? 0 : ops[o].kind == BPGPU_TS_APPEND_U64 ? 8 : ops[o].len;
                 return d + off_in[o];
             },
             [&](size_t o) -> char * { return ops[o].lens ? d + off_lens[o] : nullptr; });
    if (nstates) memcpy(h + off_states, states_in, nstates * TS);
    for (size_t o = 0; o < nops; o++) {
        const bpgpu_ts_op &op = ops[o];
        if (pl.out_len[o]) continue;
        const size_t len = op.kind == BPGPU_TS_APPEND_U64 ? 8 : op.len;
        // a row is read up to its own length; ONE message for all rows (stride 0) is staged whole, whatever the rows take of it
        for (size_t r = 0; r < nbatch && op.lens && !rc; r++)
            if (op.lens[r] > op.len) rc = fail(c, BPGPU_ERR_INVALID_ARG, "op %zu: lens[%zu] = %u > len = %zu", o, r, op.lens[r], op.len);
        if (rc) return io.finish(rc);   // (rows of earlier ops are staged already: the exit clears them)
        for (size_t r = 0; r < (op.stride ? nbatch : 1) && len; r++)
            memcpy(h + off_in[o] + r * len, (const char *)op.data + r * op.stride, op.lens && op.stride ? op.lens[r] : len);
        if (op.lens) memcpy(h + off_lens[o], op.lens, nbatch * 4);
    }
    rc = io.upload();
    if (rc) return io.finish(rc);
    tsb_launch(c, s, nbatch, pl, d, new_label ? d + pl.off_st0 : d + off_states, new_label ? 0 : stride_in, io.d(r_out));
    if (hipGetLastError() != hipSuccess) rc = fail(c, BPGPU_ERR_HIP, "launch failed");
    rc = io.finish(io.download(rc));
    if (rc) return rc;
    const char *ho = io.h(r_out);
    memcpy(states_out, ho, nbatch * TS);
    for (size_t o = 0; o < nops; o++)
        for (size_t r = 0; r < nbatch && pl.out_len[o]; r++) memcpy((char *)ops[o].data + r * ops[o].stride, ho + off_out[o] + r * pl.out_len[o], pl.out_len[o]);
    return BPGPU_OK;
}

extern "C" int bpgpu_transcript_batch_dev(bpgpu_ctx *c, size_t nbatch, const uint8_t *new_label, size_t new_label_len, const void *d_states_in, size_t stride_in,
                                          const bpgpu_ts_op *ops, size_t nops, void *d_states_out, void *stream) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    tsb_plan pl;
    int rc = tsb_check(c, nbatch, new_label, new_label_len, d_states_in, stride_in, ops, nops, d_states_out, pl);
    if (rc) return rc;
    if (nbatch == 0) return BPGPU_OK;
    uintptr_t al = (uintptr_t)d_states_in | (uintptr_t)d_states_out;
    for (size_t o = 0; o < nops; o++) al |= (uintptr_t)ops[o].lens;
    if (al & 3) return fail(c, BPGPU_ERR_INVALID_ARG, "device states and lens must be 4-byte aligned");
    if (d_states_in == d_states_out && stride_in == 0 && nbatch > 1)
        return fail(c, BPGPU_ERR_INVALID_ARG, "states_out may be states_in only with one state per row");
    return dev_call(c, stream, [&](hipStream_t s) {
        int rcb = ipp_reserve(c, align_up(pl.bytes));
        if (rcb) return rcb;
        char *h = nullptr, *d = c->ipp_buf;
        if ((rcb = c->io.pin_alloc(pl.bytes, &h))) return rcb;
        tsb_fill(h, pl, ops, new_label, new_label_len,
                 [&](size_t o, uint64_t *stride) -> char * {
                     *stride = ops[o].stride;
                     return (char *)ops[o].data;
                 },
                 [&](size_t o) -> char * { return (char *)ops[o].lens; });
        if (pl.bytes && (rcb = HIPRC(c, hipMemcpyAsync(d, h, pl.bytes, hipMemcpyHostToDevice, s)))) return rcb;
        if ((rcb = c->io.pin_mark(s))) return rcb;
        tsb_launch(c, s, nbatch, pl, d, new_label ? d + pl.off_st0 : d_states_in, new_label ? 0 : stride_in, d_states_out);
        if (hipGetLastError() != hipSuccess) return fail(c, BPGPU_ERR_HIP, "launch failed");
        return BPGPU_OK;
    });
}

// the pool form: the whole call on the next device's context (pool.hip)
extern "C" int bpgpu_internal_pool_run_on_context(bpgpu_pool *p, size_t nbatch, uint8_t *verdict, int (*run)(bpgpu_ctx *, void *), void *arg);
namespace {
struct r1cs_call {
    const bpgpu_r1cs_circuit *circuit;
    size_t nbatch, proof_stride, transcript_stride;
    const uint8_t *proofs, *commitments, *transcripts, *rng32;
    const uint32_t *proof_lens;
    uint8_t *verdict, *msm_out, *transcripts_out;
};
int r1cs_call_run(bpgpu_ctx *c, void *arg) {
    const r1cs_call *a = (const r1cs_call *)arg;
    return bpgpu_r1cs_verify_batch_ts(c, a->circuit, a->nbatch, a->proofs, a->proof_stride, a->proof_lens, a->commitments, a->transcripts,
                                      a->transcript_stride, a->rng32, a->verdict, a->msm_out, a->transcripts_out);
}
struct r1cs_rlc_call {
    size_t ngroups;
    const bpgpu_r1cs_circuit *const *circuits;
    const size_t *nbatch, *proof_stride, *transcript_stride;
    const uint8_t *const *proofs;
    const uint32_t *const *proof_lens;
    const uint8_t *const *commitments, *const *transcripts;
    const uint8_t *rng32, *weights64;
    uint8_t *verdict, *batch_out, *transcripts_out;
};
int r1cs_rlc_call_run(bpgpu_ctx *c, void *arg) {
    const r1cs_rlc_call *a = (const r1cs_rlc_call *)arg;
    return bpgpu_r1cs_verify_rlc(c, a->ngroups, a->circuits, a->nbatch, a->proofs, a->proof_stride, a->proof_lens, a->commitments, a->transcripts,
                                 a->transcript_stride, a->rng32, a->weights64, a->verdict, a->batch_out, a->transcripts_out);
}
}  // namespace

extern "C" int bpgpu_pool_r1cs_verify_ts(bpgpu_pool *pool, const bpgpu_r1cs_circuit *circuit, size_t nbatch, const uint8_t *proofs, size_t proof_stride,
                                         const uint32_t *proof_lens, const uint8_t *commitments, const uint8_t *transcripts, size_t transcript_stride,
                                         const uint8_t *rng32, uint8_t *verdict, uint8_t *msm_out, uint8_t *transcripts_out) {
    if (!pool || !circuit) return BPGPU_ERR_INVALID_ARG;
    r1cs_call a{circuit, nbatch, proof_stride, transcript_stride, proofs, commitments, transcripts, rng32, proof_lens, verdict, msm_out, transcripts_out};
    return bpgpu_internal_pool_run_on_context(pool, nbatch, verdict, r1cs_call_run, &a);
}

extern "C" int bpgpu_pool_r1cs_verify_rlc(bpgpu_pool *pool, size_t ngroups, const bpgpu_r1cs_circuit *const *circuits, const size_t *nbatch,
                                          const uint8_t *const *proofs, const size_t *proof_stride, const uint32_t *const *proof_lens,
                                          const uint8_t *const *commitments, const uint8_t *const *transcripts, const size_t *transcript_stride,
                                          const uint8_t *rng32, const uint8_t *weights64, uint8_t *verdict, uint8_t *batch_out, uint8_t *transcripts_out) {
    if (!pool || ngroups == 0 || !circuits || !nbatch || !proofs || !proof_stride || !proof_lens || !commitments || !transcripts || !transcript_stride)
        return BPGPU_ERR_INVALID_ARG;
    size_t total = 0;
    for (size_t g = 0; g < ngroups; g++) total += nbatch[g];
    if (total == 0) {   // (as the context form: nothing to combine)
        for (size_t g = 0; g < ngroups; g++)
            if (!circuits[g]) return BPGPU_ERR_INVALID_ARG;
        if (batch_out) memset(batch_out, 0, 33);
        return BPGPU_OK;
    }
    r1cs_rlc_call a{ngroups, circuits, nbatch, proof_stride, transcript_stride, proofs, proof_lens, commitments, transcripts, rng32, weights64,
                    verdict, batch_out, transcripts_out};
    return bpgpu_internal_pool_run_on_context(pool, total, verdict, r1cs_rlc_call_run, &a);
}

// ============================================================================
// batch-combined range-proof verification over MIXED shapes (rlc_mix.h; an ADDITIONAL entry point, as bpgpu_rangeproof_verify_rlc)
// ============================================================================
namespace {
// one group's inputs on the device; its proof i is proof gp0 + i of the call, its unique terms start at u0 of the combined list
struct rp_mix_group {
    size_t n, m, nbatch, proof_len, k, gp0, u0;
    const char *d_proofs, *d_coms;
    const uint8_t *label;
    size_t label_len;
    bool whole;   // rejected as a whole: every proof gets the code of the per-shape path, the group contributes nothing
    // caller-supplied transcripts (bpgpu_rangeproof_verify_rlc_mixed_ts): h_ts (host) is ONE state for the group (ts_stride == 0) or one per
    // proof, then also staged at d_ts_in; ts_uniform: all of them at one STROBE position (u_*): the scripted replay.  d_ts_out (optional):
    // the group's slice of the advanced states.  h_ts == nullptr: the group starts from its label.
    const uint8_t *h_ts = nullptr;
    size_t ts_stride = 0;
    const char *d_ts_in = nullptr;
    char *d_ts_out = nullptr;
    bool ts_uniform = false;
    uint32_t u_pos = 0, u_pos_begin = 0, u_flags = 0;
};
// where the per-proof path starts the group's proofs (groups rejected as a whole, and the fallback)
static rp_transcripts rp_mix_transcripts(const rp_mix_group &g) {
    rp_transcripts tr;
    if (!g.h_ts) {
        tr.label = g.label;
        tr.label_len = g.label_len;
        return tr;
    }
    if (g.ts_stride) {
        tr.d_ts_in = g.d_ts_in;
        tr.ts_uniform = g.ts_uniform;
        tr.u_pos = g.u_pos, tr.u_pos_begin = g.u_pos_begin, tr.u_flags = g.u_flags;
    } else {
        tr.shared_ts = g.h_ts;
    }
    tr.d_ts_out = g.d_ts_out;
    return tr;
}
}  // namespace

// A group's class (rp_classify): whole = false -- a shape the combination takes (k set); whole = true -- the per-shape path gives every proof
// of the group one code
static int rp_mix_classify(bpgpu_ctx *c, size_t n, size_t m, size_t proof_len, size_t *k_out, bool *whole) {
    const rp_class cl = rp_classify(n, m, proof_len, c->gens_capacity, c->party_capacity);
    if (cl.unsupported) return fail(c, BPGPU_ERR_INVALID_ARG, "n*m > 2^%d not supported", BP_RP_MAX_K);
    *whole = cl.all_verdict || cl.shape_verdict;
    *k_out = *whole ? 0 : cl.k;
    return BPGPU_OK;
}

// R = sum_i rho_i MegaCheck_i over every group: per group launch 1 (k_rlc_mix_front) and the weigh launch, then the reduction of the
// limb sums, ONE shared-generator MSM over (N, M) = (max n, max m) and the verdicts (undecided where R is not the identity).
// d_rng64 / d_weights64: total x 64 bytes in call order, or null -- then drawn here, keyed by the call-global index; *d_rng_used is the
// buffer the batching challenges came from (for the per-proof fallback).
static int rp_mix_dev_locked(bpgpu_ctx *c, std::vector<rp_mix_group> &gr, size_t total, const char *d_rng64, const char *d_weights64, uint8_t *d_verdict,
                             uint8_t *d_batch, hipStream_t s, const char **d_rng_used) {
    if (!c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    size_t N = 0, M = 0, u_total = 0;
    for (auto &g : gr) {
        if (g.whole || g.nbatch == 0) continue;
        N = std::max(N, g.n), M = std::max(M, g.m);
        g.u0 = u_total;
        u_total += g.nbatch * (4 + 2 * g.k + g.m);
    }
    if (u_total > RM_MAX_TERMS) return fail(c, BPGPU_ERR_INVALID_ARG, "more than 2^24 proof-specific terms in one call");
    const size_t nrows = N ? 2 * N * M + 2 : 0;
    comb_layout lay(std::max<size_t>(u_total, 1) * 32, nrows * 80 + 16, nrows * 32 + 16, 0);   // (no weights of its own: they arrive as 64 bytes per proof)
    const size_t off_gst = lay.add(total * 4), off_rdraw = lay.add(d_rng64 ? 0 : total * 64), off_wdraw = lay.add(d_weights64 ? 0 : total * 64);
    int rc = lay.reserve(c);
    if (rc) return rc;
    char *d_csc = lay.d_csc, *d_cpt = lay.d_cpt, *d_acc = lay.d_acc, *d_gen = lay.d_row, *d_res = lay.d_res, *d_gst = lay.base + off_gst,
         *d_rdraw = lay.base + off_rdraw, *d_wdraw = lay.base + off_wdraw;
    const uint32_t n32 = (uint32_t)total;
    if (!d_rng64) {   // as the per-proof path's seeded mode (the tests' chain seed pins it), but per call and under this entry point's domain
        rlc_key key;
        if (c->test_seed_set) memcpy(key.w, c->test_seed, 32);
        else if (!bp::fast_random((uint8_t *)key.w, 32)) return fail(c, BPGPU_ERR_HIP, "getrandom failed");
        LAUNCH(c, s, "rlc_mix_draw", k_rlc_mix_draw, (n32 + 63) / 64, 64, n32, key, (uint32_t)RM_RNG_DOMAIN, (uint32_t *)d_rdraw);
        d_rng64 = d_rdraw;
    }
    if (!d_weights64) {   // (never the test seed: weights stay unpredictable)
        rlc_key key;
        if (!bp::fast_random((uint8_t *)key.w, 32)) return fail(c, BPGPU_ERR_HIP, "getrandom failed");
        LAUNCH(c, s, "rlc_mix_draw", k_rlc_mix_draw, (n32 + 63) / 64, 64, n32, key, (uint32_t)RM_WEIGHT_DOMAIN, (uint32_t *)d_wdraw);
        d_weights64 = d_wdraw;
    }
    *d_rng_used = d_rng64;
    // groups rejected as a whole: the per-shape path's own codes, written now; the verdict launch leaves them alone
    for (const auto &g : gr) {
        if (!g.whole || g.nbatch == 0) continue;
        rp_call a = rp_call_of(g.n, g.m, g.nbatch, g.d_proofs, g.proof_len, g.d_coms, rp_mix_transcripts(g), d_rng64 + 64 * g.gp0, d_verdict + g.gp0);
        a.s = s;
        rc = rp_verify_chain(c, a);
        if (rc) return rc;
        HIPCHK(c, hipMemsetAsync(d_gst + 4 * g.gp0, 0xff, 4 * g.nbatch, s));   // (every word RLC_GSTATUS_DONE)
    }
    if (nrows) HIPCHK(c, hipMemsetAsync(d_acc, 0, nrows * 80, s));
    for (const auto &g : gr) {
        if (g.whole || g.nbatch == 0) continue;
        rp_shape sh;
        sh.n = (uint32_t)g.n, sh.m = (uint32_t)g.m, sh.nm = (uint32_t)(g.n * g.m), sh.k = (uint32_t)g.k, sh.U = (uint32_t)(4 + 2 * g.k + g.m);
        sh.proof_len = (uint32_t)g.proof_len, sh.nproofs = (uint32_t)g.nbatch, sh.shape_verdict = 0;
        uint32_t lg_m = 0;
        while (((size_t)1 << lg_m) < g.m) lg_m++;
        rm_group mg;
        mg.nproofs = sh.nproofs, mg.nstride = (sh.nproofs + 63) / 64 * 64, mg.n = sh.n, mg.m = sh.m, mg.N = (uint32_t)N, mg.M = (uint32_t)M;
        mg.gp0 = (uint32_t)g.gp0, mg.u0 = (uint32_t)g.u0;
        const uint64_t nt = (uint64_t)mg.nstride * rm_terms(sh);   // (a multiple of 64: whole wavefronts)
        if (nt > 0x7fffffffull) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large for this shape");
        const rp_fields fl = rp_field_layout(sh.k, sh.m);
        arena_plan ap;
        const size_t off_fields = ap.add((size_t)fl.count * g.nbatch * BP_RP_REC * 4 + 16), off_st = ap.add(g.nbatch * 4),
                     off_usc = ap.add(g.nbatch * sh.U * 32);
        rc = arena_reserve(c, ap.total);
        if (rc) return rc;
        char *a = c->arena;
        // Where the group's transcripts start, and the form of the front end's transcript role.  A label: always the per-shape script.  The
        // caller's states: rangeproof_domain_sep(n, m) is applied on the device (part of the script then); one state for the group travels in
        // `init` like a label's; one state per proof with all of them at one STROBE position: the script compiled for that position, the
        // sponge words from ts_in; positions that differ (or option transcript_script = 0): the byte-wise replay.
        rp_strobe_init init;
        const uint32_t *ts_in = nullptr;
        if (!g.h_ts) make_strobe_init(init, g.label, g.label_len, g.n, g.m);
        else if (!g.ts_stride) strobe_init_from_state(init, g.h_ts);
        else {
            memset(&init, 0, sizeof init);
            init.pos = g.u_pos, init.pos_begin = g.u_pos_begin, init.cur_flags = g.u_flags;   // (meaningful when ts_uniform only)
            ts_in = (const uint32_t *)g.d_ts_in;
        }
        const bool replay = g.h_ts && (c->no_script || (g.ts_stride && !g.ts_uniform));
        const rp_script_hdr *d_script = nullptr;
        if (!replay) {
            rc = script_for(c, s, sh.n, sh.m, sh.k, init, g.h_ts != nullptr, &d_script);
            if (rc) return rc;
        }
        HIPCHK(c, hipMemsetAsync(a + off_st, 0, g.nbatch * 4, s));
        const uint32_t n_tr = (sh.nproofs + RP_BLOCK - 1) / RP_BLOCK, n_pt = (sh.nproofs * sh.U + RP_BLOCK - 1) / RP_BLOCK;
        // rng64 / weights64 rows are indexed by the proof's position in the CALL: this group's slice starts at gp0.  Soundness rests on it --
        // a slice taken at 0 would hand (group 0, proof i) and (group 1, proof i) the same weight
        if (replay)
            LAUNCH(c, s, "rlc_mix_front", k_rlc_mix_front_replay, n_tr + n_pt, RP_BLOCK, sh, init, n_tr, (const uint8_t *)g.d_proofs, (const uint8_t *)g.d_coms,
                   (const uint8_t *)d_rng64 + 64 * g.gp0, (const uint8_t *)d_weights64 + 64 * g.gp0, (uint32_t *)(a + off_fields), (uint32_t *)(a + off_st),
                   c->prm, lg_m, (uint32_t *)(a + off_usc), ts_in, (uint32_t *)g.d_ts_out);
        else
            LAUNCH(c, s, "rlc_mix_front", k_rlc_mix_front, n_tr + n_pt, RP_BLOCK, sh, init, n_tr, (const uint8_t *)g.d_proofs, (const uint8_t *)g.d_coms,
                   (const uint8_t *)d_rng64 + 64 * g.gp0, (const uint8_t *)d_weights64 + 64 * g.gp0, (uint32_t *)(a + off_fields), (uint32_t *)(a + off_st),
                   c->prm, lg_m, (uint32_t *)(a + off_usc), d_script, ts_in, (uint32_t *)g.d_ts_out);
        LAUNCH(c, s, "rlc_mix_weigh", k_rlc_mix_weigh, (uint32_t)(nt / 64), 64, mg, sh, c->prm, (const uint8_t *)g.d_proofs, (const uint8_t *)g.d_coms,
               (const uint32_t *)(a + off_st), (const uint32_t *)(a + off_fields), (const uint32_t *)(a + off_usc), (uint32_t *)d_csc, (uint32_t *)d_cpt,
               (uint32_t *)d_gst, (unsigned long long *)d_acc);
    }
    HIPCHK(c, hipMemsetAsync(d_res, 0, 64, s));   // (no group left: R is the identity)
    if (u_total) {
        LAUNCH(c, s, "rlc_mix_reduce", k_rlc_comb_reduce, (uint32_t)((nrows + 63) / 64), 64, (uint32_t)nrows, (const unsigned long long *)d_acc, (uint32_t *)d_gen);
        rc = msm_shared_dev_locked(c, N, M, 1, u_total, d_gen, d_csc, d_cpt, d_res, d_res + 32, nullptr, s);
        if (rc) return rc;
    }
    LAUNCH(c, s, "rlc_mix_verdict", k_rlc_comb_verdict, (n32 + 63) / 64, 64, n32, (const uint32_t *)d_gst, (const uint32_t *)d_res, (const uint8_t *)(d_res + 32),
           d_verdict, d_batch);
    HIPCHK(c, hipGetLastError());
    return BPGPU_OK;
}

// The host form of the mixed-shape combination: every group from its label (labels / label_lens), or -- transcripts != nullptr -- from the
// caller's states (bpgpu_rangeproof_verify_rlc_mixed_ts: transcripts lie group after group, one state where transcript_stride[g] == 0, else
// nbatch[g]; transcripts_out: optional total x 208 bytes).
static int rp_mix_host_call(bpgpu_ctx *c, size_t ngroups, const size_t *n, const size_t *m, const size_t *nbatch, const size_t *proof_len, const uint8_t *proofs,
                            const uint8_t *commitments, const uint8_t *const *labels, const size_t *label_lens, const uint8_t *transcripts,
                            const size_t *transcript_stride, const uint8_t *rng64, const uint8_t *weights64, uint8_t *verdict, uint8_t *batch_out,
                            uint8_t *transcripts_out) {
    const bool ts = transcripts != nullptr;
    const size_t TS = BPGPU_TRANSCRIPT_BYTES;
    size_t total = 0, bytes_p = 0, bytes_c = 0;
    for (size_t g = 0; g < ngroups; g++) {
        if (!ts && label_lens[g] && !labels[g]) return BPGPU_ERR_INVALID_ARG;
        if (nbatch[g] > RM_MAX_TERMS || proof_len[g] > 0xffffffu || m[g] > 0xffffu) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large");
        total += nbatch[g];
        bytes_p += nbatch[g] * proof_len[g];
        bytes_c += nbatch[g] * m[g] * 32;
    }
    if (total == 0) {
        if (batch_out) memset(batch_out, 0, 33);
        return BPGPU_OK;
    }
    if (!verdict || (bytes_p && !proofs) || (bytes_c && !commitments)) return BPGPU_ERR_INVALID_ARG;
    if (total > RM_MAX_TERMS) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large");
    std::lock_guard<std::mutex> lk(c->mu);
    std::vector<rp_mix_group> gr;
    const uint8_t *src_t = transcripts;
    for (size_t g = 0, gp = 0; g < ngroups; g++) {   // (every refusal before the context is entered)
        const size_t nst = ts ? (transcript_stride[g] ? nbatch[g] : 1) : 0;   // (a group without proofs still has its state(s) in the buffer)
        if (ts && transcript_stride[g] != 0 && transcript_stride[g] != TS)
            return fail(c, BPGPU_ERR_INVALID_ARG, "transcript_stride of group %zu neither 0 nor BPGPU_TRANSCRIPT_BYTES", g);
        if (nbatch[g]) {
            rp_mix_group mg{n[g], m[g], nbatch[g], proof_len[g], 0, gp, 0, nullptr, nullptr, ts ? nullptr : labels[g], ts ? 0 : label_lens[g], false};
            if (ts) {
                mg.h_ts = src_t;
                mg.ts_stride = transcript_stride[g];
                mg.u_pos = src_t[200], mg.u_pos_begin = src_t[201], mg.u_flags = src_t[202];
                mg.ts_uniform = true;
                for (size_t b = 0; b < nst; b++) {
                    const uint8_t *st = src_t + b * TS;
                    if (!ts_state_ok(st)) return fail(c, BPGPU_ERR_INVALID_ARG, "malformed transcript state %zu of group %zu", b, g);
                    if (st[200] != src_t[200] || st[201] != src_t[201] || st[202] != src_t[202]) mg.ts_uniform = false;
                }
            }
            const int rcc = rp_mix_classify(c, n[g], m[g], proof_len[g], &mg.k, &mg.whole);
            if (rcc) return rcc;
            gr.push_back(mg);
            gp += nbatch[g];
        }
        src_t += nst * TS;
    }
    HIPCHK(c, hipSetDevice(c->device));
    // staging: per group its proofs and commitments (and its states, where it has one per proof); then every proof's rng bytes and weights;
    // then the outputs
    std::vector<size_t> off(3 * ngroups, 0);
    size_t in = 0;
    for (size_t g = 0; g < ngroups; g++) {
        off[3 * g] = in, in += nbatch[g] ? align_up(nbatch[g] * proof_len[g] + 64) : 0;
        off[3 * g + 1] = in, in += nbatch[g] ? align_up(nbatch[g] * m[g] * 32 + 64) : 0;
        off[3 * g + 2] = in, in += (ts && transcript_stride[g]) ? align_up(nbatch[g] * TS) : 0;
    }
    hipStream_t s = c->stream;
    host_call<bpgpu_ctx> io(c, s);
    const int r_g = io.in(in), r_r = io.in(rng64 ? total * 64 : 0), r_w = io.in(weights64 ? total * 64 : 0);   // (the groups' pieces: off[] inside r_g)
    const int r_v = io.out(total), r_b = io.out(64), r_to = io.out(transcripts_out ? total * TS : 0);
    int rc = io.open();
    if (rc) return rc;
    char *h = io.h(r_g), *d = io.d(r_g);
    const uint8_t *src_p = proofs, *src_c = commitments;
    for (size_t g = 0, gi = 0; g < ngroups; g++) {
        const size_t nb = nbatch[g];
        if (nb == 0) continue;
        memcpy(h + off[3 * g], src_p, nb * proof_len[g]);
        if (m[g]) memcpy(h + off[3 * g + 1], src_c, nb * m[g] * 32);
        src_p += nb * proof_len[g];
        src_c += nb * m[g] * 32;
        gr[gi].d_proofs = d + off[3 * g];
        gr[gi].d_coms = d + off[3 * g + 1];
        if (ts && transcript_stride[g]) {
            memcpy(h + off[3 * g + 2], gr[gi].h_ts, nb * TS);
            gr[gi].d_ts_in = d + off[3 * g + 2];
        }
        if (transcripts_out) gr[gi].d_ts_out = io.d(r_to) + gr[gi].gp0 * TS;
        gi++;
    }
    if (rng64) io.put(r_r, rng64, total * 64);
    if (weights64) io.put(r_w, weights64, total * 64);
    char *d_v = io.d(r_v);
    const char *d_rng_used = nullptr;
    rc = io.upload();
    if (!rc) rc = rp_mix_dev_locked(c, gr, total, rng64 ? io.d(r_r) : nullptr, weights64 ? io.d(r_w) : nullptr, (uint8_t *)d_v, (uint8_t *)io.d(r_b), s, &d_rng_used);
    rc = io.finish(io.download(rc));
    if (rc) return rc;
    // where R is not the identity, or did not decode: every group the combination took again through the per-proof chain of its shape, with
    // the same rng bytes (inputs, and rng bytes drawn above, are still on the device)
    // (the per-proof path writes the same advanced states again: byte for byte those of bpgpu_rangeproof_verify_batch_ts either way)
    return io.deliver_combined(r_v, verdict, total, r_b, batch_out, r_to, transcripts_out, total * TS, [&] {
        for (const auto &g : gr) {
            if (g.whole) continue;
            rp_call a = rp_call_of(g.n, g.m, g.nbatch, g.d_proofs, g.proof_len, g.d_coms, rp_mix_transcripts(g), d_rng_used + 64 * g.gp0, d_v + g.gp0);
            a.s = s;
            const int rcg = rp_verify_chain(c, a);
            if (rcg) return rcg;
        }
        return (int)BPGPU_OK;
    });
}

extern "C" int bpgpu_rangeproof_verify_rlc_mixed(bpgpu_ctx *c, size_t ngroups, const size_t *n, const size_t *m, const size_t *nbatch, const size_t *proof_len,
                                                 const uint8_t *proofs, const uint8_t *commitments, const uint8_t *const *labels, const size_t *label_lens,
                                                 const uint8_t *rng64, const uint8_t *weights64, uint8_t *verdict, uint8_t *batch_out) {
    if (!c || (ngroups && (!n || !m || !nbatch || !proof_len || !labels || !label_lens))) return BPGPU_ERR_INVALID_ARG;
    return rp_mix_host_call(c, ngroups, n, m, nbatch, proof_len, proofs, commitments, labels, label_lens, nullptr, nullptr, rng64, weights64, verdict, batch_out,
                            nullptr);
}

extern "C" int bpgpu_rangeproof_verify_rlc_mixed_ts(bpgpu_ctx *c, size_t ngroups, const size_t *n, const size_t *m, const size_t *nbatch, const size_t *proof_len,
                                                    const uint8_t *proofs, const uint8_t *commitments, const uint8_t *transcripts,
                                                    const size_t *transcript_stride, const uint8_t *rng64, const uint8_t *weights64, uint8_t *verdict,
                                                    uint8_t *batch_out, uint8_t *transcripts_out) {
    if (!c || (ngroups && (!n || !m || !nbatch || !proof_len || !transcripts || !transcript_stride))) return BPGPU_ERR_INVALID_ARG;
    if (!ngroups) {
        if (batch_out) memset(batch_out, 0, 33);
        return BPGPU_OK;
    }
    return rp_mix_host_call(c, ngroups, n, m, nbatch, proof_len, proofs, commitments, nullptr, nullptr, transcripts, transcript_stride, rng64, weights64, verdict,
                            batch_out, transcripts_out);
}

// ---- the one-shape combination on the callers' own transcripts (rp_verify_chain with rlc = true and caller states) -----------------
extern "C" int bpgpu_rangeproof_verify_rlc_ts(bpgpu_ctx *c, size_t n, size_t m, size_t nbatch, const uint8_t *proofs, size_t proof_len, const uint8_t *commitments,
                                              const uint8_t *transcripts, size_t transcript_stride, const uint8_t *rng64, const uint8_t *weights64,
                                              uint8_t *verdict, uint8_t *batch_out, uint8_t *transcripts_out) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    if (!transcripts || (transcript_stride != 0 && transcript_stride != BPGPU_TRANSCRIPT_BYTES))
        return fail(c, BPGPU_ERR_INVALID_ARG, "transcripts missing, or transcript_stride neither 0 nor BPGPU_TRANSCRIPT_BYTES");
    rp_transcripts tr;
    if (!transcript_stride) {
        if (!ts_state_ok(transcripts)) return fail(c, BPGPU_ERR_INVALID_ARG, "malformed transcript state");
        tr.shared_ts = transcripts;
    } else if (nbatch) {   // the states are in host memory: all at one STROBE position -> the per-shape script, as the pool's combining queue decides it
        tr.ts_uniform = true;
        tr.u_pos = transcripts[200], tr.u_pos_begin = transcripts[201], tr.u_flags = transcripts[202];
        for (size_t b = 0; b < nbatch; b++) {
            const uint8_t *st = transcripts + b * BPGPU_TRANSCRIPT_BYTES;
            if (!ts_state_ok(st)) return fail(c, BPGPU_ERR_INVALID_ARG, "malformed transcript state %zu", b);
            if (st[200] != transcripts[200] || st[201] != transcripts[201] || st[202] != transcripts[202]) tr.ts_uniform = false;
        }
    }
    uint8_t bo[33];
    return rp_host_call(c, n, m, nbatch, proofs, proof_len, commitments, tr, transcript_stride ? transcripts : nullptr, rng64, verdict, nullptr, transcripts_out,
                        true, weights64, batch_out ? batch_out : bo);
}

extern "C" int bpgpu_rangeproof_verify_rlc_ts_dev(bpgpu_ctx *c, size_t n, size_t m, size_t nbatch, const void *d_proofs, size_t proof_len,
                                                  const void *d_commitments, const uint8_t *shared_transcript, const void *d_transcripts, const void *d_rng64,
                                                  const void *d_weights64, void *d_verdict, void *d_batch_out, void *d_transcripts_out, void *stream) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    if ((shared_transcript != nullptr) == (d_transcripts != nullptr))
        return fail(c, BPGPU_ERR_INVALID_ARG, "give exactly one of shared_transcript / d_transcripts");
    rp_transcripts tr;
    tr.shared_ts = shared_transcript;
    tr.d_ts_in = d_transcripts;
    tr.d_ts_out = d_transcripts_out;
    rp_call a = rp_call_of(n, m, nbatch, d_proofs, proof_len, d_commitments, tr, d_rng64, d_verdict);
    a.rlc = true;
    a.d_weights64 = d_weights64;
    a.d_batch_out = d_batch_out;
    return rp_dev_call(c, a, stream);
}

namespace {
struct rp_mix_call {
    size_t ngroups;
    const size_t *n, *m, *nbatch, *proof_len;
    const uint8_t *proofs, *commitments;
    const uint8_t *const *labels;
    const size_t *label_lens;
    const uint8_t *rng64, *weights64;
    uint8_t *verdict, *batch_out;
    const uint8_t *transcripts;   // != nullptr: the _ts form (labels unused)
    const size_t *transcript_stride;
    uint8_t *transcripts_out;
};
int rp_mix_call_run(bpgpu_ctx *c, void *arg) {
    const rp_mix_call *a = (const rp_mix_call *)arg;
    if (a->transcripts)
        return bpgpu_rangeproof_verify_rlc_mixed_ts(c, a->ngroups, a->n, a->m, a->nbatch, a->proof_len, a->proofs, a->commitments, a->transcripts,
                                                    a->transcript_stride, a->rng64, a->weights64, a->verdict, a->batch_out, a->transcripts_out);
    return bpgpu_rangeproof_verify_rlc_mixed(c, a->ngroups, a->n, a->m, a->nbatch, a->proof_len, a->proofs, a->commitments, a->labels, a->label_lens, a->rng64,
                                             a->weights64, a->verdict, a->batch_out);
}
}  // namespace

extern "C" int bpgpu_pool_rangeproof_verify_rlc_mixed(bpgpu_pool *pool, size_t ngroups, const size_t *n, const size_t *m, const size_t *nbatch,
                                                      const size_t *proof_len, const uint8_t *proofs, const uint8_t *commitments, const uint8_t *const *labels,
                                                      const size_t *label_lens, const uint8_t *rng64, const uint8_t *weights64, uint8_t *verdict,
                                                      uint8_t *batch_out) {
    if (!pool || (ngroups && (!n || !m || !nbatch || !proof_len || !labels || !label_lens))) return BPGPU_ERR_INVALID_ARG;
    size_t total = 0;
    for (size_t g = 0; g < ngroups; g++) total += nbatch[g];
    if (total == 0) {   // (as the context form: nothing to combine)
        if (batch_out) memset(batch_out, 0, 33);
        return BPGPU_OK;
    }
    rp_mix_call a{ngroups, n, m, nbatch, proof_len, proofs, commitments, labels, label_lens, rng64, weights64, verdict, batch_out, nullptr, nullptr, nullptr};
    return bpgpu_internal_pool_run_on_context(pool, total, verdict, rp_mix_call_run, &a);
}

extern "C" int bpgpu_pool_rangeproof_verify_rlc_mixed_ts(bpgpu_pool *pool, size_t ngroups, const size_t *n, const size_t *m, const size_t *nbatch,
                                                         const size_t *proof_len, const uint8_t *proofs, const uint8_t *commitments, const uint8_t *transcripts,
                                                         const size_t *transcript_stride, const uint8_t *rng64, const uint8_t *weights64, uint8_t *verdict,
                                                         uint8_t *batch_out, uint8_t *transcripts_out) {
    if (!pool || (ngroups && (!n || !m || !nbatch || !proof_len || !transcripts || !transcript_stride))) return BPGPU_ERR_INVALID_ARG;
    size_t total = 0;
    for (size_t g = 0; g < ngroups; g++) total += nbatch[g];
    if (total == 0) {   // (as the context form: nothing to combine)
        if (batch_out) memset(batch_out, 0, 33);
        return BPGPU_OK;
    }
    rp_mix_call a{ngroups, n, m, nbatch, proof_len, proofs, commitments, nullptr, nullptr, rng64, weights64, verdict, batch_out, transcripts, transcript_stride,
                  transcripts_out};
    return bpgpu_internal_pool_run_on_context(pool, total, verdict, rp_mix_call_run, &a);
}

// ============================================================================
// proofs of knowledge of commitment openings (opening.h)
// ============================================================================
// the argument rules every entry point of the family shares; `proof_len` is 0 for the creation
static int opn_check_args(bpgpu_ctx *c, int form, size_t nbatch, size_t proof_len, bool create, const void *values, size_t value_bytes) {
    if (form != BPGPU_OPENING_FULL && form != BPGPU_OPENING_BLINDING) return fail(c, BPGPU_ERR_INVALID_ARG, "form must be BPGPU_OPENING_FULL or BPGPU_OPENING_BLINDING");
    if (!create && proof_len != (form == BPGPU_OPENING_FULL ? 96u : 64u)) return fail(c, BPGPU_ERR_INVALID_ARG, "proof_len must be 96 (form 0) or 64 (form 1)");
    if (values && value_bytes != 8 && value_bytes != 32) return fail(c, BPGPU_ERR_INVALID_ARG, "value_bytes must be 8 (u64) or 32 (scalars)");
    if (create && form == BPGPU_OPENING_FULL && !values) return fail(c, BPGPU_ERR_INVALID_ARG, "values missing");
    if (!create && form == BPGPU_OPENING_FULL && values) return fail(c, BPGPU_ERR_INVALID_ARG, "form 0 has no public value: values must be NULL");
    if (nbatch > OPN_RLC_MAX_PROOFS) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large: at most 2^23 proofs per call");
    return BPGPU_OK;
}
static opn_shape opn_make_shape(int form, size_t nbatch, const void *values, size_t value_bytes, const ipp_ts &ts) {
    opn_shape sh;
    sh.form = (uint32_t)form;
    sh.nproofs = (uint32_t)nbatch;
    sh.value_words = values ? (uint32_t)(value_bytes / 4) : 0u;
    sh.ts_in_stride = ts.stride;
    return sh;
}

// the staging and the k_opn_front launch (lane = proof) of nbatch proofs
static int opn_front_dev_locked(bpgpu_ctx *c, int form, size_t nbatch, const void *d_proofs, const ipp_ts &ts, const void *d_C, const void *d_values,
                                size_t value_bytes, void *d_ts_out, hipStream_t s, front_staged &stg) {
    if (!c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    const int rc = front_stage_locked(c, s, nbatch * 2 * 32 + 64, nbatch * OPN_GEN_ROW * 32 + 64, nbatch * 4, nbatch + 64, nbatch * 32 + 64, stg);
    if (rc) return rc;
    rp_strobe_init init;
    ipp_ts_init(init, ts);
    const opn_shape sh = opn_make_shape(form, nbatch, d_values, value_bytes, ts);
    LAUNCH(c, s, "opn_front", k_opn_front, (sh.nproofs + RP_BLOCK - 1) / RP_BLOCK, RP_BLOCK, sh, init, (const uint32_t *)d_proofs, (const uint32_t *)d_C,
           (const uint32_t *)d_values, (const uint32_t *)ts.d_in, (uint32_t *)stg.d_sc, (uint32_t *)stg.d_pt, (uint32_t *)stg.d_gen, (uint32_t *)stg.d_stat,
           (uint32_t *)d_ts_out);
    return BPGPU_OK;
}

// per proof: the front end, then the shared-generator chain with 2 unique terms per row -- s_r and s_v go through the window tables of
// B_blinding and B (a row of three generator-table scalars: G_0 takes 0), C and R decode in the chain -- then the verdicts
static int opn_verify_dev_locked(bpgpu_ctx *c, int form, size_t nbatch, const void *d_proofs, const ipp_ts &ts, const void *d_C, const void *d_values,
                                 size_t value_bytes, void *d_verdict, void *d_msm_out, void *d_ts_out, hipStream_t s) {
    front_staged stg;
    int rc = opn_front_dev_locked(c, form, nbatch, d_proofs, ts, d_C, d_values, value_bytes, d_ts_out, s, stg);
    if (rc) return rc;
    rc = msm_shared_dev_locked(c, 1, 1, nbatch, 2, stg.d_gen, stg.d_sc, stg.d_pt, stg.d_out, stg.d_mst, nullptr, s, true);
    if (rc) return rc;
    const uint32_t nb32 = (uint32_t)nbatch;
    LAUNCH(c, s, "opn_verdict", k_ipp_verdict, (nb32 + 63) / 64, 64, nb32, (const uint32_t *)stg.d_stat, (const uint8_t *)stg.d_mst, (const uint32_t *)stg.d_out,
           (uint8_t *)d_verdict);
    if (d_msm_out) HIPCHK(c, hipMemcpyAsync(d_msm_out, stg.d_out, nbatch * 32, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipGetLastError());
    return BPGPU_OK;
}

// combined: R = sum_p rho_p Check_p = (sum rho_p s_r) B_blinding + (sum rho_p s_v) B + sum_p (-rho_p c_p) C_p + (-rho_p) R_p: the front end,
// the weights, the weigh launch (U = 2, two shared rows), the reduction into the generator-table row and ONE multiscalar multiplication
// over 2 nbatch points, then the verdicts (undecided where R is not the identity).  Nothing is staged per (proof, generator).
static int opn_rlc_dev_locked(bpgpu_ctx *c, int form, size_t nbatch, const void *d_proofs, const ipp_ts &ts, const void *d_C, const void *d_values,
                              size_t value_bytes, const void *d_weights64, uint8_t *d_verdict, uint8_t *d_batch, void *d_ts_out, hipStream_t s) {
    front_staged stg;
    int rc = opn_front_dev_locked(c, form, nbatch, d_proofs, ts, d_C, d_values, value_bytes, d_ts_out, s, stg);
    if (rc) return rc;
    const size_t nterms = 2 * nbatch;
    comb_layout lay(nterms * 32 + 64, OPN_GEN_ROW * 80, OPN_GEN_ROW * 32 + 64, nbatch * 32);
    rc = lay.reserve(c, &d_batch);
    if (rc) return rc;
    const uint32_t nb32 = (uint32_t)nbatch, nstride = (uint32_t)((nbatch + 63) / 64 * 64);
    rc = comb_begin_locked(c, s, "opn_rlc_rho", lay, nb32, d_weights64, OPN_RLC_WEIGHT_DOMAIN, OPN_GEN_ROW);   // (the row of G_0 stays 0)
    if (rc) return rc;
    LAUNCH(c, s, "opn_rlc_weigh", k_opn_rlc_weigh, 4 * nstride / 64, 64, nb32, nstride, (const uint32_t *)stg.d_stat, (const uint32_t *)lay.d_rho,
           (const uint32_t *)stg.d_gen, (const uint32_t *)stg.d_sc, (const uint32_t *)stg.d_pt, (uint32_t *)lay.d_csc, (uint32_t *)lay.d_cpt,
           (unsigned long long *)lay.d_acc);
    return comb_finish_locked(c, s, "opn_rlc_reduce", "opn_rlc_verdict", lay, stg, OPN_GEN_ROW, 1, 1, true, nterms, nb32, d_verdict, d_batch);
}

// host pointers, both verifiers: rlc = the combined check with its per-proof fallback
static int opn_verify_host_call(bpgpu_ctx *c, int form, size_t nbatch, const uint8_t *proofs, size_t proof_len, const uint8_t *transcripts, size_t transcript_stride,
                                const uint8_t *commitments, const void *values, size_t value_bytes, bool rlc, const uint8_t *weights64, uint8_t *verdict,
                                uint8_t *msm_out, uint8_t *batch_out, uint8_t *transcripts_out) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    int rc = opn_check_args(c, form, nbatch, proof_len, false, values, value_bytes);
    if (rc) return rc;
    if ((rc = ipp_ts_host_args(c, transcripts, transcript_stride, nbatch))) return rc;
    if (nbatch == 0) {
        if (rlc && batch_out) memset(batch_out, 0, 33);
        return BPGPU_OK;
    }
    if (!proofs || !commitments || !verdict) return BPGPU_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t TS = BPGPU_TRANSCRIPT_BYTES, nstates = transcript_stride ? nbatch : 1;
    host_call<bpgpu_ctx> io(c, s);
    const int r_pr = io.in(nbatch * proof_len + 64), r_c = io.in(nbatch * 32 + 64), r_val = io.in(values ? nbatch * value_bytes + 64 : 0), r_ti = io.in(nstates * TS),
              r_w = io.in(weights64 ? nbatch * 64 : 0);
    const int r_v = io.out(nbatch), r_o = io.out(rlc ? 64 : nbatch * 32), r_t = io.out(transcripts_out ? nbatch * TS : 0);
    rc = io.open();
    if (rc) return rc;
    io.put(r_pr, proofs, nbatch * proof_len);
    io.put(r_c, commitments, nbatch * 32);
    if (values) io.put(r_val, values, nbatch * value_bytes);
    io.put(r_ti, transcripts, nstates * TS);
    if (weights64) io.put(r_w, weights64, nbatch * 64);
    const ipp_ts ts = ipp_ts_staged(io.d(r_ti), transcript_stride);
    const void *a_val = values ? io.d(r_val) : nullptr;
    void *a_to = transcripts_out ? io.d(r_t) : nullptr;
    rc = io.upload();
    if (!rc) {
        if (rlc)
            rc = opn_rlc_dev_locked(c, form, nbatch, io.d(r_pr), ts, io.d(r_c), a_val, value_bytes, weights64 ? io.d(r_w) : nullptr, (uint8_t *)io.d(r_v),
                                    (uint8_t *)io.d(r_o), a_to, s);
        else rc = opn_verify_dev_locked(c, form, nbatch, io.d(r_pr), ts, io.d(r_c), a_val, value_bytes, io.d(r_v), io.d(r_o), a_to, s);
    }
    rc = io.finish(io.download(rc));
    if (rc) return rc;
    if (rlc)   // where R is not the identity, or a point of the combined MSM did not decode: the batch again through the per-proof path
        return io.deliver_combined(r_v, verdict, nbatch, r_o, batch_out, r_t, transcripts_out, nbatch * TS, [&] {
            return opn_verify_dev_locked(c, form, nbatch, io.d(r_pr), ts, io.d(r_c), a_val, value_bytes, io.d(r_v), nullptr, nullptr, s);
        });
    if (transcripts_out) memcpy(transcripts_out, io.h(r_t), nbatch * TS);
    if (msm_out) memcpy(msm_out, io.h(r_o), nbatch * 32);
    memcpy(verdict, io.h(r_v), nbatch);
    return BPGPU_OK;
}

extern "C" int bpgpu_opening_verify_batch_ts(bpgpu_ctx *c, int form, size_t nbatch, const uint8_t *proofs, size_t proof_len, const uint8_t *transcripts,
                                             size_t transcript_stride, const uint8_t *commitments, const void *values, size_t value_bytes, uint8_t *verdict,
                                             uint8_t *msm_out, uint8_t *transcripts_out) {
    return opn_verify_host_call(c, form, nbatch, proofs, proof_len, transcripts, transcript_stride, commitments, values, value_bytes, false, nullptr, verdict, msm_out,
                                nullptr, transcripts_out);
}
extern "C" int bpgpu_opening_verify_rlc_ts(bpgpu_ctx *c, int form, size_t nbatch, const uint8_t *proofs, size_t proof_len, const uint8_t *transcripts,
                                           size_t transcript_stride, const uint8_t *commitments, const void *values, size_t value_bytes, const uint8_t *weights64,
                                           uint8_t *verdict, uint8_t *batch_out, uint8_t *transcripts_out) {
    return opn_verify_host_call(c, form, nbatch, proofs, proof_len, transcripts, transcript_stride, commitments, values, value_bytes, true, weights64, verdict, nullptr,
                                batch_out, transcripts_out);
}

// device pointers, both verifiers
static int opn_verify_dev_call(bpgpu_ctx *c, int form, size_t nbatch, const void *d_proofs, size_t proof_len, const uint8_t *shared_transcript,
                               const void *d_transcripts, const void *d_commitments, const void *d_values, size_t value_bytes, bool rlc, const void *d_weights64,
                               void *d_verdict, void *d_out, void *d_transcripts_out, void *stream) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    int rc = opn_check_args(c, form, nbatch, proof_len, false, d_values, value_bytes);
    if (rc) return rc;
    ipp_ts ts;
    if ((rc = ipp_ts_dev_args(c, shared_transcript, d_transcripts, d_transcripts_out, ts))) return rc;
    if (nbatch == 0) return BPGPU_OK;
    if (!d_proofs || !d_commitments || !d_verdict) return BPGPU_ERR_INVALID_ARG;
    if (((uintptr_t)d_proofs | (uintptr_t)d_commitments | (uintptr_t)d_values) & 3) return fail(c, BPGPU_ERR_INVALID_ARG, "device buffers must be 4-byte aligned");
    return dev_call(c, stream, [&](hipStream_t s) {
        if (rlc)
            return opn_rlc_dev_locked(c, form, nbatch, d_proofs, ts, d_commitments, d_values, value_bytes, d_weights64, (uint8_t *)d_verdict, (uint8_t *)d_out,
                                      d_transcripts_out, s);
        return opn_verify_dev_locked(c, form, nbatch, d_proofs, ts, d_commitments, d_values, value_bytes, d_verdict, d_out, d_transcripts_out, s);
    });
}
extern "C" int bpgpu_opening_verify_batch_ts_dev(bpgpu_ctx *c, int form, size_t nbatch, const void *d_proofs, size_t proof_len, const uint8_t *shared_transcript,
                                                 const void *d_transcripts, const void *d_commitments, const void *d_values, size_t value_bytes, void *d_verdict,
                                                 void *d_msm_out, void *d_transcripts_out, void *stream) {
    return opn_verify_dev_call(c, form, nbatch, d_proofs, proof_len, shared_transcript, d_transcripts, d_commitments, d_values, value_bytes, false, nullptr, d_verdict,
                               d_msm_out, d_transcripts_out, stream);
}
extern "C" int bpgpu_opening_verify_rlc_ts_dev(bpgpu_ctx *c, int form, size_t nbatch, const void *d_proofs, size_t proof_len, const uint8_t *shared_transcript,
                                               const void *d_transcripts, const void *d_commitments, const void *d_values, size_t value_bytes,
                                               const void *d_weights64, void *d_verdict, void *d_batch_out, void *d_transcripts_out, void *stream) {
    return opn_verify_dev_call(c, form, nbatch, d_proofs, proof_len, shared_transcript, d_transcripts, d_commitments, d_values, value_bytes, true, d_weights64,
                               d_verdict, d_batch_out, d_transcripts_out, stream);
}

// creation: ONE launch.  v (form 0), r and the seeds come first in the staging: the secret span, cleared on every exit
extern "C" int bpgpu_opening_create_batch_ts(bpgpu_ctx *c, int form, size_t nbatch, const uint8_t *transcripts, size_t transcript_stride, const uint8_t *rng32,
                                             const uint8_t *commitments, const void *values, size_t value_bytes, const uint8_t *blindings, uint8_t *proofs_out,
                                             uint8_t *status, uint8_t *transcripts_out) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    int rc = opn_check_args(c, form, nbatch, 0, true, values, value_bytes);
    if (rc) return rc;
    if ((rc = ipp_ts_host_args(c, transcripts, transcript_stride, nbatch))) return rc;
    if (nbatch == 0) return BPGPU_OK;
    if (!commitments || !blindings || !proofs_out || !status) return BPGPU_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    hipStream_t s = c->stream;
    const size_t TS = BPGPU_TRANSCRIPT_BYTES, nstates = transcript_stride ? nbatch : 1, proof_len = form == BPGPU_OPENING_FULL ? 96 : 64;
    host_call<bpgpu_ctx> io(c, s);
    const int r_bl = io.in(nbatch * 32), r_seed = io.in(nbatch * 32), r_val = io.in(values ? nbatch * value_bytes : 0), r_c = io.in(nbatch * 32),
              r_ti = io.in(nstates * TS);
    const int r_pr = io.out(nbatch * proof_len), r_st = io.out(nbatch), r_t = io.out(transcripts_out ? nbatch * TS : 0);
    io.secrets(io.off[form == BPGPU_OPENING_FULL ? r_c : r_val]);   // blindings, seeds and, where they are secret, the values
    rc = io.open();
    if (rc) return io.finish(rc);
    io.put(r_bl, blindings, nbatch * 32);
    if (rng32) io.put(r_seed, rng32, nbatch * 32);
    else if ((rc = os_random(c, io.h(r_seed), nbatch * 32)) != 0) return io.finish(rc);
    if (values) io.put(r_val, values, nbatch * value_bytes);
    io.put(r_c, commitments, nbatch * 32);
    io.put(r_ti, transcripts, nstates * TS);
    if ((rc = io.upload())) return io.finish(rc);
    do {
        uint32_t *d_ids = nullptr;
        if ((rc = gen_ids_for(c, 1, 1, &d_ids))) break;   // the shared path's list: [0] = B_blinding, [1] = B
        const bool ct = c->prover_ct;
        fb_walk w;
        if ((rc = fb_walk_for(c, ct, w))) break;
        const ipp_ts ts = ipp_ts_staged(io.d(r_ti), transcript_stride);
        const opn_shape sh = opn_make_shape(form, nbatch, values, value_bytes, ts);
        opn_create_in in;
        in.values = values ? (const uint32_t *)io.d(r_val) : nullptr;
        in.blindings = (const uint32_t *)io.d(r_bl);
        in.seeds = (const uint8_t *)io.d(r_seed);
        in.commitments = (const uint32_t *)io.d(r_c);
        in.ts_in = (const uint32_t *)io.d(r_ti);
        const uint32_t grid = (sh.nproofs + BP_BLOCK - 1) / BP_BLOCK;
        uint32_t *d_to = transcripts_out ? (uint32_t *)io.d(r_t) : nullptr;
        LAUNCH_CT(c, s, ct, "opn_create", k_opn_create, grid, BP_BLOCK, sh, in, w.prm, (const uint32_t *)d_ids, w.table, (uint32_t *)io.d(r_pr), (uint8_t *)io.d(r_st),
                  d_to);
        if (hipGetLastError() != hipSuccess) rc = fail(c, BPGPU_ERR_HIP, "launch failed");
    } while (0);
    rc = io.finish(io.download(rc));
    if (rc) return rc;
    memcpy(proofs_out, io.h(r_pr), nbatch * proof_len);
    memcpy(status, io.h(r_st), nbatch);
    if (transcripts_out) memcpy(transcripts_out, io.h(r_t), nbatch * TS);
    return BPGPU_OK;
}

// ============================================================================
// rewinding range proofs (rewind.h): one launch, lane = row
// ============================================================================
// the argument rules the two entry points share: n, and the one length a proof of (n, 1) has
static int rwd_check_args(bpgpu_ctx *c, size_t n, size_t nbatch, size_t proof_len, rwd_shape &sh) {
    int rc = rpp_check_nm(c, n, 1);
    if (rc) return rc;
    size_t k = 0;
    while (((size_t)1 << k) < n) k++;
    if (proof_len != 32 * (9 + 2 * k)) return fail(c, BPGPU_ERR_INVALID_ARG, "proof_len must be 32 * (9 + 2 lg n) = %zu", 32 * (9 + 2 * k));
    if (nbatch > RWD_MAX_BATCH) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large: at most 2^26 rows per call");
    sh.n = (uint32_t)n;
    sh.k = (uint32_t)k;
    sh.nproofs = (uint32_t)nbatch;
    sh.proof_words = (uint32_t)(proof_len / 4);
    sh.ts_in_stride = 0;
    return BPGPU_OK;
}
// enqueue the launch on s; constant-time under the context option "prover_constant_time" (its own small-window table, built on first use)
static int rwd_launch_locked(bpgpu_ctx *c, hipStream_t s, const rwd_shape &sh, const rwd_in &in, const rwd_out &out) {
    uint32_t *d_ids = nullptr;
    int rc = gen_ids_for(c, 1, 1, &d_ids);   // the shared path's list: [0] = B_blinding, [1] = B
    if (rc) return rc;
    const bool ct = c->prover_ct;
    fb_walk w;
    if ((rc = fb_walk_for(c, ct, w))) return rc;
    const uint32_t grid = (sh.nproofs + BP_BLOCK - 1) / BP_BLOCK;
    LAUNCH_CT(c, s, ct, "rewind", k_rewind, grid, BP_BLOCK, sh, in, out, w.prm, (const uint32_t *)d_ids, w.table);
    if (hipGetLastError() != hipSuccess) return fail(c, BPGPU_ERR_HIP, "launch failed");
    return BPGPU_OK;
}

// the seeds lead the staged inputs and value, message and blinding lead the outputs: the secret spans, cleared on every exit
extern "C" int bpgpu_rangeproof_rewind_batch(bpgpu_ctx *c, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len, const uint8_t *commitments,
                                             const uint8_t *transcripts, size_t transcript_stride, const uint8_t *rng32, uint8_t *status_out,
                                             uint64_t *values_out, uint8_t *messages_out, uint8_t *blindings_out) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    rwd_shape sh;
    int rc = rwd_check_args(c, n, nbatch, proof_len, sh);
    if (rc) return rc;
    if ((rc = ipp_ts_host_args(c, transcripts, transcript_stride, nbatch))) return rc;
    if (nbatch == 0) return BPGPU_OK;
    if (!proofs || !commitments || !rng32 || !status_out || !values_out || !messages_out || !blindings_out) return BPGPU_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    hipStream_t s = c->stream;
    const size_t TS = BPGPU_TRANSCRIPT_BYTES, nstates = transcript_stride ? nbatch : 1;
    host_call<bpgpu_ctx> io(c, s);
    const int r_seed = io.in(nbatch * 32), r_pr = io.in(nbatch * proof_len), r_c = io.in(nbatch * 32), r_ti = io.in(nstates * TS);
    const int r_v = io.out(nbatch * 8), r_m = io.out(nbatch * 16), r_g = io.out(nbatch * 32), r_st = io.out(nbatch);
    io.secrets(io.off[r_pr]);   // the seeds
    rc = io.open();
    if (rc) return io.finish(rc);
    io.put(r_seed, rng32, nbatch * 32);
    io.put(r_pr, proofs, nbatch * proof_len);
    io.put(r_c, commitments, nbatch * 32);
    io.put(r_ti, transcripts, nstates * TS);
    if (!(rc = io.upload())) {
        sh.ts_in_stride = transcript_stride ? BP_TS_WORDS : 0;
        const rwd_in in = {(const uint32_t *)io.d(r_pr), (const uint32_t *)io.d(r_c), (const uint8_t *)io.d(r_seed), (const uint32_t *)io.d(r_ti)};
        const rwd_out out = {(uint8_t *)io.d(r_st), (uint32_t *)io.d(r_v), (uint32_t *)io.d(r_m), (uint32_t *)io.d(r_g)};
        rc = rwd_launch_locked(c, s, sh, in, out);
    }
    rc = io.finish(io.download(rc));
    // the staged copies of value, message and blinding are secrets too: handed over, then cleared (the output span up to the status)
    if (!rc) {
        memcpy(values_out, io.h(r_v), nbatch * 8);
        memcpy(messages_out, io.h(r_m), nbatch * 16);
        memcpy(blindings_out, io.h(r_g), nbatch * 32);
        memcpy(status_out, io.h(r_st), nbatch);
    }
    if (io.hb) {
        memset(io.h(r_v), 0, io.off[r_st] - io.off[r_v]);
        if (io.hb == c->io.pin) c->io.last_secret_bytes = io.off[r_st];
    }
    return rc;
}

// device pointers: nothing is staged, nothing is read back; the caller's buffers are the caller's
extern "C" int bpgpu_rangeproof_rewind_batch_dev(bpgpu_ctx *c, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len, const void *d_commitments,
                                                 const void *d_transcripts, size_t transcript_stride, const void *d_rng32, void *d_status_out,
                                                 void *d_values_out, void *d_messages_out, void *d_blindings_out, void *stream) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    rwd_shape sh;
    int rc = rwd_check_args(c, n, nbatch, proof_len, sh);
    if (rc) return rc;
    if (transcript_stride != 0 && transcript_stride != BPGPU_TRANSCRIPT_BYTES)
        return fail(c, BPGPU_ERR_INVALID_ARG, "transcript_stride must be 0 or %d", BPGPU_TRANSCRIPT_BYTES);
    if (nbatch == 0) return BPGPU_OK;
    if (!d_proofs || !d_commitments || !d_rng32 || !d_status_out || !d_values_out || !d_messages_out || !d_blindings_out) return BPGPU_ERR_INVALID_ARG;
    if (!d_transcripts) return fail(c, BPGPU_ERR_INVALID_ARG, "transcripts missing");
    if (((uintptr_t)d_values_out & 7) ||
        (((uintptr_t)d_proofs | (uintptr_t)d_commitments | (uintptr_t)d_transcripts | (uintptr_t)d_rng32 | (uintptr_t)d_messages_out | (uintptr_t)d_blindings_out) & 3))
        return fail(c, BPGPU_ERR_INVALID_ARG, "device buffers must be 4-byte aligned (values: 8-byte)");
    sh.ts_in_stride = transcript_stride ? BP_TS_WORDS : 0;
    const rwd_in in = {(const uint32_t *)d_proofs, (const uint32_t *)d_commitments, (const uint8_t *)d_rng32, (const uint32_t *)d_transcripts};
    const rwd_out out = {(uint8_t *)d_status_out, (uint32_t *)d_values_out, (uint32_t *)d_messages_out, (uint32_t *)d_blindings_out};
    return dev_call(
        c, stream, [&] { return c->d_table ? BPGPU_OK : fail(c, BPGPU_ERR_NO_GENS, "generators not loaded"); },
        [&](hipStream_t s) { return rwd_launch_locked(c, s, sh, in, out); });
}

// ============================================================================
// scanning range proofs under many keys (scan.h): prefixes, one replay per row, candidates per (row, key), open
// ============================================================================
static int scn_check_args(bpgpu_ctx *c, size_t n, size_t nbatch, size_t proof_len, size_t nkeys, rwd_shape &sh) {
    int rc = rwd_check_args(c, n, nbatch, proof_len, sh);
    if (rc) return rc;
    if (nkeys < 1 || nkeys > SCN_MAX_KEYS) return fail(c, BPGPU_ERR_INVALID_ARG, "nkeys must be 1 .. 1024");
    if (nbatch * nkeys > SCN_MAX_CANDIDATES) return fail(c, BPGPU_ERR_INVALID_ARG, "scan too large: at most 2^28 (row, key) candidates per call");
    return BPGPU_OK;
}
// Enqueue the four launches on s.  The working set (key prefixes, x and z, the survivors, the derived seeds: secrets) lies in the arena,
// which the caller clears on the stream behind the last launch.
static int scn_launch_locked(bpgpu_ctx *c, hipStream_t s, const rwd_shape &sh, const rwd_in &in, const uint32_t *d_keys, uint32_t nkeys, const rwd_out &out,
                             uint32_t *d_key_index, size_t *ws_bytes = nullptr) {
    uint32_t *d_ids = nullptr;
    int rc = gen_ids_for(c, 1, 1, &d_ids);   // [0] = B_blinding, [1] = B
    if (rc) return rc;
    const bool ct = c->prover_ct;
    fb_walk w;
    if ((rc = fb_walk_for(c, ct, w))) return rc;
    const size_t nb = sh.nproofs;
    arena_plan ap;
    const size_t off_pre = ap.add((size_t)nkeys * BP_TS_WORDS * 4), off_base = ap.add(BP_TS_WORDS * 4), off_st = ap.add(nb * 4), off_xz = ap.add(nb * 64),
                 off_j = ap.add(nb * 4), off_seed = ap.add(nb * 32);
    if ((rc = arena_reserve(c, ap.total))) return rc;
    if (ws_bytes) *ws_bytes = ap.total;
    char *b = c->arena;
    const scn_ws ws = {(uint32_t *)(b + off_pre), (uint32_t *)(b + off_base), (uint32_t *)(b + off_st), (uint32_t *)(b + off_xz), (uint32_t *)(b + off_j),
                       (uint32_t *)(b + off_seed)};
    const scn_keys keys = {d_keys, nkeys};
    const uint32_t grid = (sh.nproofs + BP_BLOCK - 1) / BP_BLOCK;
    LAUNCH(c, s, "scan_prefix", k_scan_prefix, (nkeys + BP_BLOCK - 1) / BP_BLOCK, BP_BLOCK, keys, ws);
    LAUNCH(c, s, "scan_replay", k_scan_replay, grid, BP_BLOCK, sh, in, ws);
    LAUNCH_CT(c, s, ct, "scan_cand", k_scan_cand, dim3(grid, nkeys), BP_BLOCK, sh, in, ws);
    LAUNCH_CT(c, s, ct, "scan_open", k_scan_open, grid, BP_BLOCK, sh, in, keys, ws, out, d_key_index, w.prm, (const uint32_t *)d_ids, w.table);
    if (hipGetLastError() != hipSuccess) return fail(c, BPGPU_ERR_HIP, "launch failed");
    return BPGPU_OK;
}

// the keys lead the staged inputs and value, message, blinding and key index lead the outputs: the secret spans, cleared on every exit
extern "C" int bpgpu_rangeproof_scan_batch(bpgpu_ctx *c, size_t n, size_t nbatch, const uint8_t *proofs, size_t proof_len, const uint8_t *commitments,
                                           const uint8_t *transcripts, size_t transcript_stride, const uint8_t *keys32, size_t nkeys, uint8_t *status_out,
                                           uint32_t *key_index_out, uint64_t *values_out, uint8_t *messages_out, uint8_t *blindings_out) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    rwd_shape sh;
    int rc = scn_check_args(c, n, nbatch, proof_len, nkeys, sh);
    if (rc) return rc;
    if ((rc = ipp_ts_host_args(c, transcripts, transcript_stride, nbatch))) return rc;
    if (nbatch == 0) return BPGPU_OK;
    if (!keys32) return fail(c, BPGPU_ERR_INVALID_ARG, "keys32 missing");
    if (!proofs || !commitments || !status_out || !key_index_out || !values_out || !messages_out || !blindings_out) return BPGPU_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    hipStream_t s = c->stream;
    const size_t TS = BPGPU_TRANSCRIPT_BYTES, nstates = transcript_stride ? nbatch : 1;
    host_call<bpgpu_ctx> io(c, s);
    const int r_key = io.in(nkeys * 32), r_pr = io.in(nbatch * proof_len), r_c = io.in(nbatch * 32), r_ti = io.in(nstates * TS);
    const int r_v = io.out(nbatch * 8), r_m = io.out(nbatch * 16), r_g = io.out(nbatch * 32), r_k = io.out(nbatch * 4), r_st = io.out(nbatch);
    io.secrets(io.off[r_pr]);   // the keys
    rc = io.open();
    if (rc) return io.finish(rc);
    io.put(r_key, keys32, nkeys * 32);
    io.put(r_pr, proofs, nbatch * proof_len);
    io.put(r_c, commitments, nbatch * 32);
    io.put(r_ti, transcripts, nstates * TS);
    if (!(rc = io.upload())) {
        sh.ts_in_stride = transcript_stride ? BP_TS_WORDS : 0;
        const rwd_in in = {(const uint32_t *)io.d(r_pr), (const uint32_t *)io.d(r_c), nullptr, (const uint32_t *)io.d(r_ti)};
        const rwd_out out = {(uint8_t *)io.d(r_st), (uint32_t *)io.d(r_v), (uint32_t *)io.d(r_m), (uint32_t *)io.d(r_g)};
        rc = scn_launch_locked(c, s, sh, in, (const uint32_t *)io.d(r_key), (uint32_t)nkeys, out, (uint32_t *)io.d(r_k));
    }
    rc = io.finish(io.download(rc));
    // the staged copies of value, message, blinding and key index are secrets too: handed over, then cleared (the output span up to the status)
    if (!rc) {
        memcpy(values_out, io.h(r_v), nbatch * 8);
        memcpy(messages_out, io.h(r_m), nbatch * 16);
        memcpy(blindings_out, io.h(r_g), nbatch * 32);
        memcpy(key_index_out, io.h(r_k), nbatch * 4);
        memcpy(status_out, io.h(r_st), nbatch);
    }
    if (io.hb) {
        memset(io.h(r_v), 0, io.off[r_st] - io.off[r_v]);
        if (io.hb == c->io.pin) c->io.last_secret_bytes = io.off[r_st];
    }
    return rc;
}

// device pointers: nothing is staged, nothing is read back; the working set is cleared on the stream behind the open
extern "C" int bpgpu_rangeproof_scan_batch_dev(bpgpu_ctx *c, size_t n, size_t nbatch, const void *d_proofs, size_t proof_len, const void *d_commitments,
                                               const void *d_transcripts, size_t transcript_stride, const void *d_keys32, size_t nkeys, void *d_status_out,
                                               void *d_key_index_out, void *d_values_out, void *d_messages_out, void *d_blindings_out, void *stream) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    rwd_shape sh;
    int rc = scn_check_args(c, n, nbatch, proof_len, nkeys, sh);
    if (rc) return rc;
    if (transcript_stride != 0 && transcript_stride != BPGPU_TRANSCRIPT_BYTES)
        return fail(c, BPGPU_ERR_INVALID_ARG, "transcript_stride must be 0 or %d", BPGPU_TRANSCRIPT_BYTES);
    if (nbatch == 0) return BPGPU_OK;
    if (!d_keys32) return fail(c, BPGPU_ERR_INVALID_ARG, "keys32 missing");
    if (!d_proofs || !d_commitments || !d_status_out || !d_key_index_out || !d_values_out || !d_messages_out || !d_blindings_out) return BPGPU_ERR_INVALID_ARG;
    if (!d_transcripts) return fail(c, BPGPU_ERR_INVALID_ARG, "transcripts missing");
    if (((uintptr_t)d_values_out & 7) || (((uintptr_t)d_proofs | (uintptr_t)d_commitments | (uintptr_t)d_transcripts | (uintptr_t)d_keys32 | (uintptr_t)d_key_index_out |
                                           (uintptr_t)d_messages_out | (uintptr_t)d_blindings_out) & 3))
        return fail(c, BPGPU_ERR_INVALID_ARG, "device buffers must be 4-byte aligned (values: 8-byte)");
    dev_scope<bpgpu_ctx> sc(c);
    if (sc.rc) return sc.rc;
    if (!c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    if ((rc = sc.enter(stream))) return rc;
    hipStream_t s = sc.s;
    sh.ts_in_stride = transcript_stride ? BP_TS_WORDS : 0;
    const rwd_in in = {(const uint32_t *)d_proofs, (const uint32_t *)d_commitments, nullptr, (const uint32_t *)d_transcripts};
    const rwd_out out = {(uint8_t *)d_status_out, (uint32_t *)d_values_out, (uint32_t *)d_messages_out, (uint32_t *)d_blindings_out};
    size_t ws_bytes = 0;   // (what this call laid out in the arena: all that it wrote there)
    rc = scn_launch_locked(c, s, sh, in, (const uint32_t *)d_keys32, (uint32_t)nkeys, out, (uint32_t *)d_key_index_out, &ws_bytes);
    const bool ok = !ws_bytes || hipMemsetAsync(c->arena, 0, ws_bytes, s) == hipSuccess;
    const int rc2 = sc.leave();
    if (!rc && !ok) rc = fail(c, BPGPU_ERR_HIP, "clearing the scan's working set failed");
    return rc ? rc : rc2;
}

// ============================================================================
// proofs of recorded linear relations between points (sigma.h)
// ============================================================================
struct bpgpu_sigma_relation {
    bpgpu_ctx *ctx = nullptr;   // (compared, never followed, by destroy: the context may be gone by then)
    uint64_t ctx_serial = 0;    // a later context at the same address is another context
    int device = 0;
    sig_rel h{};
    sig_rel *d = nullptr;       // the record on the context's device
};

static int sig_parse(bpgpu_ctx *c, const uint8_t *desc, size_t desc_len, size_t gens_capacity, sig_rel &r) {
    const char *why = sig_rel_parse(desc, desc_len, gens_capacity, r);
    return why ? fail(c, BPGPU_ERR_INVALID_ARG, "%s", why) : BPGPU_OK;
}
extern "C" int bpgpu_sigma_descriptor_check(const uint8_t *desc, size_t desc_len, size_t gens_capacity, uint8_t digest[32]) {
    sig_rel r;
    const int rc = sig_parse(nullptr, desc, desc_len, gens_capacity, r);
    if (!rc && digest) memcpy(digest, r.digest, 32);
    return rc;
}
extern "C" int bpgpu_sigma_relation_create(bpgpu_ctx *c, const uint8_t *desc, size_t desc_len, bpgpu_sigma_relation **out) {
    if (!c || !out) return BPGPU_ERR_INVALID_ARG;
    *out = nullptr;
    std::lock_guard<std::mutex> lk(c->mu);
    sig_rel r;
    const int rcp = sig_parse(c, desc, desc_len, c->gens_capacity, r);
    if (rcp) return rcp;
    HIPCHK(c, hipSetDevice(c->device));
    sig_rel *d = nullptr;
    if (hipMalloc((void **)&d, sizeof r) != hipSuccess) return fail(c, BPGPU_ERR_HIP, "out of device memory");
    if (hipMemcpy(d, &r, sizeof r, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        return fail(c, BPGPU_ERR_HIP, "copying the relation failed");
    }
    bpgpu_sigma_relation *rel = new bpgpu_sigma_relation;
    rel->ctx = c;
    rel->ctx_serial = c->serial;
    rel->device = c->device;
    rel->h = r;
    rel->d = d;
    *out = rel;
    return BPGPU_OK;
}
extern "C" void bpgpu_sigma_relation_destroy(bpgpu_sigma_relation *rel) {
    if (!rel) return;
    if (rel->d) {
        (void)hipSetDevice(rel->device);
        (void)hipDeviceSynchronize();   // a _dev call may still be reading the record on a caller's stream
        (void)hipFree(rel->d);
    }
    delete rel;
}
extern "C" int bpgpu_sigma_relation_shape(const bpgpu_sigma_relation *rel, size_t *S, size_t *P, size_t *E, uint8_t digest[32]) {
    if (!rel) return BPGPU_ERR_INVALID_ARG;
    if (S) *S = rel->h.S;
    if (P) *P = rel->h.P;
    if (E) *E = rel->h.E;
    if (digest) memcpy(digest, rel->h.digest, 32);
    return BPGPU_OK;
}

// the argument rules every entry point of the family shares; `proof_len` is 0 for the creation
static int sig_check_args(bpgpu_ctx *c, const bpgpu_sigma_relation *rel, size_t nbatch, size_t proof_len, bool create) {
    if (!rel || rel->ctx != c || rel->ctx_serial != c->serial) return fail(c, BPGPU_ERR_INVALID_ARG, "the relation is missing or was recorded on another context");
    const size_t want = 32 * (size_t)(rel->h.E + rel->h.S);
    if (!create && proof_len != want) return fail(c, BPGPU_ERR_INVALID_ARG, "proof_len must be 32 (E + S) = %zu", want);
    if (nbatch * (rel->h.P + rel->h.E) > SIG_RLC_MAX_TERMS) return fail(c, BPGPU_ERR_INVALID_ARG, "batch too large: at most 2^24 / (P + E) proofs per call");
    return BPGPU_OK;
}
// (under the lock) the generators may have been replaced since the relation was recorded
static int sig_check_gens_locked(bpgpu_ctx *c, const bpgpu_sigma_relation *rel) {
    if (!c->d_table) return fail(c, BPGPU_ERR_NO_GENS, "generators not loaded");
    if (rel->h.G > c->gens_capacity) return fail(c, BPGPU_ERR_NO_GENS, "the relation uses G_%u: beyond the loaded generators", rel->h.G - 1);
    return BPGPU_OK;
}

// the staging and the k_sig_front launch (lane = proof) of nbatch proofs: nbatch E rows of P + 1 unique terms and 2 + G generator columns
static int sig_front_dev_locked(bpgpu_ctx *c, const bpgpu_sigma_relation *rel, size_t nbatch, const void *d_proofs, const ipp_ts &ts, const void *d_points,
                                void *d_ts_out, hipStream_t s, front_staged &stg) {
    int rc = sig_check_gens_locked(c, rel);
    if (rc) return rc;
    const size_t rows = nbatch * rel->h.E, U = sig_uniq(rel->h), GR = sig_gen_row(rel->h);
    rc = front_stage_locked(c, s, rows * U * 32 + 64, rows * GR * 32 + 64, nbatch * 4, rows + 64, rows * 32 + 64, stg);
    if (rc) return rc;
    rp_strobe_init init;
    ipp_ts_init(init, ts);
    const uint32_t nb32 = (uint32_t)nbatch;
    LAUNCH(c, s, "sig_front", k_sig_front, (nb32 + RP_BLOCK - 1) / RP_BLOCK, RP_BLOCK, (const sig_rel *)rel->d, nb32, init, (const uint32_t *)d_proofs,
           (const uint32_t *)d_points, (const uint32_t *)ts.d_in, ts.stride, (uint32_t *)stg.d_sc, (uint32_t *)stg.d_pt, (uint32_t *)stg.d_gen,
           (uint32_t *)stg.d_stat, (uint32_t *)d_ts_out);
    return BPGPU_OK;
}

// per proof: the front end, then the shared-generator chain with one row per (proof, equation), then the verdicts
static int sig_verify_dev_locked(bpgpu_ctx *c, const bpgpu_sigma_relation *rel, size_t nbatch, const void *d_proofs, const ipp_ts &ts, const void *d_points,
                                 void *d_verdict, void *d_msm_out, void *d_ts_out, hipStream_t s) {
    front_staged stg;
    int rc = sig_front_dev_locked(c, rel, nbatch, d_proofs, ts, d_points, d_ts_out, s, stg);
    if (rc) return rc;
    const size_t rows = nbatch * rel->h.E;
    rc = msm_shared_dev_locked(c, rel->h.G, 1, rows, sig_uniq(rel->h), stg.d_gen, stg.d_sc, stg.d_pt, stg.d_out, stg.d_mst, nullptr, s, true);
    if (rc) return rc;
    const uint32_t nb32 = (uint32_t)nbatch;
    LAUNCH(c, s, "sig_verdict", k_sig_verdict, (nb32 + 63) / 64, 64, nb32, rel->h.E, (const uint32_t *)stg.d_stat, (const uint8_t *)stg.d_mst,
           (const uint32_t *)stg.d_out, (uint8_t *)d_verdict);
    if (d_msm_out) HIPCHK(c, hipMemcpyAsync(d_msm_out, stg.d_out, rows * 32, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipGetLastError());
    return BPGPU_OK;
}

// combined: R = sum_{p,k} rho_{p,k} Check_{p,k}: the front end, one weight per (proof, equation), the weigh launch (P + E unique terms per
// proof, 2 + G shared rows), the reduction into the generator-table row and ONE multiscalar multiplication over nbatch (P + E) points,
// then the verdicts (undecided where R is not the identity)
static int sig_rlc_dev_locked(bpgpu_ctx *c, const bpgpu_sigma_relation *rel, size_t nbatch, const void *d_proofs, const ipp_ts &ts, const void *d_points,
                              const void *d_weights64, uint8_t *d_verdict, uint8_t *d_batch, void *d_ts_out, hipStream_t s) {
    front_staged stg;
    int rc = sig_front_dev_locked(c, rel, nbatch, d_proofs, ts, d_points, d_ts_out, s, stg);
    if (rc) return rc;
    const size_t NU = rel->h.P + rel->h.E, GR = sig_gen_row(rel->h), nterms = NU * nbatch, nrho = nbatch * rel->h.E;
    comb_layout lay(nterms * 32 + 64, GR * 80, GR * 32 + 64, nrho * 32);
    rc = lay.reserve(c, &d_batch);
    if (rc) return rc;
    const uint32_t nb32 = (uint32_t)nbatch, nstride = (uint32_t)((nbatch + 63) / 64 * 64);
    rc = comb_begin_locked(c, s, "sig_rlc_rho", lay, (uint32_t)nrho, d_weights64, SIG_RLC_WEIGHT_DOMAIN, GR);
    if (rc) return rc;
    LAUNCH(c, s, "sig_rlc_weigh", k_sig_rlc_weigh, (uint32_t)((NU + GR) * nstride / 64), 64, (const sig_rel *)rel->d, nb32, nstride, (const uint32_t *)stg.d_stat,
           (const uint32_t *)lay.d_rho, (const uint32_t *)stg.d_gen, (const uint32_t *)stg.d_sc, (const uint32_t *)stg.d_pt, (const uint32_t *)d_points,
           (uint32_t *)lay.d_csc, (uint32_t *)lay.d_cpt, (unsigned long long *)lay.d_acc);
    // (GR <= 10: the reduce is one workgroup)
    return comb_finish_locked(c, s, "sig_rlc_reduce", "sig_rlc_verdict", lay, stg, GR, rel->h.G, 1, true, nterms, nb32, d_verdict, d_batch);
}

// host pointers, both verifiers: rlc = the combined check with its per-proof fallback
static int sig_verify_host_call(bpgpu_ctx *c, const bpgpu_sigma_relation *rel, size_t nbatch, const uint8_t *proofs, size_t proof_len, const uint8_t *transcripts,
                                size_t transcript_stride, const uint8_t *points, bool rlc, const uint8_t *weights64, uint8_t *verdict, uint8_t *msm_out,
                                uint8_t *batch_out, uint8_t *transcripts_out) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    int rc = sig_check_args(c, rel, nbatch, proof_len, false);
    if (rc) return rc;
    if ((rc = ipp_ts_host_args(c, transcripts, transcript_stride, nbatch))) return rc;
    if (nbatch == 0) {
        if (rlc && batch_out) memset(batch_out, 0, 33);
        return BPGPU_OK;
    }
    if (!proofs || !points || !verdict) return BPGPU_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t TS = BPGPU_TRANSCRIPT_BYTES, nstates = transcript_stride ? nbatch : 1, P = rel->h.P, E = rel->h.E;
    host_call<bpgpu_ctx> io(c, s);
    const int r_pr = io.in(nbatch * proof_len + 64), r_p = io.in(nbatch * P * 32 + 64), r_ti = io.in(nstates * TS), r_w = io.in(weights64 ? nbatch * E * 64 : 0);
    const int r_v = io.out(nbatch), r_o = io.out(rlc ? 64 : nbatch * E * 32), r_t = io.out(transcripts_out ? nbatch * TS : 0);
    rc = io.open();
    if (rc) return rc;
    io.put(r_pr, proofs, nbatch * proof_len);
    io.put(r_p, points, nbatch * P * 32);
    io.put(r_ti, transcripts, nstates * TS);
    if (weights64) io.put(r_w, weights64, nbatch * E * 64);
    const ipp_ts ts = ipp_ts_staged(io.d(r_ti), transcript_stride);
    void *a_to = transcripts_out ? io.d(r_t) : nullptr;
    rc = io.upload();
    if (!rc) {
        if (rlc)
            rc = sig_rlc_dev_locked(c, rel, nbatch, io.d(r_pr), ts, io.d(r_p), weights64 ? io.d(r_w) : nullptr, (uint8_t *)io.d(r_v), (uint8_t *)io.d(r_o), a_to, s);
        else rc = sig_verify_dev_locked(c, rel, nbatch, io.d(r_pr), ts, io.d(r_p), io.d(r_v), io.d(r_o), a_to, s);
    }
    rc = io.finish(io.download(rc));
    if (rc) return rc;
    if (rlc)   // where R is not the identity, or a point of the combined MSM did not decode: the batch again through the per-proof path
        return io.deliver_combined(r_v, verdict, nbatch, r_o, batch_out, r_t, transcripts_out, nbatch * TS,
                                   [&] { return sig_verify_dev_locked(c, rel, nbatch, io.d(r_pr), ts, io.d(r_p), io.d(r_v), nullptr, nullptr, s); });
    if (transcripts_out) memcpy(transcripts_out, io.h(r_t), nbatch * TS);
    if (msm_out) memcpy(msm_out, io.h(r_o), nbatch * E * 32);
    memcpy(verdict, io.h(r_v), nbatch);
    return BPGPU_OK;
}

extern "C" int bpgpu_sigma_verify_batch_ts(bpgpu_ctx *c, const bpgpu_sigma_relation *rel, size_t nbatch, const uint8_t *proofs, size_t proof_len,
                                           const uint8_t *transcripts, size_t transcript_stride, const uint8_t *points, uint8_t *verdict, uint8_t *msm_out,
                                           uint8_t *transcripts_out) {
    return sig_verify_host_call(c, rel, nbatch, proofs, proof_len, transcripts, transcript_stride, points, false, nullptr, verdict, msm_out, nullptr, transcripts_out);
}
extern "C" int bpgpu_sigma_verify_rlc_ts(bpgpu_ctx *c, const bpgpu_sigma_relation *rel, size_t nbatch, const uint8_t *proofs, size_t proof_len,
                                         const uint8_t *transcripts, size_t transcript_stride, const uint8_t *points, const uint8_t *weights64, uint8_t *verdict,
                                         uint8_t *batch_out, uint8_t *transcripts_out) {
    return sig_verify_host_call(c, rel, nbatch, proofs, proof_len, transcripts, transcript_stride, points, true, weights64, verdict, nullptr, batch_out, transcripts_out);
}

// device pointers, both verifiers
static int sig_verify_dev_call(bpgpu_ctx *c, const bpgpu_sigma_relation *rel, size_t nbatch, const void *d_proofs, size_t proof_len, const uint8_t *shared_transcript,
                               const void *d_transcripts, const void *d_points, bool rlc, const void *d_weights64, void *d_verdict, void *d_out,
                               void *d_transcripts_out, void *stream) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    int rc = sig_check_args(c, rel, nbatch, proof_len, false);
    if (rc) return rc;
    ipp_ts ts;
    if ((rc = ipp_ts_dev_args(c, shared_transcript, d_transcripts, d_transcripts_out, ts))) return rc;
    if (nbatch == 0) return BPGPU_OK;
    if (!d_proofs || !d_points || !d_verdict) return BPGPU_ERR_INVALID_ARG;
    if (((uintptr_t)d_proofs | (uintptr_t)d_points) & 3) return fail(c, BPGPU_ERR_INVALID_ARG, "device buffers must be 4-byte aligned");
    return dev_call(c, stream, [&](hipStream_t s) {
        if (rlc) return sig_rlc_dev_locked(c, rel, nbatch, d_proofs, ts, d_points, d_weights64, (uint8_t *)d_verdict, (uint8_t *)d_out, d_transcripts_out, s);
        return sig_verify_dev_locked(c, rel, nbatch, d_proofs, ts, d_points, d_verdict, d_out, d_transcripts_out, s);
    });
}
extern "C" int bpgpu_sigma_verify_batch_ts_dev(bpgpu_ctx *c, const bpgpu_sigma_relation *rel, size_t nbatch, const void *d_proofs, size_t proof_len,
                                               const uint8_t *shared_transcript, const void *d_transcripts, const void *d_points, void *d_verdict,
                                               void *d_msm_out, void *d_transcripts_out, void *stream) {
    return sig_verify_dev_call(c, rel, nbatch, d_proofs, proof_len, shared_transcript, d_transcripts, d_points, false, nullptr, d_verdict, d_msm_out,
                               d_transcripts_out, stream);
}
extern "C" int bpgpu_sigma_verify_rlc_ts_dev(bpgpu_ctx *c, const bpgpu_sigma_relation *rel, size_t nbatch, const void *d_proofs, size_t proof_len,
                                             const uint8_t *shared_transcript, const void *d_transcripts, const void *d_points, const void *d_weights64,
                                             void *d_verdict, void *d_batch_out, void *d_transcripts_out, void *stream) {
    return sig_verify_dev_call(c, rel, nbatch, d_proofs, proof_len, shared_transcript, d_transcripts, d_points, true, d_weights64, d_verdict, d_batch_out,
                               d_transcripts_out, stream);
}

// creation: per slice of rows the product launch (lane = (instance-base term, row)) and the walk (lane = (equation, row)), then ONE finish
// launch over the batch.  A slice is as many rows as keep the product launch at SIG_CREATE_LANES lanes: their tables of multiples live
// in the workspace (c->ipp_buf: the products are partial sums of the T_k, part of the prover's working set).  The secrets and the seeds
// come first in the staging: the secret span, cleared on every exit
#define SIG_CREATE_LANES 65536u
extern "C" int bpgpu_sigma_create_batch_ts(bpgpu_ctx *c, const bpgpu_sigma_relation *rel, size_t nbatch, const uint8_t *transcripts, size_t transcript_stride,
                                           const uint8_t *rng32, const uint8_t *points, const uint8_t *secrets, uint8_t *proofs_out, uint8_t *status,
                                           uint8_t *transcripts_out) {
    if (!c) return BPGPU_ERR_INVALID_ARG;
    int rc = sig_check_args(c, rel, nbatch, 0, true);
    if (rc) return rc;
    if ((rc = ipp_ts_host_args(c, transcripts, transcript_stride, nbatch))) return rc;
    if (nbatch == 0) return BPGPU_OK;
    if (!points || !secrets || !proofs_out || !status) return BPGPU_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = sig_check_gens_locked(c, rel))) return rc;
    hipStream_t s = c->stream;
    const size_t TS = BPGPU_TRANSCRIPT_BYTES, nstates = transcript_stride ? nbatch : 1, S = rel->h.S, P = rel->h.P, proof_len = 32 * (size_t)(rel->h.E + S);
    host_call<bpgpu_ctx> io(c, s);
    const int r_x = io.in(nbatch * S * 32), r_seed = io.in(nbatch * 32), r_p = io.in(nbatch * P * 32 + 64), r_ti = io.in(nstates * TS);
    const int r_pr = io.out(nbatch * proof_len), r_st = io.out(nbatch), r_t = io.out(transcripts_out ? nbatch * TS : 0);
    io.secrets(io.off[r_p]);   // secrets and seeds
    rc = io.open();
    if (rc) return io.finish(rc);
    io.put(r_x, secrets, nbatch * S * 32);
    if (rng32) io.put(r_seed, rng32, nbatch * 32);
    else if ((rc = os_random(c, io.h(r_seed), nbatch * 32)) != 0) return io.finish(rc);
    io.put(r_p, points, nbatch * P * 32);
    io.put(r_ti, transcripts, nstates * TS);
    if ((rc = io.upload())) return io.finish(rc);
    do {
        const bool ct = c->prover_ct;
        fb_walk w;
        if ((rc = fb_walk_for(c, ct, w))) break;
        const uint32_t nb32 = (uint32_t)nbatch, nvb = rel->h.nvb, E = rel->h.E;
        uint32_t slice = SIG_CREATE_LANES / (nvb ? nvb : 1) / 64 * 64;   // (nvb <= 32: at least 2 048 rows)
        if (slice > nb32) slice = (nb32 + 63) / 64 * 64;
        const size_t sz_tab = align_up((size_t)nvb * slice * SIG_VB_WORDS * 4 + 64), sz_prod = align_up((size_t)nvb * slice * 160 + 64), sz_bad = align_up(nbatch * 4);
        if ((rc = ipp_reserve(c, sz_tab + sz_prod + sz_bad))) break;
        sig_ws ws;
        ws.tab = (uint32_t *)c->ipp_buf;
        ws.prod = (uint32_t *)(c->ipp_buf + sz_tab);
        ws.bad = (uint32_t *)(c->ipp_buf + sz_tab + sz_prod);
        ws.nstride = slice;
        if (hipMemsetAsync(ws.bad, 0, sz_bad, s) != hipSuccess) {
            rc = fail(c, BPGPU_ERR_HIP, "memset failed");
            break;
        }
        sig_create_in in;
        in.secrets = (const uint32_t *)io.d(r_x);
        in.seeds = (const uint8_t *)io.d(r_seed);
        in.points = (const uint32_t *)io.d(r_p);
        in.ts_in = (const uint32_t *)io.d(r_ti);
        in.ts_in_stride = transcript_stride ? BP_TS_WORDS : 0;
        in.nrows = nb32;
        for (uint32_t row0 = 0; row0 < nb32; row0 += slice) {   // (slices run one after another on the stream: they share the workspace)
            ws.row0 = row0;
            const uint32_t nslice = std::min<uint32_t>(slice, nb32 - row0);
            if (nvb) LAUNCH_CT(c, s, ct, "sig_vb", k_sig_vb, nvb * slice / BP_BLOCK, BP_BLOCK, (const sig_rel *)rel->d, in, ws);
            LAUNCH_CT(c, s, ct, "sig_walk", k_sig_walk, E * slice / BP_BLOCK, BP_BLOCK, rel->h, in, ws, nslice, w.prm, w.table, (uint32_t *)io.d(r_pr));
        }
        LAUNCH(c, s, "sig_finish", k_sig_finish, (nb32 + RP_BLOCK - 1) / RP_BLOCK, RP_BLOCK, (const sig_rel *)rel->d, in, (const uint32_t *)ws.bad,
               (uint32_t *)io.d(r_pr), (uint8_t *)io.d(r_st), transcripts_out ? (uint32_t *)io.d(r_t) : nullptr);
        if (hipGetLastError() != hipSuccess) rc = fail(c, BPGPU_ERR_HIP, "launch failed");
    } while (0);
    rc = io.finish(io.download(rc));
    if (rc) return rc;
    memcpy(proofs_out, io.h(r_pr), nbatch * proof_len);
    memcpy(status, io.h(r_st), nbatch);
    if (transcripts_out) memcpy(transcripts_out, io.h(r_t), nbatch * TS);
    return BPGPU_OK;
}
