// Host-side staging of the host-pointer entry points (host-only C++, no kernels: it also compiles with g++ against a fake HIP
// runtime, tests/cpu_host_io/).
//   host_staging: the context's pinned block, its guard event and the persistent device IO buffer.
//   host_call:    ONE call's use of them -- regions declared in order, one H2D copy, one D2H copy, one wait.
//   dev_scope / dev_call: ONE device-pointer call -- lock, device, stream, ctx_enter ... ctx_leave on every path.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

static inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// a failed HIP call inside a host_staging member: its text and hipGetErrorString go to the context's error text
#define HOST_IO_CHK(call)                                             \
    do {                                                              \
        hipError_t e_ = (call);                                       \
        if (e_ != hipSuccess) return hip_failed(#call " failed", e_); \
    } while (0)

struct host_staging {
    // pinned host staging (ragged work decompositions, library-drawn randomness, the host-pointer entry points' IO):
    // copies out of it are truly asynchronous; pin_ev guards its reuse by the next call
    char *pin = nullptr;
    size_t last_secret_bytes = 0;      // leading bytes of the pinned block that held the last prover call's secrets
    size_t pin_cap = 0, pin_off = 0, pin_marked = 0;   // pin_marked: bytes already guarded by a recorded pin_ev (pin_mark)
    hipEvent_t pin_ev = nullptr;
    bool pin_pending = false;
    int hip_err_code = -1;             // what a failed HIP call returns to the owner ...
    std::vector<char *> pin_retired;   // outgrown mid-call: still referenced by that call, freed when the next one begins
    // persistent device-side IO buffer of the host-pointer entry points (no hipMalloc / hipFree per call)
    char *io_dev = nullptr;
    size_t io_cap = 0;
    std::string *err = nullptr;        // ... and the owner's error text, where the failing call and hipGetErrorString go

    int failed(const char *text) {
        if (err) *err = text;
        return hip_err_code;
    }
    int hip_failed(const char *what, hipError_t e) {
        if (err) *err = std::string(what) + ": " + hipGetErrorString(e);
        return hip_err_code;
    }

    // A call begins: the block is empty again and what the previous call retired is freed.  keep_retired: the call continues an
    // earlier one of the same entry point that still holds pointers into retired blocks (the per-proof fallback of a combined check).
    int begin(bool keep_retired) {
        pin_off = 0;
        pin_marked = 0;
        if (!pin_retired.empty() && !keep_retired) {
            if (pin_pending) HOST_IO_CHK(hipEventSynchronize(pin_ev));
            pin_pending = false;
            for (char *q : pin_retired) hipHostFree(q);
            pin_retired.clear();
        }
        return 0;
    }
    // bump allocation from the pinned block; the first allocation of a call waits until the previous call's copies out of the
    // block are done.  A block outgrown in mid-call is retired, not freed: earlier pieces of this call stay valid.
    int pin_alloc(size_t bytes, char **out) {
        if (pin_pending) {
            HOST_IO_CHK(hipEventSynchronize(pin_ev));
            pin_pending = false;
        }
        const size_t need = pin_off + align_up(bytes);
        if (need > pin_cap) {
            if (pin && pin_off) pin_retired.push_back(pin);
            else if (pin) HOST_IO_CHK(hipHostFree(pin));
            pin = nullptr;
            pin_cap = 0;
            const size_t cap = need + need / 2 + (64 << 10);
            HOST_IO_CHK(hipHostMalloc((void **)&pin, cap, hipHostMallocDefault));
            pin_cap = cap;
            pin_off = 0;
            pin_marked = 0;
        }
        *out = pin + pin_off;
        pin_off += align_up(bytes);
        return 0;
    }
    // An H2D copy out of the block has just been enqueued on s and nothing else of this call will touch the bytes allocated so
    // far: record the guard event NOW rather than at the end of the call, so that the next call on this context waits for the
    // copy, not for the whole launch chain behind it (device-pointer calls that stage only their rng bytes or a segment table:
    // with many lanes in flight the host would otherwise stall on every reuse of a lane)
    int pin_mark(hipStream_t s) {
        HOST_IO_CHK(hipEventRecord(pin_ev, s));
        pin_pending = true;
        pin_marked = pin_off;
        return 0;
    }
    int io_reserve(size_t bytes) {
        if (bytes <= io_cap) return 0;
        HOST_IO_CHK(hipDeviceSynchronize());
        if (io_dev) HOST_IO_CHK(hipFree(io_dev));
        io_dev = nullptr;
        io_cap = 0;
        const size_t cap = bytes + bytes / 2 + (64 << 10);
        HOST_IO_CHK(hipMalloc((void **)&io_dev, cap));
        io_cap = cap;
        return 0;
    }
    // the call's stream work is enqueued: staged bytes behind the last mark are in flight on s, the next call waits for them
    int left(hipStream_t s) {
        if (pin_off > pin_marked) {
            HOST_IO_CHK(hipEventRecord(pin_ev, s));
            pin_pending = true;
        }
        return 0;
    }
    // the stream has been drained
    void waited() {
        pin_pending = false;
        pin_off = 0;
    }
    void release() {
        if (io_dev) hipFree(io_dev);
        if (pin) hipHostFree(pin);
        for (char *q : pin_retired) hipHostFree(q);
        if (pin_ev) hipEventDestroy(pin_ev);
        io_dev = pin = nullptr;
        pin_ev = nullptr;
        pin_retired.clear();
        io_cap = pin_cap = pin_off = pin_marked = 0;
    }
};

struct dev_span {
    char *p;
    size_t bytes;
};

// One host-pointer call.  Ctx has a member `host_staging io` and, as free functions, ctx_enter(c, s, keep_staging), ctx_leave(c, s),
// host_wait(c, s) and secret_spans(c, dev_span[3]) (the device working sets a prover clears besides io_dev).
// Regions are declared in order -- inputs (uploaded), outputs (downloaded), device-only ones -- each align_up(bytes) wide, at the
// same offset in the pinned block and in io_dev; sizes are taken as given (callers keep their slack bytes in them).
template <class Ctx>
struct host_call {
    enum { MAX_REGIONS = 24 };
    Ctx *c;
    hipStream_t s;
    host_staging &st;
    size_t off[MAX_REGIONS + 1] = {0};
    int n = 0, n_in = 0, n_out = 0;   // regions [0, n_in) are inputs, [n_in, n_out) outputs, [n_out, n) device-only
    char *hb = nullptr;               // the call's pinned block: stays valid (retired at worst) until the next call begins
    bool entered = false, has_secrets = false, bad_plan = false;
    size_t secret_bytes = 0;

    host_call(Ctx *c_, hipStream_t s_) : c(c_), s(s_), st(c_->io) {}

    // a region too many, or declared out of order, makes open() fail: nothing is written past off[]
    int region(size_t bytes, bool in_order = true) {
        if (n >= MAX_REGIONS || !in_order) {
            bad_plan = true;
            return 0;
        }
        off[n + 1] = off[n] + align_up(bytes);
        return n++;
    }
    int in(size_t bytes) {
        const int r = region(bytes, n == n_in);
        if (!bad_plan) n_in = n_out = n;
        return r;
    }
    int out(size_t bytes) {
        const int r = region(bytes, n == n_out);
        if (!bad_plan) n_out = n;
        return r;
    }
    int dev(size_t bytes) { return region(bytes); }
    // a prover: finish() clears the device working sets and the leading `bytes` of the pinned block
    void secrets(size_t bytes) {
        has_secrets = true;
        secret_bytes = bytes;
    }

    size_t in_bytes() const { return off[n_in]; }
    size_t out_bytes() const { return off[n_out] - off[n_in]; }
    size_t width(int r) const { return off[r + 1] - off[r]; }
    char *h(int r) const { return hb + off[r]; }
    char *d(int r) const { return st.io_dev + off[r]; }
    void put(int r, const void *src, size_t bytes) { memcpy(h(r), src, bytes); }

    int open() {
        if (bad_plan) return st.failed("host_call: more than MAX_REGIONS regions, or regions declared out of order");
        int rc = ctx_enter(c, s, false);
        if (rc) return rc;
        entered = true;
        rc = st.io_reserve(off[n]);
        if (rc) return rc;
        return st.pin_alloc(off[n_out], &hb);
    }
    // the per-proof fallback: pointers of the first pass stay valid
    int reopen() { return ctx_enter(c, s, true); }
    int upload() {
        hipError_t e = hipMemcpyAsync(st.io_dev, hb, in_bytes(), hipMemcpyHostToDevice, s);
        return e == hipSuccess ? 0 : st.hip_failed("hipMemcpyAsync(io_dev, h, in_bytes, hipMemcpyHostToDevice, s) failed", e);
    }
    // the output span, or its leading `bytes`; skipped when the call has failed already
    int download(int rc, size_t bytes = ~(size_t)0) {
        if (rc) return rc;
        if (bytes > out_bytes()) bytes = out_bytes();
        if (hipMemcpyAsync(h(n_in), d(n_in), bytes, hipMemcpyDeviceToHost, s) != hipSuccess) return st.failed("D2H copy failed");
        return 0;
    }
    // the submit form: results stay in flight
    int leave_in_flight() { return ctx_leave(c, s); }
    // Every exit after a successful ctx_enter: the call's end is recorded (ctx_leave), the stream is drained (host_wait).  A prover's
    // device buffers are cleared on the stream behind its last copy, the secret part of its pinned block after the wait.
    int finish(int rc) {
        if (!entered) return rc;
        bool ok = true;
        if (has_secrets) {
            dev_span b[4] = {{st.io_dev, st.io_cap}};
            secret_spans(c, b + 1);
            for (const dev_span &x : b)
                if (x.p) ok = hipMemsetAsync(x.p, 0, x.bytes, s) == hipSuccess && ok;
        }
        const int rc2 = ctx_leave(c, s), rc3 = host_wait(c, s);
        if (has_secrets) {
            if (hb && secret_bytes) memset(hb, 0, secret_bytes);
            st.last_secret_bytes = (hb == st.pin) ? secret_bytes : 0;
            if (!rc && !ok) rc = st.failed("clearing the prover's working set failed");
        }
        return rc ? rc : (rc2 ? rc2 : rc3);
    }
    // The combined check did not decide: `per_proof` enqueues the batch again proof by proof (inputs are still on the device), its
    // verdicts -- the outputs up to the end of region r_verdict -- replace the first pass's.  The first pass's batch_out (33 bytes
    // at h(r_batch)) is kept.  The outputs may sit in a block that the first pass outgrew and retired: reopen keeps it alive.
    template <class F>
    int rerun_per_proof(int r_verdict, int r_batch, F per_proof) {
        char bo[33];
        memcpy(bo, h(r_batch), 33);
        int rc = reopen();
        if (rc) return rc;
        rc = finish(download(per_proof(), off[r_verdict + 1] - off[n_in]));
        if (rc) return rc;
        memcpy(h(r_batch), bo, 33);
        return 0;
    }
    // What a combined check hands to its caller once finish() has succeeded: batch_out (33 bytes) and the transcripts are the first
    // pass's; the verdicts are the first pass's where the combination decided (byte 0 of the batch result is 0), the per-proof
    // rerun's otherwise.  A failed rerun is returned and leaves the caller's verdicts untouched.  batch_out / ts_out may be null.
    template <class F>
    int deliver_combined(int r_verdict, uint8_t *verdict, size_t verdict_bytes, int r_batch, uint8_t *batch_out, int r_ts, uint8_t *ts_out, size_t ts_bytes,
                         F per_proof) {
        if (batch_out) memcpy(batch_out, h(r_batch), 33);
        if (ts_out) memcpy(ts_out, h(r_ts), ts_bytes);
        if ((uint8_t)h(r_batch)[0] != 0) {
            const int rc = rerun_per_proof(r_verdict, r_batch, per_proof);
            if (rc) return rc;
        }
        memcpy(verdict, h(r_verdict), verdict_bytes);
        return 0;
    }
};

// One device-pointer call.  Ctx has `std::mutex mu`, `int device`, `hipStream_t stream`, `host_staging io` and the free functions
// ctx_enter / ctx_leave.  The scope holds the lock from its construction and has set the device (rc: why it could not); after a
// successful enter() the context is left exactly once -- by leave(), or by the destructor on a path that returned without it.
template <class Ctx>
struct dev_scope {
    Ctx *c;
    std::lock_guard<std::mutex> lk;
    hipStream_t s = nullptr;
    bool entered = false;
    int rc = 0;

    explicit dev_scope(Ctx *c_) : c(c_), lk(c_->mu) {
        const hipError_t e = hipSetDevice(c->device);
        if (e != hipSuccess) rc = c->io.hip_failed("hipSetDevice(c->device) failed", e);
    }
    ~dev_scope() {
        if (entered) (void)ctx_leave(c, s);
    }
    // the caller's stream, or the context's own where it gives none
    int enter(void *stream) {
        s = stream ? (hipStream_t)stream : c->stream;
        const int rce = ctx_enter(c, s, false);
        entered = !rce;
        return rce;
    }
    int leave() {
        entered = false;
        return ctx_leave(c, s);
    }
};
// ... and the whole of it where nothing happens behind the leave: `pre` (checks of the context's state, under the lock) refuses before the
// context is entered; then the body's code if non-zero, else ctx_leave's; ctx_enter's, and no body, where that fails
template <class Ctx, class P, class F>
static inline int dev_call(Ctx *c, void *stream, P pre, F body) {
    dev_scope<Ctx> sc(c);
    if (sc.rc) return sc.rc;
    int rc = pre();
    if (!rc) rc = sc.enter(stream);
    if (rc) return rc;
    rc = body(sc.s);
    const int rc2 = sc.leave();
    return rc ? rc : rc2;
}
template <class Ctx, class F>
static inline int dev_call(Ctx *c, void *stream, F body) {
    return dev_call(c, stream, [] { return 0; }, body);
}
