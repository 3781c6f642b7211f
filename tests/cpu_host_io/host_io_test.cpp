// TEST-ONLY: the staging state machine of the host-pointer entry points (bulletproofs_amd/csrc/host_io.h) on the CPU, against the fake
// HIP runtime of tests/cpu_pool/fake_device.cpp: streams are threads, copies are memcpys done BY THE STREAM THREAD, device memory is
// malloc'ed -- a pinned block freed while a copy is queued, or read after it was freed, is a use-after-free AddressSanitizer reports.
// The context below has what bpgpu.hip's has around the staging: ctx_enter / ctx_leave / host_wait, a pending submitted result, three
// working sets a prover clears.  These are re-implementations: host_io.h must not need bpgpu_ctx, so the production ctx_enter /
// collect_locked glue of bpgpu.hip itself is covered by the GPU suite only; what runs here is host_staging, host_call and dev_scope /
// dev_call.
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "../../bulletproofs_amd/csrc/host_io.h"

extern "C" void fake_stream_gate(hipStream_t s);
extern "C" void fake_open_gates(void);

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

struct test_ctx {
    host_staging io;
    std::string err;
    std::mutex mu;
    int device = 0;
    hipStream_t stream = nullptr;
    int fail_enter = 0, fail_leave = 0, fail_wait = 0;   // injected return codes
    int enters = 0, leaves = 0;                          // calls of ctx_enter that succeeded / of ctx_leave
    hipStream_t left_on = nullptr;                       // the stream of the last ctx_leave
    char *work[3] = {nullptr, nullptr, nullptr};
    size_t work_cap[3] = {1000, 0, 4096};
    struct {
        bool active = false;
        const char *h_out = nullptr;
        size_t bytes = 0;
        char *dst = nullptr;
    } pend;
    int deliveries = 0;
    test_ctx() {
        io.err = &err;
        io.hip_err_code = -4;
        hipStreamCreateWithFlags(&stream, 0);
        hipEventCreateWithFlags(&io.pin_ev, 0);
        for (int i = 0; i < 3; i++)
            if (work_cap[i]) hipMalloc((void **)&work[i], work_cap[i]);
    }
    ~test_ctx() {
        hipDeviceSynchronize();
        io.release();
        for (char *w : work)
            if (w) hipFree(w);
        hipStreamDestroy(stream);
    }
};
static int host_wait(test_ctx *c, hipStream_t s) {
    hipStreamSynchronize(s);
    c->io.waited();
    return c->fail_wait;
}
static int collect(test_ctx *c) {
    if (!c->pend.active) return 0;
    auto p = c->pend;
    c->pend.active = false;
    int rc = host_wait(c, c->stream);
    if (rc) return rc;
    memcpy(p.dst, p.h_out, p.bytes);
    c->deliveries++;
    return 0;
}
static int ctx_enter(test_ctx *c, hipStream_t, bool keep_staging) {
    if (c->fail_enter) return c->fail_enter;
    if (c->pend.active) {
        int rc = collect(c);
        if (rc) return rc;
    }
    c->enters++;
    return c->io.begin(keep_staging);
}
static int ctx_leave(test_ctx *c, hipStream_t s) {
    c->leaves++;
    c->left_on = s;
    if (c->fail_leave) return c->fail_leave;
    return c->io.left(s);
}
static void secret_spans(test_ctx *c, dev_span b[3]) {
    for (int i = 0; i < 3; i++) b[i] = {c->work[i], c->work_cap[i]};
}
typedef host_call<test_ctx> call;

static bool all_bytes(const char *p, size_t n, char v) {
    for (size_t i = 0; i < n; i++)
        if (p[i] != v) return false;
    return true;
}
// "the device": outputs = the leading bytes of the inputs
static void run_device(call &io) {
    hipMemcpyAsync(io.d(io.n_in), io.d(0), io.out_bytes() < io.in_bytes() ? io.out_bytes() : io.in_bytes(), hipMemcpyDeviceToDevice, io.s);
}

static void test_layout() {
    test_ctx c;
    const size_t ins[] = {0, 1, 255, 256, 257, (size_t)3 << 20, 0, ((size_t)5 << 20) + 7}, outs[] = {1, 0, 257}, devs[] = {0, 1000, (size_t)2 << 20};
    call io(&c, c.stream);
    int r[16], n = 0;
    size_t want[17] = {0};
    for (size_t b : ins) r[n] = io.in(b), want[n + 1] = want[n] + ((b + 255) & ~(size_t)255), n++;
    for (size_t b : outs) r[n] = io.out(b), want[n + 1] = want[n] + ((b + 255) & ~(size_t)255), n++;
    for (size_t b : devs) r[n] = io.dev(b), want[n + 1] = want[n] + ((b + 255) & ~(size_t)255), n++;
    CHECK(io.n == 14 && io.n_in == 8 && io.n_out == 11);
    for (int i = 0; i < n; i++) CHECK(r[i] == i && io.off[i] == want[i]);
    CHECK(io.off[n] == want[n]);
    CHECK(io.in_bytes() == want[8] && io.out_bytes() == want[11] - want[8]);
    CHECK(io.width(r[0]) == 0 && io.width(r[1]) == 256 && io.width(r[3]) == 256 && io.width(r[4]) == 512 && io.width(r[9]) == 0);
    CHECK(io.open() == 0);
    CHECK(c.io.pin_cap >= want[11] && c.io.io_cap >= want[14]);   // the host block has no room for device-only regions
    for (int i = 0; i < n; i++) CHECK(io.d(i) - io.d(0) == (ptrdiff_t)want[i]);
    for (int i = 0; i < 11; i++) CHECK(io.h(i) - io.h(0) == io.d(i) - io.d(0));
    CHECK(io.h(0) == io.h(1) && io.h(6) == io.h(7) && io.d(11) == io.d(12));   // zero-byte regions take no room
    // end to end: one upload, the device, one download
    for (size_t i = 0; i < io.in_bytes(); i++) io.h(0)[i] = (char)(i * 7 + 1);
    CHECK(io.upload() == 0);
    run_device(io);
    CHECK(io.finish(io.download(0)) == 0);
    for (size_t i = 0; i < io.out_bytes(); i++) CHECK(io.h(8)[i] == (char)(i * 7 + 1));
    {   // a plan the fixed-capacity array cannot hold, or one out of order, fails at open and writes nothing past off[]
        call big(&c, c.stream);
        for (int i = 0; i < call::MAX_REGIONS + 3; i++) big.in(100);
        CHECK(big.n == call::MAX_REGIONS && big.open() == -4 && !c.err.empty() && !big.entered);
        CHECK(big.finish(-4) == -4);
        call wrong(&c, c.stream);
        wrong.out(16);
        wrong.in(16);
        CHECK(wrong.open() == -4);
    }
    puts("layout ok");
}

static void test_growth_inside_a_call() {
    test_ctx c;
    call io(&c, c.stream);
    const int r_i = io.in(300), r_o = io.out(300);
    CHECK(io.open() == 0);
    char *first = io.hb;
    memset(io.h(r_i), 0x31, 300);
    CHECK(io.upload() == 0);
    char *nested = nullptr;
    CHECK(c.io.pin_alloc(c.io.pin_cap + 1, &nested) == 0);   // outgrows the block: it is retired, not freed
    CHECK(c.io.pin_retired.size() == 1 && c.io.pin_retired[0] == first && c.io.pin != first && io.hb == first);
    memset(nested, 0x77, 64);
    run_device(io);
    CHECK(io.finish(io.download(0)) == 0);
    CHECK(all_bytes(io.h(r_o), 300, 0x31));                  // downloaded into the retired block, still readable
    CHECK(c.io.pin_retired.size() == 1);
    CHECK(io.reopen() == 0);                                 // the fallback: nothing retired is freed
    CHECK(c.io.pin_retired.size() == 1 && c.io.pin_retired[0] == first);
    hipMemsetAsync(io.d(r_o), 0x32, 100, c.stream);
    CHECK(io.finish(io.download(0, 100)) == 0);
    CHECK(all_bytes(io.h(r_o), 100, 0x32) && all_bytes(io.h(r_o) + 100, 200, 0x31));
    call next(&c, c.stream);                                 // the next ordinary call frees it (no read of `first` from here on)
    next.in(16);
    next.out(16);
    CHECK(next.open() == 0);
    CHECK(c.io.pin_retired.empty());
    CHECK(next.finish(0) == 0);
    puts("growth ok");
}

static void test_reuse_guard() {
    test_ctx c;
    {   // a call that left without waiting, its copies held at a gate: the next call's first allocation waits for them
        call a(&c, c.stream);
        a.in(256);
        a.out(256);
        CHECK(a.open() == 0);
        memset(a.h(0), 0x11, 256);
        fake_stream_gate(c.stream);
        CHECK(a.upload() == 0);
        run_device(a);
        CHECK(a.download(0) == 0);
        CHECK(a.leave_in_flight() == 0);
        CHECK(c.io.pin_pending);
        std::atomic<bool> got{false};
        std::thread t([&] {
            call b(&c, c.stream);
            b.in(256);
            b.out(256);
            CHECK(b.open() == 0);
            got = true;
            memset(b.h(0), 0x22, 256);   // (would race with a's queued upload if the guard had not held)
            CHECK(b.finish(0) == 0);
        });
        std::this_thread::sleep_for(std::chrono::milliseconds(60));
        CHECK(!got.load());
        fake_open_gates();
        t.join();
        CHECK(got.load());
    }
    {   // after a mark the next allocation waits up to the mark only, not for what is queued behind it
        CHECK(c.io.begin(false) == 0);
        char *h = nullptr;
        CHECK(c.io.pin_alloc(256, &h) == 0);
        CHECK(c.io.io_reserve(256) == 0);
        CHECK(hipMemcpyAsync(c.io.io_dev, h, 256, hipMemcpyHostToDevice, c.stream) == hipSuccess);
        CHECK(c.io.pin_mark(c.stream) == 0);
        fake_stream_gate(c.stream);
        hipMemsetAsync(c.io.io_dev, 0, 256, c.stream);   // "the launch chain", held
        CHECK(c.io.left(c.stream) == 0);
        CHECK(c.io.begin(false) == 0);
        std::atomic<bool> got{false};
        std::thread t([&] {
            char *h2 = nullptr;
            CHECK(c.io.pin_alloc(256, &h2) == 0);
            got = true;
        });
        for (int i = 0; i < 500 && !got.load(); i++) std::this_thread::sleep_for(std::chrono::milliseconds(10));
        CHECK(got.load());                               // ... with the gate still closed
        CHECK(hipStreamQuery(c.stream) == hipErrorNotReady);
        fake_open_gates();
        t.join();
        hipStreamSynchronize(c.stream);
        c.io.waited();
    }
    puts("reuse guard ok");
}

static void test_finish() {
    test_ctx c;
    {   // rc priority: the call's, then ctx_leave's, then host_wait's
        const int cases[4][4] = {{5, 7, 9, 5}, {0, 7, 9, 7}, {0, 0, 9, 9}, {0, 0, 0, 0}};
        for (const auto &k : cases) {
            call io(&c, c.stream);
            io.in(64);
            io.out(64);
            CHECK(io.open() == 0);
            c.fail_leave = k[1], c.fail_wait = k[2];
            CHECK(io.finish(k[0]) == k[3]);
            c.fail_leave = c.fail_wait = 0;
            hipStreamSynchronize(c.stream);
            c.io.waited();
        }
        call never(&c, c.stream);   // not opened: finish hands the code back and touches nothing
        CHECK(never.finish(3) == 3);
    }
    for (int rc_call : {0, 3}) {   // secrets: the leading k host bytes and every device buffer, whatever the call's rc
        call io(&c, c.stream);
        const int r_a = io.in(500), r_b = io.in(100), r_o = io.out(700);
        io.secrets(io.off[r_b]);
        CHECK(io.open() == 0);
        const size_t k = io.off[r_b], all = io.off[r_o + 1];
        memset(io.hb, 0x5a, all);
        hipMemsetAsync(c.io.io_dev, 0xaa, c.io.io_cap, c.stream);
        for (int i = 0; i < 3; i++)
            if (c.work[i]) hipMemsetAsync(c.work[i], 0xaa, c.work_cap[i], c.stream);
        (void)r_a;
        CHECK(io.finish(rc_call) == rc_call);
        CHECK(all_bytes(io.hb, k, 0) && all_bytes(io.hb + k, all - k, 0x5a));
        CHECK(c.io.last_secret_bytes == k);
        CHECK(all_bytes(c.io.io_dev, c.io.io_cap, 0));
        for (int i = 0; i < 3; i++)
            if (c.work[i]) CHECK(all_bytes(c.work[i], c.work_cap[i], 0));
    }
    {   // a call without secrets clears nothing
        call io(&c, c.stream);
        io.in(256);
        io.out(256);
        CHECK(io.open() == 0);
        memset(io.hb, 0x5a, 512);
        hipMemsetAsync(c.work[0], 0xaa, c.work_cap[0], c.stream);
        CHECK(io.finish(0) == 0);
        CHECK(all_bytes(io.hb, 512, 0x5a) && all_bytes(c.work[0], c.work_cap[0], (char)0xaa));
    }
    puts("finish ok");
}

// a submitted call: outputs stay in flight, collect (or the next open) delivers them, once
static void submit(test_ctx &c, char fill, char *dst) {
    call io(&c, c.stream);
    io.in(256);
    const int r_o = io.out(256);
    CHECK(io.open() == 0);
    memset(io.h(0), fill, 256);
    fake_stream_gate(c.stream);
    CHECK(io.upload() == 0);
    run_device(io);
    CHECK(io.download(0) == 0);
    CHECK(io.leave_in_flight() == 0);
    c.pend.active = true;
    c.pend.h_out = io.h(r_o);
    c.pend.bytes = 256;
    c.pend.dst = dst;
}
static void test_submit_collect() {
    test_ctx c;
    char dst[256];
    memset(dst, 0x7f, 256);
    submit(c, 0x41, dst);
    CHECK(all_bytes(dst, 256, 0x7f));   // in flight: nothing delivered yet
    fake_open_gates();
    CHECK(collect(&c) == 0);
    CHECK(all_bytes(dst, 256, 0x41) && c.deliveries == 1);
    memset(dst, 0x7f, 256);
    CHECK(collect(&c) == 0);            // delivered once
    CHECK(all_bytes(dst, 256, 0x7f) && c.deliveries == 1);

    submit(c, 0x42, dst);
    fake_open_gates();
    call next(&c, c.stream);            // the next open comes first: it delivers, then reuses the block
    next.in(256);
    next.out(256);
    CHECK(next.open() == 0);
    CHECK(all_bytes(dst, 256, 0x42) && c.deliveries == 2);
    memset(next.h(0), 0x43, 512);
    CHECK(next.finish(0) == 0);
    memset(dst, 0x7f, 256);
    CHECK(collect(&c) == 0);
    CHECK(all_bytes(dst, 256, 0x7f) && c.deliveries == 2);
    puts("submit/collect ok");
}

// a device-pointer call: lock, stream, enter, body, ONE leave; the body's code first, then ctx_leave's
static void test_dev_call() {
    test_ctx c;
    hipStream_t mine = nullptr;
    hipStreamCreateWithFlags(&mine, 0);
    for (hipStream_t given : {mine, (hipStream_t) nullptr}) {   // the caller's stream, or the context's own where none is given
        const hipStream_t want = given ? given : c.stream;
        const int cases[4][3] = {{5, 7, 5}, {0, 7, 7}, {5, 0, 5}, {0, 0, 0}};   // body, ctx_leave, returned
        for (const auto &k : cases) {
            const int enters = c.enters, leaves = c.leaves;
            int ran = 0;
            c.fail_leave = k[1];
            const int rc = dev_call(&c, (void *)given, [&](hipStream_t s) {
                ran++;
                CHECK(s == want);
                CHECK(c.leaves == leaves);                   // not left before or during the body
                std::thread([&] { CHECK(!c.mu.try_lock()); }).join();   // the lock is held (asked from another thread: try_lock by the owner is undefined)
                return k[0];
            });
            c.fail_leave = 0;
            CHECK(rc == k[2] && ran == 1);
            CHECK(c.enters == enters + 1 && c.leaves == leaves + 1 && c.left_on == want);
            CHECK(c.mu.try_lock());                          // ... and free afterwards
            c.mu.unlock();
        }
    }
    {   // ctx_enter fails: no body, no leave, its code
        const int leaves = c.leaves;
        int ran = 0;
        c.fail_enter = 11;
        CHECK(dev_call(&c, nullptr, [&](hipStream_t) { return ++ran; }) == 11);
        c.fail_enter = 0;
        CHECK(ran == 0 && c.leaves == leaves);
        CHECK(c.mu.try_lock());
        c.mu.unlock();
    }
    {   // a check under the lock in front of the enter: where it refuses, its code, no enter, no body, no leave; where it passes, as above
        const int enters = c.enters, leaves = c.leaves;
        int ran = 0, checked = 0;
        auto pre = [&](int code) {
            return [&, code] {
                checked++;
                std::thread([&] { CHECK(!c.mu.try_lock()); }).join();
                CHECK(c.enters == enters);
                return code;
            };
        };
        CHECK(dev_call(&c, nullptr, pre(17), [&](hipStream_t) { return ++ran; }) == 17);
        CHECK(checked == 1 && ran == 0 && c.enters == enters && c.leaves == leaves);
        CHECK(dev_call(&c, (void *)mine, pre(0), [&](hipStream_t s) { return s == mine ? 0 : 1; }) == 0);
        CHECK(checked == 2 && c.enters == enters + 1 && c.leaves == leaves + 1 && c.left_on == mine);
        CHECK(c.mu.try_lock());
        c.mu.unlock();
    }
    {   // the scope alone: a path that returns without leave() is left by the destructor, one that called leave() is not left twice
        const int leaves = c.leaves;
        {
            dev_scope<test_ctx> sc(&c);
            CHECK(sc.rc == 0 && sc.enter((void *)mine) == 0 && sc.s == mine && c.leaves == leaves);
        }
        CHECK(c.leaves == leaves + 1 && c.left_on == mine);
        {
            dev_scope<test_ctx> sc(&c);
            CHECK(sc.enter(nullptr) == 0 && sc.s == c.stream);
            c.fail_leave = 9;
            CHECK(sc.leave() == 9);
            c.fail_leave = 0;
        }
        CHECK(c.leaves == leaves + 2 && c.left_on == c.stream);
        {
            dev_scope<test_ctx> sc(&c);   // never entered: never left
            c.fail_enter = 3;
            CHECK(sc.enter(nullptr) == 3);
            c.fail_enter = 0;
        }
        CHECK(c.leaves == leaves + 2);
        CHECK(c.mu.try_lock());
        c.mu.unlock();
    }
    hipStreamSynchronize(mine);
    hipStreamDestroy(mine);
    puts("dev call ok");
}

// The tail of a combined check: regions at their exact sizes -- inputs 300, outputs verdicts (n), batch result (64), transcripts (n * 208).
// First pass: "the device" fills verdicts with 0x10, the batch result with `byte0` then 0x20.., transcripts with 0x30; the per-proof pass
// overwrites ALL outputs on the device with 0x40 / 0x50 / 0x60 (only its verdicts may reach the caller).
struct comb_case {
    static const size_t N = 37, TSB = 37 * 208;
    call io;
    int r_i, r_v, r_b, r_t;
    comb_case(test_ctx &c) : io(&c, c.stream) {
        r_i = io.in(300);
        r_v = io.out(N), r_b = io.out(64), r_t = io.out(TSB);
    }
    void fill(char v, char b0, char b, char t) {
        hipMemsetAsync(io.d(r_v), v, N, io.s);
        hipMemsetAsync(io.d(r_b), b, 64, io.s);
        hipMemsetAsync(io.d(r_b), b0, 1, io.s);
        hipMemsetAsync(io.d(r_t), t, TSB, io.s);
    }
    void first_pass(test_ctx &c, char byte0, bool outgrow) {
        CHECK(io.open() == 0);
        memset(io.h(r_i), 0x31, 300);
        CHECK(io.upload() == 0);
        if (outgrow) {   // the pinned block is outgrown in mid-call: the outputs come back into a retired block
            char *nested = nullptr, *first = io.hb;
            CHECK(c.io.pin_alloc(c.io.pin_cap + 1, &nested) == 0);
            CHECK(c.io.pin_retired.size() == 1 && c.io.pin_retired[0] == first && io.hb == first);
            memset(nested, 0x77, 64);
        }
        fill(0x10, byte0, 0x20, 0x30);
        CHECK(io.finish(io.download(0)) == 0);
    }
};
static void test_combined_delivery() {
    const size_t N = comb_case::N, TSB = comb_case::TSB;
    for (bool outgrow : {false, true}) {
        {   // decided (byte 0 == 0): no second pass, everything the first pass's
            test_ctx c;
            comb_case k(c);
            k.first_pass(c, 0, outgrow);
            uint8_t *v = new uint8_t[N], *b = new uint8_t[33], *t = new uint8_t[TSB];
            int calls = 0;
            CHECK(k.io.deliver_combined(k.r_v, v, N, k.r_b, b, k.r_t, t, TSB, [&] { return ++calls; }) == 0);
            CHECK(calls == 0);
            CHECK(all_bytes((char *)v, N, 0x10) && b[0] == 0 && all_bytes((char *)b + 1, 32, 0x20) && all_bytes((char *)t, TSB, 0x30));
            delete[] v, delete[] b, delete[] t;
        }
        {   // undecided: ONE second pass, its verdicts; batch_out (all 33 bytes) and transcripts the first pass's
            test_ctx c;
            comb_case k(c);
            k.first_pass(c, 0x21, outgrow);
            uint8_t *v = new uint8_t[N], *b = new uint8_t[33], *t = new uint8_t[TSB];
            int calls = 0;
            const int enters = c.enters, leaves = c.leaves;
            CHECK(k.io.deliver_combined(k.r_v, v, N, k.r_b, b, k.r_t, t, TSB, [&] {
                calls++;
                if (outgrow) CHECK(c.io.pin_retired.size() == 1);   // the reopen kept the retired block
                k.fill(0x40, 0x51, 0x50, 0x60);
                return 0;
            }) == 0);
            CHECK(calls == 1 && c.enters == enters + 1 && c.leaves == leaves + 1);
            CHECK(all_bytes((char *)v, N, 0x40));
            CHECK(b[0] == 0x21 && all_bytes((char *)b + 1, 32, 0x20) && all_bytes((char *)t, TSB, 0x30));
            CHECK((uint8_t)k.io.h(k.r_b)[0] == 0x21 && all_bytes(k.io.h(k.r_b) + 1, 32, 0x20));   // the staged copy too
            delete[] v, delete[] b, delete[] t;
            // optional outputs left out: the verdicts still arrive
            comb_case k2(c);
            k2.first_pass(c, 0, false);
            uint8_t v2[comb_case::N];
            CHECK(k2.io.deliver_combined(k2.r_v, v2, N, k2.r_b, nullptr, k2.r_t, nullptr, 0, [&] { return 1; }) == 0);
            CHECK(all_bytes((char *)v2, N, 0x10));
        }
        {   // the second pass fails -- in the callable, or in its finish: that code, and the caller's verdicts untouched
            for (int where : {0, 1}) {
                test_ctx c;
                comb_case k(c);
                k.first_pass(c, 1, outgrow);
                uint8_t *v = new uint8_t[N], *b = new uint8_t[33], *t = new uint8_t[TSB];
                memset(v, 0x7f, N);
                int calls = 0;
                const int rc = k.io.deliver_combined(k.r_v, v, N, k.r_b, b, k.r_t, t, TSB, [&] {
                    calls++;
                    k.fill(0x40, 0x51, 0x50, 0x60);
                    if (where == 1) c.fail_wait = 13;
                    return where == 0 ? 12 : 0;
                });
                c.fail_wait = 0;
                CHECK(rc == (where == 0 ? 12 : 13) && calls == 1);
                CHECK(all_bytes((char *)v, N, 0x7f));
                CHECK(b[0] == 1 && all_bytes((char *)b + 1, 32, 0x20) && all_bytes((char *)t, TSB, 0x30));   // (handed out before the rerun)
                delete[] v, delete[] b, delete[] t;
            }
        }
    }
    puts("combined delivery ok");
}

int main() {
    test_layout();
    test_growth_inside_a_call();
    test_reuse_guard();
    test_finish();
    test_submit_collect();
    test_dev_call();
    test_combined_delivery();
    puts("all ok");
    return 0;
}
