// Test-only HIP module: thin kernels around the device build of the limb arithmetics (limb_ops.h, the same wrappers the CPU
// harness runs) and the __device__ copies of horner_wave.h's wavefront drivers, for tests/test_gpu_limb_bounds.py.  One lane per
// case for fe_* / sc28_* / ge_*, one 64-lane workgroup per case for hw_* and the drivers.  Every buffer is sized from the case count
// and every kernel guards its case index by it.  The extern "C" wrappers allocate, copy, launch, synchronise and copy back, and return
// the first HIP error instead of aborting.  Never part of libbpgpu.so.
#include <hip/hip_runtime.h>
#include <vector>

#include "../cpu_harness/limb_ops.h"

using namespace bp;

// kernel bodies only in the device pass: the host pass sees wavevec.h's host types
__global__ __launch_bounds__(64) void k_fe_raw(int op, uint32_t n, const uint32_t *a, const uint32_t *b, uint32_t *out, uint8_t *ok) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i < n) ok[i] = lo::fe_raw(op, a + 10 * i, b + 10 * i, out + 10 * i);
#endif
}
__global__ __launch_bounds__(64) void k_fe_cols_raw(uint32_t n, const uint64_t *c, uint32_t *out, uint8_t *ok) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i < n) ok[i] = lo::fe_cols_raw(c + 10 * i, out + 10 * i);
#endif
}
__global__ __launch_bounds__(64) void k_limbs_to_fe_raw(uint32_t n, const uint32_t *l16, uint32_t *out, uint8_t *ok) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i < n) ok[i] = lo::limbs_to_fe_raw(l16 + 16 * i, out + 10 * i);
#endif
}
__global__ __launch_bounds__(64) void k_sc_raw(int op, uint32_t n, const uint32_t *a, const uint32_t *b, uint32_t *out, uint8_t *ok) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i < n) ok[i] = lo::sc_raw(op, a + 10 * i, b + 10 * i, out + 10 * i);
#endif
}
__global__ __launch_bounds__(64) void k_sc_cols_raw(uint32_t n, const uint64_t *c, uint32_t *out, uint8_t *ok) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i < n) ok[i] = lo::sc_cols_raw(c + 20 * i, out + 10 * i);
#endif
}
__global__ __launch_bounds__(64) void k_ge_raw(int op, uint32_t n, const uint32_t *p, const uint32_t *q, uint32_t *out, uint8_t *ok) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i < n) ok[i] = lo::ge_raw(op, p + 40 * i, q + 40 * i, out + 40 * i);
#endif
}
// one wavefront (= workgroup) per case; the case index is uniform over the workgroup
__global__ __launch_bounds__(64) void k_hw_raw(int op, uint32_t n, const uint32_t *a, const uint32_t *b, int nsq, uint32_t *out, uint8_t *ok) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ __attribute__((aligned(16))) uint32_t lds[128];
    const uint32_t c = blockIdx.x, lane = threadIdx.x;
    if (c >= n) return;
    wv_ctx cx;
    cx.lds = lds;
    const wu32 r = lo::hw_raw(cx, op, a[64 * c + lane], b[64 * c + lane], nsq);
    out[64 * c + lane] = r;
    const uint64_t over = __ballot(r > LO_HW_SMALL);
    if (lane == 0) ok[c] = over == 0;
#endif
}
__global__ __launch_bounds__(64) void k_drv_invsqrt(uint32_t n, const uint32_t *t8, uint32_t *out10) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ __attribute__((aligned(16))) uint32_t lds[128];
    const uint32_t c = blockIdx.x;
    if (c >= n) return;
    hw_invsqrt_raw_fe((const uint16_t *)(t8 + 8 * c), lds, (fe *)(out10 + 10 * c));
#endif
}
__global__ __launch_bounds__(64) void k_drv_decode(uint32_t n, const uint32_t *w8, uint32_t *out40) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t c = blockIdx.x;
    if (c >= n) return;
    ge_ext r;
    hw_ristretto_decode(r, w8 + 8 * c);
    if (threadIdx.x == 0) *(ge_ext *)(out40 + 40 * c) = r;
#endif
}
__global__ __launch_bounds__(64) void k_drv_point_shift(uint32_t n, const uint32_t *p40, int shift, uint32_t *out40) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t c = blockIdx.x;
    if (c >= n) return;
    const ge_ext p = *(const ge_ext *)(p40 + 40 * c);
    hw_point_shift(p, shift, (ge_ext *)(out40 + 40 * c));
#endif
}
__global__ __launch_bounds__(64) void k_drv_shift_table8(uint32_t n, const uint32_t *p40, int shift, uint32_t *out320) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t c = blockIdx.x;
    if (c >= n) return;
    const ge_ext p = *(const ge_ext *)(p40 + 40 * c);
    hw_shift_table8(p, shift, (ge_cached *)(out320 + 320 * c));
#endif
}
__global__ __launch_bounds__(64) void k_drv_horner(uint32_t n, const uint16_t *colq16, uint32_t *out40) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t c = blockIdx.x;
    if (c >= n) return;
    hw_horner_msm(colq16 + 4096 * (size_t)c, (ge_ext *)(out40 + 40 * c));
#endif
}
__global__ __launch_bounds__(64) void k_drv_horner8(uint32_t n, const uint16_t *colq8, uint32_t *out40) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ __attribute__((aligned(16))) uint32_t lds[128];
    const uint32_t c = blockIdx.x;
    if (c >= n) return;
    hw_horner8_msm(colq8 + 2048 * (size_t)c, lds, (ge_ext *)(out40 + 40 * c));
#endif
}

namespace {
// device buffers of one call; the first HIP error sticks and is what the wrapper returns
struct Dev {
    std::vector<void *> ptrs;
    hipError_t err = hipSuccess;
    ~Dev() {
        for (void *p : ptrs) (void)hipFree(p);
    }
    template <class T>
    T *alloc(size_t count) {
        void *d = nullptr;
        if (err != hipSuccess) return nullptr;
        err = hipMalloc(&d, count * sizeof(T));
        if (err != hipSuccess) return nullptr;
        ptrs.push_back(d);
        err = hipMemset(d, 0, count * sizeof(T));
        return (T *)d;
    }
    template <class T>
    T *in(const T *h, size_t count) {
        T *d = alloc<T>(count);
        if (err == hipSuccess) err = hipMemcpy(d, h, count * sizeof(T), hipMemcpyHostToDevice);
        return d;
    }
    template <class T>
    void back(T *h, const T *d, size_t count) {
        if (err == hipSuccess) err = hipMemcpy(h, d, count * sizeof(T), hipMemcpyDeviceToHost);
    }
    bool ready() const { return err == hipSuccess; }
    void done() {
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
    }
};
inline dim3 lanes(uint32_t n) { return dim3((n + 63u) / 64u); }
}  // namespace

extern "C" {
int g_fe_raw(int op, uint32_t n, const uint32_t *a, const uint32_t *b, uint32_t *out, uint8_t *ok) {
    if (n == 0) return 0;
    Dev d;
    const uint32_t *da = d.in(a, 10 * (size_t)n), *db = d.in(b, 10 * (size_t)n);
    uint32_t *dout = d.alloc<uint32_t>(10 * (size_t)n);
    uint8_t *dok = d.alloc<uint8_t>(n);
    if (d.ready()) hipLaunchKernelGGL(k_fe_raw, lanes(n), dim3(64), 0, 0, op, n, da, db, dout, dok);
    d.done();
    d.back(out, dout, 10 * (size_t)n);
    d.back(ok, dok, n);
    return (int)d.err;
}
int g_fe_cols_raw(uint32_t n, const uint64_t *c, uint32_t *out, uint8_t *ok) {
    if (n == 0) return 0;
    Dev d;
    const uint64_t *dc = d.in(c, 10 * (size_t)n);
    uint32_t *dout = d.alloc<uint32_t>(10 * (size_t)n);
    uint8_t *dok = d.alloc<uint8_t>(n);
    if (d.ready()) hipLaunchKernelGGL(k_fe_cols_raw, lanes(n), dim3(64), 0, 0, n, dc, dout, dok);
    d.done();
    d.back(out, dout, 10 * (size_t)n);
    d.back(ok, dok, n);
    return (int)d.err;
}
int g_limbs_to_fe_raw(uint32_t n, const uint32_t *l16, uint32_t *out, uint8_t *ok) {
    if (n == 0) return 0;
    Dev d;
    const uint32_t *dl = d.in(l16, 16 * (size_t)n);
    uint32_t *dout = d.alloc<uint32_t>(10 * (size_t)n);
    uint8_t *dok = d.alloc<uint8_t>(n);
    if (d.ready()) hipLaunchKernelGGL(k_limbs_to_fe_raw, lanes(n), dim3(64), 0, 0, n, dl, dout, dok);
    d.done();
    d.back(out, dout, 10 * (size_t)n);
    d.back(ok, dok, n);
    return (int)d.err;
}
int g_sc_raw(int op, uint32_t n, const uint32_t *a, const uint32_t *b, uint32_t *out, uint8_t *ok) {
    if (n == 0) return 0;
    Dev d;
    const uint32_t *da = d.in(a, 10 * (size_t)n), *db = d.in(b, 10 * (size_t)n);
    uint32_t *dout = d.alloc<uint32_t>(10 * (size_t)n);
    uint8_t *dok = d.alloc<uint8_t>(n);
    if (d.ready()) hipLaunchKernelGGL(k_sc_raw, lanes(n), dim3(64), 0, 0, op, n, da, db, dout, dok);
    d.done();
    d.back(out, dout, 10 * (size_t)n);
    d.back(ok, dok, n);
    return (int)d.err;
}
int g_sc_cols_raw(uint32_t n, const uint64_t *c, uint32_t *out, uint8_t *ok) {
    if (n == 0) return 0;
    Dev d;
    const uint64_t *dc = d.in(c, 20 * (size_t)n);
    uint32_t *dout = d.alloc<uint32_t>(10 * (size_t)n);
    uint8_t *dok = d.alloc<uint8_t>(n);
    if (d.ready()) hipLaunchKernelGGL(k_sc_cols_raw, lanes(n), dim3(64), 0, 0, n, dc, dout, dok);
    d.done();
    d.back(out, dout, 10 * (size_t)n);
    d.back(ok, dok, n);
    return (int)d.err;
}
int g_ge_raw(int op, uint32_t n, const uint32_t *p, const uint32_t *q, uint32_t *out, uint8_t *ok) {
    if (n == 0) return 0;
    Dev d;
    const uint32_t *dp = d.in(p, 40 * (size_t)n), *dq = d.in(q, 40 * (size_t)n);
    uint32_t *dout = d.alloc<uint32_t>(40 * (size_t)n);
    uint8_t *dok = d.alloc<uint8_t>(n);
    if (d.ready()) hipLaunchKernelGGL(k_ge_raw, lanes(n), dim3(64), 0, 0, op, n, dp, dq, dout, dok);
    d.done();
    d.back(out, dout, 40 * (size_t)n);
    d.back(ok, dok, n);
    return (int)d.err;
}
int g_hw_raw(int op, uint32_t n, const uint32_t *a, const uint32_t *b, int nsq, uint32_t *out, uint8_t *ok) {
    if (n == 0) return 0;
    Dev d;
    const uint32_t *da = d.in(a, 64 * (size_t)n), *db = d.in(b, 64 * (size_t)n);
    uint32_t *dout = d.alloc<uint32_t>(64 * (size_t)n);
    uint8_t *dok = d.alloc<uint8_t>(n);
    if (d.ready()) hipLaunchKernelGGL(k_hw_raw, dim3(n), dim3(64), 0, 0, op, n, da, db, nsq, dout, dok);
    d.done();
    d.back(out, dout, 64 * (size_t)n);
    d.back(ok, dok, n);
    return (int)d.err;
}
int g_drv_invsqrt(uint32_t n, const uint32_t *t8, uint32_t *out10) {
    if (n == 0) return 0;
    Dev d;
    const uint32_t *dt = d.in(t8, 8 * (size_t)n);
    uint32_t *dout = d.alloc<uint32_t>(10 * (size_t)n);
    if (d.ready()) hipLaunchKernelGGL(k_drv_invsqrt, dim3(n), dim3(64), 0, 0, n, dt, dout);
    d.done();
    d.back(out10, dout, 10 * (size_t)n);
    return (int)d.err;
}
int g_drv_decode(uint32_t n, const uint32_t *w8, uint32_t *out40) {
    if (n == 0) return 0;
    Dev d;
    const uint32_t *dw = d.in(w8, 8 * (size_t)n);
    uint32_t *dout = d.alloc<uint32_t>(40 * (size_t)n);
    if (d.ready()) hipLaunchKernelGGL(k_drv_decode, dim3(n), dim3(64), 0, 0, n, dw, dout);
    d.done();
    d.back(out40, dout, 40 * (size_t)n);
    return (int)d.err;
}
int g_drv_point_shift(uint32_t n, const uint32_t *p40, int shift, uint32_t *out40) {
    if (n == 0) return 0;
    Dev d;
    const uint32_t *dp = d.in(p40, 40 * (size_t)n);
    uint32_t *dout = d.alloc<uint32_t>(40 * (size_t)n);
    if (d.ready()) hipLaunchKernelGGL(k_drv_point_shift, dim3(n), dim3(64), 0, 0, n, dp, shift, dout);
    d.done();
    d.back(out40, dout, 40 * (size_t)n);
    return (int)d.err;
}
int g_drv_shift_table8(uint32_t n, const uint32_t *p40, int shift, uint32_t *out320) {
    if (n == 0) return 0;
    Dev d;
    const uint32_t *dp = d.in(p40, 40 * (size_t)n);
    uint32_t *dout = d.alloc<uint32_t>(320 * (size_t)n);
    if (d.ready()) hipLaunchKernelGGL(k_drv_shift_table8, dim3(n), dim3(64), 0, 0, n, dp, shift, dout);
    d.done();
    d.back(out320, dout, 320 * (size_t)n);
    return (int)d.err;
}
int g_drv_horner(uint32_t n, const uint16_t *colq16, uint32_t *out40) {
    if (n == 0) return 0;
    Dev d;
    const uint16_t *dq = d.in(colq16, 4096 * (size_t)n);
    uint32_t *dout = d.alloc<uint32_t>(40 * (size_t)n);
    if (d.ready()) hipLaunchKernelGGL(k_drv_horner, dim3(n), dim3(64), 0, 0, n, dq, dout);
    d.done();
    d.back(out40, dout, 40 * (size_t)n);
    return (int)d.err;
}
int g_drv_horner8(uint32_t n, const uint16_t *colq8, uint32_t *out40) {
    if (n == 0) return 0;
    Dev d;
    const uint16_t *dq = d.in(colq8, 2048 * (size_t)n);
    uint32_t *dout = d.alloc<uint32_t>(40 * (size_t)n);
    if (d.ready()) hipLaunchKernelGGL(k_drv_horner8, dim3(n), dim3(64), 0, 0, n, dq, dout);
    d.done();
    d.back(out40, dout, 40 * (size_t)n);
    return (int)d.err;
}
}
