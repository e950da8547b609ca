// op_common.h -- what the network-op units (corr_sampler, corr_pyramid, stem_conv, conv3x3, conv1x1, gshead, group_norm, fused_loss, unproject, pack_views, splat) share:
// the fp32 / fp16 storage traits, the run-time dtype -> compile-time type dispatch, and the host-side argument checks of their extern "C" entry
// points.  Not for the rasteriser (gsr_*, capi.hip).  No floating-point arithmetic lives here, so the header is indifferent to the contraction
// setting of the unit that includes it.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gpsgs.h"

namespace {

// ---- storage types: tensors are fp32 or fp16 (stage 2 runs under AMP), the arithmetic is fp32 ------------------------------------------------
template <typename T> __device__ __forceinline__ float ldf(const T *p);
template <> __device__ __forceinline__ float ldf<float>(const float *p) { return *p; }
template <> __device__ __forceinline__ float ldf<__half>(const __half *p) { return __half2float(*p); }
template <typename T> __device__ __forceinline__ void stf(T *p, float v);
template <> __device__ __forceinline__ void stf<float>(float *p, float v) { *p = v; }
template <> __device__ __forceinline__ void stf<__half>(__half *p, float v) { *p = __float2half(v); }
template <typename T> __device__ __forceinline__ float rnd(float v);  // round to the storage type (fp16 pyramids are pooled level by level)
template <> __device__ __forceinline__ float rnd<float>(float v) { return v; }
template <> __device__ __forceinline__ float rnd<__half>(float v) { return __half2float(__float2half(v)); }

// DT 0 = fp32, 1 = fp16 (the `dtype` of the C ABI).  V = elements per 16 bytes; load / store move V elements at a 16-byte aligned address,
// store4 four elements at a 4-element aligned one; every store rounds once per element.
template <int DT_> struct Storage;
template <> struct Storage<0> {
    typedef float T;
    static constexpr int DT = 0, V = 4;
    static __device__ __forceinline__ void load(const T *p, float (&v)[4]) {
        const float4 f = *reinterpret_cast<const float4 *>(p);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    }
    static __device__ __forceinline__ void store(T *p, const float (&v)[4]) { *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]); }
    static __device__ __forceinline__ void store4(T *p, const float (&v)[4]) { store(p, v); }
    static __device__ __forceinline__ float load1(const T *p) { return ldf(p); }
    static __device__ __forceinline__ void store1(T *p, float v) { stf(p, v); }
};
template <> struct Storage<1> {
    typedef __half T;
    static constexpr int DT = 1, V = 8;
    static __device__ __forceinline__ void load(const T *p, float (&v)[8]) {
        const uint4 u = *reinterpret_cast<const uint4 *>(p);
        const __half2 *h = reinterpret_cast<const __half2 *>(&u);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float2 f = __half22float2(h[q]);
            v[2 * q] = f.x; v[2 * q + 1] = f.y;
        }
    }
    static __device__ __forceinline__ void store(T *p, const float (&v)[8]) {
        uint4 u;
        __half2 *h = reinterpret_cast<__half2 *>(&u);
#pragma unroll
        for (int q = 0; q < 4; q++) h[q] = __floats2half2_rn(v[2 * q], v[2 * q + 1]);
        *reinterpret_cast<uint4 *>(p) = u;
    }
    static __device__ __forceinline__ void store4(T *p, const float (&v)[4]) {
        uint2 u;
        __half2 *h = reinterpret_cast<__half2 *>(&u);
        h[0] = __floats2half2_rn(v[0], v[1]);
        h[1] = __floats2half2_rn(v[2], v[3]);
        *reinterpret_cast<uint2 *>(p) = u;
    }
    static __device__ __forceinline__ float load1(const T *p) { return ldf(p); }
    static __device__ __forceinline__ void store1(T *p, float v) { stf(p, v); }
};

inline bool dtype_ok(int dtype) { return dtype == 0 || dtype == 1; }

// f(Storage<dtype>()): the run-time dtype (checked by the caller) as a compile-time tag -- `typename decltype(t)::T` is float or __half,
// `decltype(t)::DT` is 0 or 1 -- so a launch is written once for both instantiations
template <class F> inline void with_dtype(int dtype, F f) {
    if (dtype == 0)
        f(Storage<0>());
    else
        f(Storage<1>());
}

// ---- the pointers of a correlation pyramid (at most four levels), by value in the kernel arguments ------------------------------------------
struct PyrPtrs {
    void *p[4];
};
struct PyrConstPtrs {
    const void *p[4];
};

// dst = the first `levels` entries of src, NULL above; false where a level that has columns (W2 >> l > 0) is NULL
template <class P, class S> inline bool pyr_ptrs(P &dst, S *const *src, int levels, int W2) {
    for (int l = 0; l < 4; l++) {
        dst.p[l] = l < levels ? src[l] : nullptr;
        if (l < levels && !dst.p[l] && (W2 >> l) > 0) return false;
    }
    return true;
}

// ---- host-side checks ------------------------------------------------------------------------------------------------------------------------
inline int launched(hipError_t e) { return e == hipSuccess ? GPSGS_OK : GPSGS_E_LAUNCH; }
inline int launched() { return launched(hipGetLastError()); }  // the return code of an entry point once its kernels are enqueued

inline size_t cdiv(size_t a, size_t b) { return (a + b - 1) / b; }
inline bool aligned(const void *p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }  // bytes a power of two; NULL is aligned

// N * H1 * W1 (non-negative ints) where an int holds it -- the sampling kernels index the (n, y, x) rows in int -- else -1; no intermediate
// product overflows
inline long long rows_in_int(int N, int H1, int W1) {
    const long long a = (long long)N * H1;  // < 2^62
    if (a == 0 || W1 == 0) return 0;
    if (a > 0x7fffffffLL) return -1;
    const long long t = a * W1;  // < 2^62
    return t > 0x7fffffffLL ? -1 : t;
}

// 2 * radius + 1 must fit an int
inline bool radius_ok(int radius) { return radius >= 0 && radius <= 0x3fffffff; }

// One thread per element in blocks of 256: does the block count of a * b * c * d elements (non-negative ints) fit a grid's x (<= 0x7fffffff)?
inline bool blocks_fit(int a, int b, int c, int d) {
    const unsigned long long cap = 0x7fffffffULL * 256;
    unsigned long long n = (unsigned long long)a * (unsigned long long)b;  // < 2^62
    if (n > cap) return false;
    n *= (unsigned long long)c;  // < 2^39 * 2^31
    if (n > cap) return false;
    return d == 0 || n <= cap / (unsigned long long)d;
}

}  // namespace
