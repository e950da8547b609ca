// corr_sampler.hip -- 1-D correlation lookup for RAFT-Stereo on gfx950: the exact-arithmetic sampling unit (no FMA contraction, by flag).
//
//   cs_forward / cs_backward                 one volume (replaces the `corr_sampler` CUDA extension called at /root/reference/core/corr.py:22,28;
//                                            semantics = CorrBlock1D, /root/reference/core/corr.py:127-146, i.e. linear interpolation of the
//                                            2r+1 taps x0-r..x0+r along W2 with zero padding)
//   cs_lookup_forward / cs_lookup_backward   the same lookup in ALL pyramid levels in one launch, written straight into the concatenated
//                                            [N, L*(2r+1), H, W] tensor (core/corr.py:44-51: CorrBlockFast1D.__call__)
// The two are interchangeable to the reference, so their bits must agree: all four kernels run the same two functions, sample_row and tap_grad.
//
// Forward: one thread per (n,y,x): 2r+2 contiguous reads of its volume row, 2r+1 stores coalesced along x.
// Backward: grad_volume row (n,y,x,:) is owned by exactly one (n,y,x), so there is no scatter and no atomic: one
// thread per grad_volume ELEMENT writes either zero or the sum of its (at most two) taps -- stores are fully
// coalesced along W2 and the zero-fill is fused (no separate memset).
#include "op_common.h"

#pragma clang fp contract(off)

namespace {

// ---- the sampling core ------------------------------------------------------------------------------------------------------------------------
// Forward of one level: the 2r+1 taps x0-r .. x0+r of the volume row v (w wide, zero outside), linearly interpolated, to o[k * hw]
template <typename T> __device__ __forceinline__ void sample_row(const T *v, int w, float x0, int r, T *o, int hw) {
    const float fl = floorf(x0);
    const float dx = x0 - fl;
    const int xs = (int)fl - r;
    const int rd = 2 * r + 1;
    float prev = (xs >= 0 && xs < w) ? ldf(v + xs) : 0.f;
    for (int k = 0; k < rd; k++) {
        const int x1 = xs + k + 1;
        const float next = (x1 >= 0 && x1 < w) ? ldf(v + x1) : 0.f;
        stf(o + (size_t)k * hw, prev * (1.0f - dx) + next * dx);
        prev = next;
    }
}

// Backward of one volume element: i = its tap index x1 - (floor(x0) - r).  Tap i - 1 read it with weight dx and tap i with 1 - dx, where those
// taps exist (0 .. rd-1): `below` and `at` are their grad_out values.  The two products are added in this order everywhere.
__device__ __forceinline__ float tap_grad(int i, int rd, float dx, float below, float at) {
    float g = 0.f;
    if (i >= 0 && i <= rd) {
        if (i > 0) g += below * dx;
        if (i < rd) g += at * (1.0f - dx);
    }
    return g;
}
// The same sum with the taps still in memory, each loaded only where it exists: grad_out is [N][levels][rd][hw], the element belongs to row yx of
// level l of sample n (the single-volume sampler is levels = 1, l = 0).  The row's offset is formed inside the guard, as the kernels always did:
// the compiler uses rd >= i >= 0 for it.
template <typename T> __device__ __forceinline__ float tap_grad(int i, int rd, float dx, const T *grad_out, int n, int levels, int l, int hw, int yx) {
    float g = 0.f;
    if (i >= 0 && i <= rd) {
        const T *go = grad_out + ((size_t)n * levels * rd + (size_t)l * rd) * hw + yx;
        if (i > 0) g += ldf(go + (size_t)(i - 1) * hw) * dx;
        if (i < rd) g += ldf(go + (size_t)i * hw) * (1.0f - dx);
    }
    return g;
}

template <typename T>
__global__ __launch_bounds__(256) void k_cs_fwd(const T *__restrict__ volume, const float *__restrict__ coords, T *__restrict__ out,
                                                int total, int H1, int W1, int W2, int r) {
    const int idx = blockIdx.x * 256 + threadIdx.x;  // (n*H1 + y)*W1 + x
    if (idx >= total) return;
    const int hw = H1 * W1;
    const int n = idx / hw, yx = idx - n * hw;
    const int rd = 2 * r + 1;
    sample_row(volume + (size_t)idx * W2, W2, coords[idx], r, out + (size_t)n * rd * hw + yx, hw);
}

template <typename T>
__global__ __launch_bounds__(256) void k_cs_bwd(const float *__restrict__ coords, const T *__restrict__ grad_out,
                                                T *__restrict__ grad_volume, size_t total, int H1, int W1, int W2, int r) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;  // ((n*H1 + y)*W1 + x)*W2 + x1
    if (e >= total) return;
    const int x1 = (int)(e % W2);
    const size_t idx = e / W2;
    const int hw = H1 * W1;
    const int n = (int)(idx / hw), yx = (int)(idx - (size_t)n * hw);
    const float x0 = coords[idx];
    const float fl = floorf(x0);
    const float dx = x0 - fl;
    const int rd = 2 * r + 1;
    const int i = x1 - ((int)fl - r);
    stf(grad_volume + e, tap_grad(i, rd, dx, grad_out, n, 1, 0, hw, yx));
}

// Same result, four consecutive x1 per thread (W2 % 4 == 0: every pyramid level of the reference's shapes): one coords load, at most five
// grad_out loads and ONE 16-byte (fp32) / 8-byte (fp16) store per thread instead of four of each -- the kernel is a pure store stream
// (grad_volume is 3.6x the bytes of everything it reads).  Per element tap_grad runs on the loaded taps.
template <typename T> struct Vec4;
template <> struct Vec4<float> { typedef float4 type; };
template <> struct Vec4<__half> { typedef uint2 type; };
__device__ __forceinline__ float4 pack4(const float (&g)[4], float) { return make_float4(g[0], g[1], g[2], g[3]); }
__device__ __forceinline__ uint2 pack4(const float (&g)[4], __half) {
    const __half2 a = __halves2half2(__float2half(g[0]), __float2half(g[1])), b = __halves2half2(__float2half(g[2]), __float2half(g[3]));
    return make_uint2(*reinterpret_cast<const uint32_t *>(&a), *reinterpret_cast<const uint32_t *>(&b));
}
template <typename T>
__global__ __launch_bounds__(256) void k_cs_bwd4(const float *__restrict__ coords, const T *__restrict__ grad_out,
                                                 T *__restrict__ grad_volume, size_t total4, int H1, int W1, int W2, int r) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;  // quad index: (((n*H1 + y)*W1 + x)*W2 + x1) / 4
    if (q >= total4) return;
    const int wq = W2 >> 2;
    const int x1 = (int)(q % wq) * 4;
    const size_t idx = q / wq;
    const int hw = H1 * W1;
    const int n = (int)(idx / hw), yx = (int)(idx - (size_t)n * hw);
    const float x0 = coords[idx];
    const float fl = floorf(x0);
    const float dx = x0 - fl;
    const int rd = 2 * r + 1;
    const int i0 = x1 - ((int)fl - r);  // tap index of the first element
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    if (i0 + 3 >= 0 && i0 <= rd) {
        const T *go = grad_out + (size_t)n * rd * hw + yx;
        float t[5];  // grad_out taps i0-1 .. i0+3 (zero outside 0..rd-1: those terms are skipped below, as in k_cs_bwd)
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const int i = i0 - 1 + k;
            t[k] = (i >= 0 && i < rd) ? ldf(go + (size_t)i * hw) : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) g[k] = tap_grad(i0 + k, rd, dx, t[k], t[k + 1]);
    }
    *reinterpret_cast<typename Vec4<T>::type *>(grad_volume + q * 4) = pack4(g, T());
}

// ---- fused multi-level lookup: the same per level, level l of a pyramid is W2 >> l wide and sampled at coords / 2^l ----------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_lookup_fwd(PyrConstPtrs pyr, const float *__restrict__ coords, T *__restrict__ out, int total, int H1,
                                                    int W1, int W2, int levels, int r) {
    const int idx = blockIdx.x * 256 + threadIdx.x;  // (n*H1 + y)*W1 + x
    if (idx >= total) return;
    const int hw = H1 * W1;
    const int n = idx / hw, yx = idx - n * hw;
    const int rd = 2 * r + 1;
    const float x = coords[idx];
    int wl = W2;
    float inv = 1.f;
    for (int l = 0; l < levels; l++) {
        T *o = out + ((size_t)n * levels * rd + (size_t)l * rd) * hw + yx;
        sample_row(reinterpret_cast<const T *>(pyr.p[l]) + (size_t)idx * wl, wl, x * inv, r, o, hw);  // coords / 2^l is exact
        wl >>= 1;
        inv *= 0.5f;
    }
}

// one thread per level-0 COLUMN position e = (row idx, c): writes element c of every level whose row is at least c+1 wide
// (each gradient row is owned by one (n, y, x), so there is no scatter and the zero fill is fused)
template <typename T>
__global__ __launch_bounds__(256) void k_lookup_bwd(const float *__restrict__ coords, const T *__restrict__ grad_out, PyrPtrs gpyr, size_t total,
                                                    int H1, int W1, int W2, int levels, int r) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % W2);
    const size_t idx = e / W2;
    const int hw = H1 * W1;
    const int n = (int)(idx / hw), yx = (int)(idx - (size_t)n * hw);
    const int rd = 2 * r + 1;
    const float x = coords[idx];
    int wl = W2;
    float inv = 1.f;
    for (int l = 0; l < levels; l++) {
        if (c < wl) {
            const float x0 = x * inv;
            const float fl = floorf(x0);
            const float dx = x0 - fl;
            const int i = c - ((int)fl - r);
            const float g = tap_grad(i, rd, dx, grad_out, n, levels, l, hw, yx);
            stf(reinterpret_cast<T *>(gpyr.p[l]) + idx * wl + c, g);
        }
        wl >>= 1;
        inv *= 0.5f;
    }
}

}  // namespace

// the arguments the four entry points share
static bool sampler_args_ok(int N, int H1, int W1, int W2, int radius, int dtype) {
    return N >= 0 && H1 >= 0 && W1 >= 0 && W2 >= 0 && radius_ok(radius) && dtype_ok(dtype);
}

extern "C" int cs_forward(const void *volume, const float *coords, void *out, int N, int H1, int W1, int W2, int radius, int dtype,
                          void *stream) {
    if (!sampler_args_ok(N, H1, W1, W2, radius, dtype)) return GPSGS_E_INVALID;
    const long long total = rows_in_int(N, H1, W1);
    if (total == 0) return GPSGS_OK;
    if (!volume || !coords || !out || total < 0) return GPSGS_E_INVALID;
    with_dtype(dtype, [&](auto t) {
        typedef typename decltype(t)::T T;
        hipLaunchKernelGGL(k_cs_fwd<T>, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, (const T *)volume, coords, (T *)out,
                           (int)total, H1, W1, W2, radius);
    });
    return launched();
}

extern "C" int cs_backward(const float *coords, const void *grad_out, void *grad_volume, int N, int H1, int W1, int W2, int radius,
                           int dtype, void *stream) {
    if (!sampler_args_ok(N, H1, W1, W2, radius, dtype)) return GPSGS_E_INVALID;
    const long long rows = rows_in_int(N, H1, W1);
    if (rows == 0 || W2 == 0) return GPSGS_OK;
    if (!coords || !grad_out || !grad_volume || rows < 0) return GPSGS_E_INVALID;
    const size_t total = (size_t)rows * W2;  // < 2^62
    // one thread per quad (k_cs_bwd4) or per element (k_cs_bwd) in blocks of 256: a block count a grid's x cannot hold is refused, not truncated
    const bool quads = (W2 & 3) == 0 && aligned(grad_volume, 16);
    const size_t threads = quads ? total / 4 : total;
    const size_t blocks = cdiv(threads, 256);
    if (blocks > 0x7fffffffULL) return GPSGS_E_INVALID;
    with_dtype(dtype, [&](auto t) {
        typedef typename decltype(t)::T T;
        hipLaunchKernelGGL((quads ? k_cs_bwd4<T> : k_cs_bwd<T>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, coords, (const T *)grad_out,
                           (T *)grad_volume, threads, H1, W1, W2, radius);
    });
    return launched();
}

extern "C" int cs_lookup_forward(const void *const *pyramid, const float *coords, void *out, int N, int H1, int W1, int W2, int levels, int radius,
                                 int dtype, void *stream) {
    if (!sampler_args_ok(N, H1, W1, W2, radius, dtype) || levels < 1 || levels > 4 || !pyramid) return GPSGS_E_INVALID;
    const long long total = rows_in_int(N, H1, W1);
    if (total == 0) return GPSGS_OK;
    if (!coords || !out || total < 0) return GPSGS_E_INVALID;
    PyrConstPtrs pp;
    if (!pyr_ptrs(pp, pyramid, levels, W2)) return GPSGS_E_INVALID;
    with_dtype(dtype, [&](auto t) {
        typedef typename decltype(t)::T T;
        hipLaunchKernelGGL(k_lookup_fwd<T>, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, pp, coords, (T *)out, (int)total, H1,
                           W1, W2, levels, radius);
    });
    return launched();
}

extern "C" int cs_lookup_backward(const float *coords, const void *grad_out, void *const *grad_pyramid, int N, int H1, int W1, int W2, int levels,
                                  int radius, int dtype, void *stream) {
    if (!sampler_args_ok(N, H1, W1, W2, radius, dtype) || levels < 1 || levels > 4 || !grad_pyramid) return GPSGS_E_INVALID;
    const long long rows = rows_in_int(N, H1, W1);
    if (rows == 0 || W2 == 0) return GPSGS_OK;
    if (!coords || !grad_out || rows < 0) return GPSGS_E_INVALID;
    const size_t total = (size_t)rows * W2;  // < 2^62
    const size_t blocks = cdiv(total, 256);  // one thread per level-0 element in blocks of 256
    if (blocks > 0x7fffffffULL) return GPSGS_E_INVALID;  // more than a grid's x holds: refused, not truncated
    PyrPtrs pp;
    if (!pyr_ptrs(pp, grad_pyramid, levels, W2)) return GPSGS_E_INVALID;
    with_dtype(dtype, [&](auto t) {
        typedef typename decltype(t)::T T;
        hipLaunchKernelGGL(k_lookup_bwd<T>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, coords, (const T *)grad_out, pp, total, H1, W1,
                           W2, levels, radius);
    });
    return launched();
}
