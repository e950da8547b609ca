// group_norm.hip -- GroupNorm forward and backward for gfx950, split over the whole chip (DESIGN.md "GroupNorm").
//
// Contiguous NCHW.  A ROW is one (sample, group): L = (C/G) * H * W contiguous elements; a PLANE is one (sample, channel): HW elements.
// The networks around the rasteriser normalise groups of 8 channels x the whole image plane, so a tensor has 8..24 rows of 0.1..2 M elements:
// one workgroup per row leaves most of the 256 CUs idle.  Here every row (forward) / plane (backward) is cut into chunks of GN_CHUNK elements,
// one 256-thread workgroup per chunk, each thread holding its 32 elements in registers:
//   k_gn_moments    chunk -> {mean, M2 = sum (x - mean)^2} of the chunk.  Two passes over the REGISTERS (shifted sum for the mean, then the squared
//                   deviations from it), so a mean far larger than the spread costs nothing (no sum x^2 anywhere).
//   k_gn_apply      every workgroup combines its row's partials itself (Chan's formula in a fixed tree order: a few hundred values, read from L2,
//                   while its own x loads are in flight), then writes y = (x - mean) * rstd * gamma[c] + beta[c]; c follows the element index (a
//                   chunk may straddle channels).  The row's first workgroup stores mean / rstd for the backward.
//   k_gn_bwd_sums   chunk of a plane -> {sum dy, sum dy (x - mean)} (x relative to the row mean: the same robustness as the forward).
//   k_gn_bwd_apply  combines the partials of its group's planes (weighted by gamma) in a fixed order, forms the two group coefficients and writes
//                   dx = rstd gamma[c] dy + c1 (x - mean) + c2; a plane's first workgroup stores the plane's two sums.
//   k_gn_param_grad one thread per channel sums the planes' sums over n in index order -> dgamma, dbeta.
// No atomics; every sum has a fixed order (per-thread strided, xor tree over the wave, waves in index order): the same bits on every run.
// Loads and stores are 16 bytes per lane wherever an element index is a multiple of the vector width (all tensor pointers are 16-byte aligned);
// the ragged head and tail of a chunk (a row that starts off a 16-byte boundary, a length that is no multiple of 4 / 8) go element by element.
#include <hip/hip_fp16.h>

#include "gsr_common.h"

namespace {

constexpr int GN_CHUNK = 8192;               // elements per workgroup
constexpr int GN_THREADS = 256;              // 4 waves, one per SIMD
constexpr int GN_PT = GN_CHUNK / GN_THREADS;  // 32 elements per thread, all in registers

// x / dx in their storage type: DT 0 = fp32 (4 elements per 16 bytes), 1 = fp16 (8)
template <int DT> struct XT;
template <> struct XT<0> {
    typedef float T;
    static constexpr int V = 4;
    static __device__ __forceinline__ void load(const T *p, float (&v)[4]) {
        const float4 f = *reinterpret_cast<const float4 *>(p);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    }
    static __device__ __forceinline__ void store(T *p, const float (&v)[4]) { *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]); }
    static __device__ __forceinline__ float load1(const T *p) { return *p; }
    static __device__ __forceinline__ void store1(T *p, float v) { *p = v; }
};
template <> struct XT<1> {
    typedef __half T;
    static constexpr int V = 8;
    static __device__ __forceinline__ void load(const T *p, float (&v)[8]) {
        const uint4 u = *reinterpret_cast<const uint4 *>(p);
        const __half2 *h = reinterpret_cast<const __half2 *>(&u);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float2 f = __half22float2(h[q]);
            v[2 * q] = f.x; v[2 * q + 1] = f.y;
        }
    }
    static __device__ __forceinline__ void store(T *p, const float (&v)[8]) {  // one rounding per element
        uint4 u;
        __half2 *h = reinterpret_cast<__half2 *>(&u);
#pragma unroll
        for (int q = 0; q < 4; q++) h[q] = __floats2half2_rn(v[2 * q], v[2 * q + 1]);
        *reinterpret_cast<uint4 *>(p) = u;
    }
    static __device__ __forceinline__ float load1(const T *p) { return __half2float(*p); }
    static __device__ __forceinline__ void store1(T *p, float v) { *p = __float2half(v); }
};

// V consecutive fp32 (y, dy) at an element index that is a multiple of V
template <int V> __device__ __forceinline__ void load_f32(const float *p, float (&v)[V]) {
#pragma unroll
    for (int q = 0; q < V / 4; q++) {
        const float4 f = reinterpret_cast<const float4 *>(p)[q];
        v[4 * q] = f.x; v[4 * q + 1] = f.y; v[4 * q + 2] = f.z; v[4 * q + 3] = f.w;
    }
}
template <int V> __device__ __forceinline__ void store_f32(float *p, const float (&v)[V]) {
#pragma unroll
    for (int q = 0; q < V / 4; q++) reinterpret_cast<float4 *>(p)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}

// Elements [b, e) of the tensor (e - b <= GN_CHUNK) as: head [b, b + nh), nvec vectors of V from v0 (a multiple of V), tail [e - nt, e); nh, nt < V.
// Vector j * 256 + tid belongs to thread tid; head element k to thread k, tail element k to thread 64 + k (another wave).
struct Span {
    size_t b, e, v0;
    int nvec, nh, nt;
};
template <int V> __device__ __forceinline__ Span make_span(size_t b, size_t e) {
    Span s;
    size_t vb = (b + V - 1) / V * V, ve = e / V * V;
    if (vb > e) vb = e;
    if (ve < vb) ve = vb;
    s.b = b; s.e = e; s.v0 = vb;
    s.nvec = (int)((ve - vb) / V); s.nh = (int)(vb - b); s.nt = (int)(e - ve);
    return s;
}
__device__ __forceinline__ bool edge_index(const Span &s, int tid, size_t &idx) {
    if (tid < s.nh) { idx = s.b + tid; return true; }
    if (tid >= 64 && tid - 64 < s.nt) { idx = s.e - s.nt + (tid - 64); return true; }
    return false;
}

// sums of two values over the workgroup, the same for every thread: xor tree inside the wave, the four waves in index order
__device__ __forceinline__ float2 block_sum2(float a, float b, float2 *red /*[4]*/) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        a += __shfl_xor(a, d, 64);
        b += __shfl_xor(b, d, 64);
    }
    const int tid = threadIdx.x;
    __syncthreads();  // the previous use of red[] has been read
    if ((tid & 63) == 0) red[tid >> 6] = make_float2(a, b);
    __syncthreads();
    return make_float2((red[0].x + red[1].x) + (red[2].x + red[3].x), (red[0].y + red[1].y) + (red[2].y + red[3].y));
}

template <int DT>
__global__ __launch_bounds__(GN_THREADS) void k_gn_moments(const typename XT<DT>::T *__restrict__ x, int L, int chunks, float2 *__restrict__ partial) {
    constexpr int V = XT<DT>::V, NV = GN_PT / V;
    __shared__ float2 red[4];
    const int tid = threadIdx.x;
    const unsigned row = blockIdx.x / (unsigned)chunks, ck = blockIdx.x - row * (unsigned)chunks;
    const size_t r0 = (size_t)row * L, b = r0 + (size_t)ck * GN_CHUNK, e = min(b + (size_t)GN_CHUNK, r0 + (size_t)L);
    const Span s = make_span<V>(b, e);
    float v[NV][V], ev = 0.f;
#pragma unroll
    for (int j = 0; j < NV; j++)
        if (j * GN_THREADS + tid < s.nvec) XT<DT>::load(x + s.v0 + (size_t)(j * GN_THREADS + tid) * V, v[j]);
    size_t ei;
    const bool edge = edge_index(s, tid, ei);
    if (edge) ev = XT<DT>::load1(x + ei);
    const float x0 = XT<DT>::load1(x + b);  // the shift: sums of x - x0 keep their digits when |mean| >> spread
    float a = edge ? ev - x0 : 0.f;
#pragma unroll
    for (int j = 0; j < NV; j++)
        if (j * GN_THREADS + tid < s.nvec) {
#pragma unroll
            for (int k = 0; k < V; k++) a += v[j][k] - x0;
        }
    const float mean = x0 + block_sum2(a, 0.f, red).x / (float)(e - b);
    float q = edge ? (ev - mean) * (ev - mean) : 0.f;
#pragma unroll
    for (int j = 0; j < NV; j++)
        if (j * GN_THREADS + tid < s.nvec) {
#pragma unroll
            for (int k = 0; k < V; k++) q += (v[j][k] - mean) * (v[j][k] - mean);
        }
    const float m2 = block_sum2(q, 0.f, red).x;
    if (tid == 0) partial[blockIdx.x] = make_float2(mean, m2);
}

template <int DT>
__global__ __launch_bounds__(GN_THREADS) void k_gn_apply(const typename XT<DT>::T *__restrict__ x, const float *__restrict__ gamma,
                                                         const float *__restrict__ beta, const float2 *__restrict__ partial, int L, int chunks, int HW,
                                                         int cpg, int G, float eps, float *__restrict__ y, float *__restrict__ mean_out,
                                                         float *__restrict__ rstd_out) {
    constexpr int V = XT<DT>::V, NV = GN_PT / V;
    __shared__ float2 red[4];
    const int tid = threadIdx.x;
    const unsigned row = blockIdx.x / (unsigned)chunks, ck = blockIdx.x - row * (unsigned)chunks;
    const size_t r0 = (size_t)row * L, b = r0 + (size_t)ck * GN_CHUNK, e = min(b + (size_t)GN_CHUNK, r0 + (size_t)L);
    const Span s = make_span<V>(b, e);
    float v[NV][V], ev = 0.f;
#pragma unroll
    for (int j = 0; j < NV; j++)
        if (j * GN_THREADS + tid < s.nvec) XT<DT>::load(x + s.v0 + (size_t)(j * GN_THREADS + tid) * V, v[j]);
    size_t ei;
    const bool edge = edge_index(s, tid, ei);
    if (edge) ev = XT<DT>::load1(x + ei);

    // the row's moments from its chunks' {mean_i, M2_i} (Chan): mean = m0 + sum n_i (mean_i - m0) / L, M2 = sum M2_i + n_i (mean_i - mean)^2
    const float2 *pr = partial + (size_t)row * chunks;
    const float m0 = pr[0].x;
    float a = 0.f;
    for (int i = tid; i < chunks; i += GN_THREADS) {
        const float ni = (float)(i == chunks - 1 ? L - i * GN_CHUNK : GN_CHUNK);
        a += ni * (pr[i].x - m0);
    }
    const float mu = m0 + block_sum2(a, 0.f, red).x / (float)L;
    float q = 0.f;
    for (int i = tid; i < chunks; i += GN_THREADS) {
        const float ni = (float)(i == chunks - 1 ? L - i * GN_CHUNK : GN_CHUNK);
        const float2 p = pr[i];
        q += p.y + ni * (p.x - mu) * (p.x - mu);
    }
    const float var = block_sum2(q, 0.f, red).x / (float)L;
    const float rs = 1.0f / sqrtf(var + eps);
    if (ck == 0 && tid == 0) {
        mean_out[row] = mu;
        rstd_out[row] = rs;
    }

    const int c0 = (int)(row % (unsigned)G) * cpg;  // the row's first channel
#pragma unroll
    for (int j = 0; j < NV; j++) {
        const int vi = j * GN_THREADS + tid;
        if (vi < s.nvec) {
            const size_t i = s.v0 + (size_t)vi * V;
            const unsigned o = (unsigned)(i - r0), cc = o / (unsigned)HW, left = (unsigned)HW - (o - cc * (unsigned)HW);  // elements left in the plane
            float out[V];
            if (left >= (unsigned)V) {
                const float g = gamma[c0 + cc], bt = beta[c0 + cc];
#pragma unroll
                for (int k = 0; k < V; k++) out[k] = (v[j][k] - mu) * rs * g + bt;
            } else {
#pragma unroll
                for (int k = 0; k < V; k++) {
                    const unsigned c = c0 + (o + k) / (unsigned)HW;
                    out[k] = (v[j][k] - mu) * rs * gamma[c] + beta[c];
                }
            }
            store_f32<V>(y + i, out);
        }
    }
    if (edge) {
        const unsigned c = c0 + (unsigned)(ei - r0) / (unsigned)HW;
        y[ei] = (ev - mu) * rs * gamma[c] + beta[c];
    }
}

template <int DT>
__global__ __launch_bounds__(GN_THREADS) void k_gn_bwd_sums(const typename XT<DT>::T *__restrict__ x, const float *__restrict__ dy,
                                                            const float *__restrict__ mean, int HW, int chunks, int C, int cpg, int G,
                                                            float2 *__restrict__ partial) {
    constexpr int V = XT<DT>::V, NV = GN_PT / V;
    __shared__ float2 red[4];
    const int tid = threadIdx.x;
    const unsigned plane = blockIdx.x / (unsigned)chunks, ck = blockIdx.x - plane * (unsigned)chunks;
    const unsigned n = plane / (unsigned)C, c = plane - n * (unsigned)C;
    const float mu = mean[(size_t)n * G + c / (unsigned)cpg];
    const size_t p0 = (size_t)plane * HW, b = p0 + (size_t)ck * GN_CHUNK, e = min(b + (size_t)GN_CHUNK, p0 + (size_t)HW);
    const Span s = make_span<V>(b, e);
    float xv[NV][V], gv[NV][V];  // every load of the chunk is issued before the first sum waits for one
#pragma unroll
    for (int j = 0; j < NV; j++) {
        const int vi = j * GN_THREADS + tid;
        if (vi < s.nvec) {
            XT<DT>::load(x + s.v0 + (size_t)vi * V, xv[j]);
            load_f32<V>(dy + s.v0 + (size_t)vi * V, gv[j]);
        }
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NV; j++)
        if (j * GN_THREADS + tid < s.nvec) {
#pragma unroll
            for (int k = 0; k < V; k++) {
                s1 += gv[j][k];
                s2 += gv[j][k] * (xv[j][k] - mu);
            }
        }
    size_t ei;
    if (edge_index(s, tid, ei)) {
        const float g = dy[ei];
        s1 += g;
        s2 += g * (XT<DT>::load1(x + ei) - mu);
    }
    const float2 t = block_sum2(s1, s2, red);
    if (tid == 0) partial[blockIdx.x] = t;
}

// gchunks = chunks (one workgroup per chunk, dx written) or 1 (dx not wanted: one workgroup per plane, which only stores the plane's sums)
template <int DT>
__global__ __launch_bounds__(GN_THREADS) void k_gn_bwd_apply(const typename XT<DT>::T *__restrict__ x, const float *__restrict__ dy,
                                                             const float *__restrict__ gamma, const float *__restrict__ mean,
                                                             const float *__restrict__ rstd, const float2 *__restrict__ partial, int HW, int chunks,
                                                             int gchunks, int C, int cpg, int G, typename XT<DT>::T *__restrict__ dx,
                                                             float2 *__restrict__ sums) {
    constexpr int V = XT<DT>::V, NV = GN_PT / V;
    __shared__ float2 red[4];
    const int tid = threadIdx.x;
    const unsigned plane = blockIdx.x / (unsigned)gchunks, ck = blockIdx.x - plane * (unsigned)gchunks;
    if (ck == 0) {  // the plane's own two sums, for k_gn_param_grad
        float a = 0.f, bb = 0.f;
        const float2 *pp = partial + (size_t)plane * chunks;
        for (int i = tid; i < chunks; i += GN_THREADS) {
            a += pp[i].x;
            bb += pp[i].y;
        }
        const float2 t = block_sum2(a, bb, red);
        if (tid == 0) sums[plane] = t;
    }
    if (dx == nullptr) return;
    const unsigned n = plane / (unsigned)C, c = plane - n * (unsigned)C, g = c / (unsigned)cpg;
    const size_t p0 = (size_t)plane * HW, b = p0 + (size_t)ck * GN_CHUNK, e = min(b + (size_t)GN_CHUNK, p0 + (size_t)HW);
    const Span s = make_span<V>(b, e);
    float xv[NV][V], gv[NV][V], ex = 0.f, eg = 0.f;
#pragma unroll
    for (int j = 0; j < NV; j++) {
        const int vi = j * GN_THREADS + tid;
        if (vi < s.nvec) {
            XT<DT>::load(x + s.v0 + (size_t)vi * V, xv[j]);
            load_f32<V>(dy + s.v0 + (size_t)vi * V, gv[j]);
        }
    }
    size_t ei;
    const bool edge = edge_index(s, tid, ei);
    if (edge) {
        ex = XT<DT>::load1(x + ei);
        eg = dy[ei];
    }
    // the group's sums: sum_c gamma[c] sum dy, sum_c gamma[c] sum dy (x - mean) over the group's cpg planes x chunks partials, in a fixed order
    const float2 *pg = partial + ((size_t)n * C + (size_t)g * cpg) * chunks;
    const float *gg = gamma + (size_t)g * cpg;
    const int cnt = cpg * chunks;
    float a = 0.f, bb = 0.f;
    for (int i = tid; i < cnt; i += GN_THREADS) {
        const float w = gg[i / chunks];
        const float2 p = pg[i];
        a += w * p.x;
        bb += w * p.y;
    }
    const float2 t = block_sum2(a, bb, red);
    const size_t row = (size_t)n * G + g;
    const float mu = mean[row], rs = rstd[row], m = (float)cpg * (float)HW;
    const float kd = rs * gamma[c], c1 = -(rs * rs * rs) * t.y / m, c2 = -rs * t.x / m;
#pragma unroll
    for (int j = 0; j < NV; j++) {
        const int vi = j * GN_THREADS + tid;
        if (vi < s.nvec) {
            float out[V];
#pragma unroll
            for (int k = 0; k < V; k++) out[k] = kd * gv[j][k] + c1 * (xv[j][k] - mu) + c2;
            XT<DT>::store(dx + s.v0 + (size_t)vi * V, out);
        }
    }
    if (edge) XT<DT>::store1(dx + ei, kd * eg + c1 * (ex - mu) + c2);
}

__global__ __launch_bounds__(GN_THREADS) void k_gn_param_grad(const float2 *__restrict__ sums, const float *__restrict__ rstd, int N, int C, int cpg,
                                                              int G, float *__restrict__ dgamma, float *__restrict__ dbeta) {
    const int c = blockIdx.x * GN_THREADS + threadIdx.x;
    if (c >= C) return;
    float dg = 0.f, db = 0.f;
    for (int n = 0; n < N; n++) {
        const float2 s = sums[(size_t)n * C + c];
        dg += rstd[(size_t)n * G + c / cpg] * s.y;
        db += s.x;
    }
    dgamma[c] = dg;
    dbeta[c] = db;
}

inline size_t cdiv(size_t a, size_t b) { return (a + b - 1) / b; }
inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// common argument checks: 0 = go on, 1 = nothing to do, < 0 = refused
int gn_check(int dtype, int N, int C, int G, int HW) {
    if (N < 0 || C < 0 || HW < 0 || G <= 0 || (dtype != 0 && dtype != 1) || C % G != 0) return GPSGS_E_INVALID;
    if ((size_t)N * C * HW == 0) return 1;
    if ((size_t)(C / G) * HW > 0x7fffffffu || (size_t)N * C * cdiv(HW, GN_CHUNK) > 0x7fffffffu ||
        (size_t)N * G * cdiv((size_t)(C / G) * HW, GN_CHUNK) > 0x7fffffffu)
        return GPSGS_E_INVALID;
    return 0;
}

}  // namespace

extern "C" size_t gn_chunk_elems(void) { return GN_CHUNK; }

extern "C" size_t gn_scratch_bytes(int N, int C, int G, int HW) {
    if (N < 0 || C < 0 || HW < 0 || G <= 0) return 0;
    const size_t rows = cdiv((size_t)C * HW, GN_CHUNK) + (size_t)G, planes = (size_t)C * cdiv(HW, GN_CHUNK);
    return 8 * (size_t)N * ((size_t)C + (rows > planes ? rows : planes));
}

extern "C" int gn_forward(const void *x, int dtype, const float *gamma, const float *beta, int N, int C, int G, int HW, float eps, float *y,
                          float *mean, float *rstd, void *scratch, void *stream) {
    const int rc = gn_check(dtype, N, C, G, HW);
    if (rc != 0) return rc < 0 ? rc : GPSGS_OK;
    if (!x || !gamma || !beta || !y || !mean || !rstd || !scratch) return GPSGS_E_INVALID;
    if (!aligned16(x) || !aligned16(y) || ((uintptr_t)scratch & 7) != 0) return GPSGS_E_INVALID;
    const int cpg = C / G, L = cpg * HW, chunks = (int)cdiv(L, GN_CHUNK);
    const dim3 grid((unsigned)((size_t)N * G * chunks)), block(GN_THREADS);
    float2 *partial = (float2 *)scratch + (size_t)N * C;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == 0) {
        hipLaunchKernelGGL(k_gn_moments<0>, grid, block, 0, s, (const float *)x, L, chunks, partial);
        hipLaunchKernelGGL(k_gn_apply<0>, grid, block, 0, s, (const float *)x, gamma, beta, (const float2 *)partial, L, chunks, HW, cpg, G, eps, y, mean, rstd);
    } else {
        hipLaunchKernelGGL(k_gn_moments<1>, grid, block, 0, s, (const __half *)x, L, chunks, partial);
        hipLaunchKernelGGL(k_gn_apply<1>, grid, block, 0, s, (const __half *)x, gamma, beta, (const float2 *)partial, L, chunks, HW, cpg, G, eps, y, mean, rstd);
    }
    return hipGetLastError() == hipSuccess ? GPSGS_OK : GPSGS_E_LAUNCH;
}

extern "C" int gn_backward(const void *x, int dtype, const float *dy, const float *gamma, const float *mean, const float *rstd, int N, int C, int G,
                           int HW, void *dx, float *dgamma, float *dbeta, void *scratch, void *stream) {
    const int rc = gn_check(dtype, N, C, G, HW);
    if (rc < 0) return rc;
    if ((dgamma != nullptr) != (dbeta != nullptr)) return GPSGS_E_INVALID;
    if (rc != 0) return GPSGS_OK;
    if (!x || !dy || !gamma || !mean || !rstd || !scratch) return GPSGS_E_INVALID;
    if (!aligned16(x) || !aligned16(dy) || !aligned16(dx) || ((uintptr_t)scratch & 7) != 0) return GPSGS_E_INVALID;
    if (!dx && !dgamma) return GPSGS_OK;
    const int cpg = C / G, chunks = (int)cdiv(HW, GN_CHUNK), gchunks = dx ? chunks : 1;
    const dim3 block(GN_THREADS);
    float2 *sums = (float2 *)scratch, *partial = sums + (size_t)N * C;
    hipStream_t s = (hipStream_t)stream;
    const unsigned planes = (unsigned)N * (unsigned)C;
    if (dtype == 0) {
        hipLaunchKernelGGL(k_gn_bwd_sums<0>, dim3(planes * chunks), block, 0, s, (const float *)x, dy, mean, HW, chunks, C, cpg, G, partial);
        hipLaunchKernelGGL(k_gn_bwd_apply<0>, dim3(planes * gchunks), block, 0, s, (const float *)x, dy, gamma, mean, rstd, (const float2 *)partial, HW,
                           chunks, gchunks, C, cpg, G, (float *)dx, sums);
    } else {
        hipLaunchKernelGGL(k_gn_bwd_sums<1>, dim3(planes * chunks), block, 0, s, (const __half *)x, dy, mean, HW, chunks, C, cpg, G, partial);
        hipLaunchKernelGGL(k_gn_bwd_apply<1>, dim3(planes * gchunks), block, 0, s, (const __half *)x, dy, gamma, mean, rstd, (const float2 *)partial, HW,
                           chunks, gchunks, C, cpg, G, (__half *)dx, sums);
    }
    if (dgamma)
        hipLaunchKernelGGL(k_gn_param_grad, dim3((unsigned)cdiv(C, GN_THREADS)), block, 0, s, (const float2 *)sums, rstd, N, C, cpg, G, dgamma, dbeta);
    return hipGetLastError() == hipSuccess ? GPSGS_OK : GPSGS_E_LAUNCH;
}
