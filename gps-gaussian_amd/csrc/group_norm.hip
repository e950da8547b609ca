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
//
// EPILOGUES (template parameter EP of k_gn_apply / k_gn_bwd_sums / k_gn_bwd_apply; gne_forward / gne_backward): what the reference's extractor runs
// after every one of these layers, folded into the same passes --
//   EP_NONE           out = y                               the kernels above, bit for bit
//   EP_RELU           out = relu(y)                         relu_(norm(conv(x)))
//   EP_RELU_ADD_RELU  out = relu(res + relu(y))             relu(x + relu_(norm2(...))), res fp32 of x's shape
// Backward: g = dout masked by the OUTER sign, read from the saved out (the next convolution keeps it alive anyway); dres = g; dy = g masked by the
// INNER sign, recomputed from x, mean, rstd, gamma, beta with the forward's own expression GN_Y (same bits as the forward stored, so no normalised
// activation is kept); the GroupNorm backward then runs on dy inside the same two kernels.  The masks are ATen's threshold_backward (v <= 0 -> +0.0f),
// the sums keep their order: the result is bit for bit what relu_ / add / relu around the EP_NONE kernels give.
#include <type_traits>

#include "op_common.h"

namespace {

constexpr int GN_CHUNK = 8192;               // elements per workgroup
constexpr int GN_THREADS = 256;              // 4 waves, one per SIMD
constexpr int GN_PT = GN_CHUNK / GN_THREADS;  // 32 elements per thread, all in registers

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

enum { EP_NONE = 0, EP_RELU = 1, EP_RELU_ADD_RELU = 2 };

// The arithmetic every instantiation shares: the forward's y (which the backward evaluates again for the inner sign), the two backward sums and dx.
// The EP_NONE instantiations keep the expressions as plain text (macros, not functions: they must compile to the instructions they always were, and
// even a helper inlined in another order changes their schedule); the compiler contracts them to
//     y  = fma((x - mu) * rs, g, bt)      dx = fma(kd, dy, c1 * d) + c2      s2 = s2 + dy * d  (NOT fused)
// The epilogue instantiations spell exactly that out, because left alone the compiler picks another contraction for the same text once a select
// feeds it (dx became fma(c1, d, kd * dy) + c2): their bits must be those of relu_ / add / relu around the EP_NONE kernels.
__device__ __forceinline__ float gn_y_fused(float x, float mu, float rs, float g, float bt) { return __fmaf_rn((x - mu) * rs, g, bt); }
__device__ __forceinline__ float gn_dx_fused(float kd, float dy, float c1, float d, float c2) { return __fmaf_rn(kd, dy, c1 * d) + c2; }
__device__ __forceinline__ void gn_acc_fused(float &s1, float &s2, float dy, float d) {
#pragma clang fp contract(off)
    s1 += dy;
    s2 += dy * d;
}
#define GN_Y(x, mu, rs, g, bt) (EP == EP_NONE ? (((x) - (mu)) * (rs) * (g) + (bt)) : gn_y_fused((x), (mu), (rs), (g), (bt)))
#define GN_DX(kd, dy, c1, d, c2) (EP == EP_NONE ? ((kd) * (dy) + (c1) * (d) + (c2)) : gn_dx_fused((kd), (dy), (c1), (d), (c2)))
__device__ __forceinline__ float relu_f(float v) { return v < 0.f ? 0.f : v; }                  // NaN goes through, as ATen's clamp_min
__device__ __forceinline__ float mask_f(float sign, float g) { return sign <= 0.f ? 0.f : g; }   // threshold_backward(g, sign, 0): +0.0f where masked
template <int EP> __device__ __forceinline__ float gn_epilogue(float y, float r) { return EP == EP_RELU ? relu_f(y) : relu_f(r + relu_f(y)); }
#define GN_OUT(y, r) (EP == EP_NONE ? (y) : gn_epilogue<EP>((y), (r)))

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
__global__ __launch_bounds__(GN_THREADS) void k_gn_moments(const typename Storage<DT>::T *__restrict__ x, int L, int chunks, float2 *__restrict__ partial) {
    constexpr int V = Storage<DT>::V, NV = GN_PT / V;
    __shared__ float2 red[4];
    const int tid = threadIdx.x;
    const unsigned row = blockIdx.x / (unsigned)chunks, ck = blockIdx.x - row * (unsigned)chunks;
    const size_t r0 = (size_t)row * L, b = r0 + (size_t)ck * GN_CHUNK, e = min(b + (size_t)GN_CHUNK, r0 + (size_t)L);
    const Span s = make_span<V>(b, e);
    float v[NV][V], ev = 0.f;
#pragma unroll
    for (int j = 0; j < NV; j++)
        if (j * GN_THREADS + tid < s.nvec) Storage<DT>::load(x + s.v0 + (size_t)(j * GN_THREADS + tid) * V, v[j]);
    size_t ei;
    const bool edge = edge_index(s, tid, ei);
    if (edge) ev = Storage<DT>::load1(x + ei);
    const float x0 = Storage<DT>::load1(x + b);  // the shift: sums of x - x0 keep their digits when |mean| >> spread
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

// res: the residual of EP_RELU_ADD_RELU (not read otherwise)
template <int DT, int EP>
__global__ __launch_bounds__(GN_THREADS) void k_gn_apply(const typename Storage<DT>::T *__restrict__ x, const float *__restrict__ gamma,
                                                         const float *__restrict__ beta, const float2 *__restrict__ partial, int L, int chunks, int HW,
                                                         int cpg, int G, float eps, float *__restrict__ y, float *__restrict__ mean_out,
                                                         float *__restrict__ rstd_out, const float *__restrict__ res) {
    constexpr int V = Storage<DT>::V, NV = GN_PT / V;
    constexpr bool RES = EP == EP_RELU_ADD_RELU;
    __shared__ float2 red[4];
    const int tid = threadIdx.x;
    const unsigned row = blockIdx.x / (unsigned)chunks, ck = blockIdx.x - row * (unsigned)chunks;
    const size_t r0 = (size_t)row * L, b = r0 + (size_t)ck * GN_CHUNK, e = min(b + (size_t)GN_CHUNK, r0 + (size_t)L);
    const Span s = make_span<V>(b, e);
    float v[NV][V], ev = 0.f;
#pragma unroll
    for (int j = 0; j < NV; j++)
        if (j * GN_THREADS + tid < s.nvec) Storage<DT>::load(x + s.v0 + (size_t)(j * GN_THREADS + tid) * V, v[j]);
    size_t ei;
    const bool edge = edge_index(s, tid, ei);
    if (edge) ev = Storage<DT>::load1(x + ei);
    float rv[RES ? NV : 1][V], er = 0.f;  // the residual's loads are in flight with x's, over the combine below
    if constexpr (RES) {
#pragma unroll
        for (int j = 0; j < NV; j++)
            if (j * GN_THREADS + tid < s.nvec) load_f32<V>(res + s.v0 + (size_t)(j * GN_THREADS + tid) * V, rv[j]);
        if (edge) er = res[ei];
    }

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
                for (int k = 0; k < V; k++) out[k] = GN_OUT(GN_Y(v[j][k], mu, rs, g, bt), rv[RES ? j : 0][k]);
            } else {
#pragma unroll
                for (int k = 0; k < V; k++) {
                    const unsigned c = c0 + (o + k) / (unsigned)HW;
                    out[k] = GN_OUT(GN_Y(v[j][k], mu, rs, gamma[c], beta[c]), rv[RES ? j : 0][k]);
                }
            }
            store_f32<V>(y + i, out);
        }
    }
    if (edge) {
        const unsigned c = c0 + (unsigned)(ei - r0) / (unsigned)HW;
        y[ei] = GN_OUT(GN_Y(ev, mu, rs, gamma[c], beta[c]), er);
    }
}

// EP != EP_NONE: `dy` is the gradient of the epilogue's output; it is masked here, element by element, to the gradient of y (see the top of the file).
// out: the forward's output, read by EP_RELU_ADD_RELU only.
template <int DT, int EP>
__global__ __launch_bounds__(GN_THREADS) void k_gn_bwd_sums(const typename Storage<DT>::T *__restrict__ x, const float *__restrict__ dy,
                                                            const float *__restrict__ mean, int HW, int chunks, int C, int cpg, int G,
                                                            float2 *__restrict__ partial, const float *__restrict__ gamma,
                                                            const float *__restrict__ beta, const float *__restrict__ rstd,
                                                            const float *__restrict__ out) {
    constexpr int V = Storage<DT>::V, NV = GN_PT / V;
    constexpr bool RES = EP == EP_RELU_ADD_RELU;
    __shared__ float2 red[4];
    const int tid = threadIdx.x;
    const unsigned plane = blockIdx.x / (unsigned)chunks, ck = blockIdx.x - plane * (unsigned)chunks;
    const unsigned n = plane / (unsigned)C, c = plane - n * (unsigned)C;
    const float mu = mean[(size_t)n * G + c / (unsigned)cpg];
    float rs = 0.f, gm = 0.f, bt = 0.f;
    if constexpr (EP != EP_NONE) {
        rs = rstd[(size_t)n * G + c / (unsigned)cpg];
        gm = gamma[c];
        bt = beta[c];
    }
    const size_t p0 = (size_t)plane * HW, b = p0 + (size_t)ck * GN_CHUNK, e = min(b + (size_t)GN_CHUNK, p0 + (size_t)HW);
    const Span s = make_span<V>(b, e);
    float xv[NV][V], gv[NV][V];  // every load of the chunk is issued before the first sum waits for one
    float ov[RES ? NV : 1][V];
#pragma unroll
    for (int j = 0; j < NV; j++) {
        const int vi = j * GN_THREADS + tid;
        if (vi < s.nvec) {
            Storage<DT>::load(x + s.v0 + (size_t)vi * V, xv[j]);
            load_f32<V>(dy + s.v0 + (size_t)vi * V, gv[j]);
            if constexpr (RES) load_f32<V>(out + s.v0 + (size_t)vi * V, ov[j]);
        }
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NV; j++)
        if (j * GN_THREADS + tid < s.nvec) {
#pragma unroll
            for (int k = 0; k < V; k++) {
                if constexpr (RES) gv[j][k] = mask_f(ov[RES ? j : 0][k], gv[j][k]);
                if constexpr (EP != EP_NONE) gv[j][k] = mask_f(GN_Y(xv[j][k], mu, rs, gm, bt), gv[j][k]);
                if constexpr (EP == EP_NONE) {
                    s1 += gv[j][k];
                    s2 += gv[j][k] * (xv[j][k] - mu);
                } else {
                    gn_acc_fused(s1, s2, gv[j][k], xv[j][k] - mu);
                }
            }
        }
    size_t ei;
    if (edge_index(s, tid, ei)) {
        float g = dy[ei];
        if constexpr (RES) g = mask_f(out[ei], g);
        if constexpr (EP != EP_NONE) g = mask_f(GN_Y(Storage<DT>::load1(x + ei), mu, rs, gm, bt), g);
        if constexpr (EP == EP_NONE) {
            s1 += g;
            s2 += g * (Storage<DT>::load1(x + ei) - mu);
        } else {
            gn_acc_fused(s1, s2, g, Storage<DT>::load1(x + ei) - mu);
        }
    }
    const float2 t = block_sum2(s1, s2, red);
    if (tid == 0) partial[blockIdx.x] = t;
}

// gchunks = chunks (one workgroup per chunk, dx and / or dres written) or 1 (neither wanted: one workgroup per plane, which only stores the plane's
// sums).  dres (EP_RELU_ADD_RELU only; NULL = not wanted) receives the outer-masked gradient.
template <int DT, int EP>
__global__ __launch_bounds__(GN_THREADS) void k_gn_bwd_apply(const typename Storage<DT>::T *__restrict__ x, const float *__restrict__ dy,
                                                             const float *__restrict__ gamma, const float *__restrict__ mean,
                                                             const float *__restrict__ rstd, const float2 *__restrict__ partial, int HW, int chunks,
                                                             int gchunks, int C, int cpg, int G, typename Storage<DT>::T *__restrict__ dx,
                                                             float2 *__restrict__ sums, const float *__restrict__ beta,
                                                             const float *__restrict__ out, float *__restrict__ dres) {
    constexpr int V = Storage<DT>::V, NV = GN_PT / V;
    constexpr bool RES = EP == EP_RELU_ADD_RELU;
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
    if (dx == nullptr && (!RES || dres == nullptr)) return;
    const unsigned n = plane / (unsigned)C, c = plane - n * (unsigned)C, g = c / (unsigned)cpg;
    const size_t p0 = (size_t)plane * HW, b = p0 + (size_t)ck * GN_CHUNK, e = min(b + (size_t)GN_CHUNK, p0 + (size_t)HW);
    const Span s = make_span<V>(b, e);
    float xv[NV][V], gv[NV][V], ex = 0.f, eg = 0.f;
    float ov[RES ? NV : 1][V], eo = 0.f;
#pragma unroll
    for (int j = 0; j < NV; j++) {
        const int vi = j * GN_THREADS + tid;
        if (vi < s.nvec) {
            Storage<DT>::load(x + s.v0 + (size_t)vi * V, xv[j]);
            load_f32<V>(dy + s.v0 + (size_t)vi * V, gv[j]);
            if constexpr (RES) load_f32<V>(out + s.v0 + (size_t)vi * V, ov[j]);
        }
    }
    size_t ei;
    const bool edge = edge_index(s, tid, ei);
    if (edge) {
        ex = Storage<DT>::load1(x + ei);
        eg = dy[ei];
        if constexpr (RES) eo = out[ei];
    }
    if constexpr (RES) {  // the outer mask; what is left is the residual's gradient
#pragma unroll
        for (int j = 0; j < NV; j++)
            if (j * GN_THREADS + tid < s.nvec) {
#pragma unroll
                for (int k = 0; k < V; k++) gv[j][k] = mask_f(ov[j][k], gv[j][k]);
                if (dres != nullptr) store_f32<V>(dres + s.v0 + (size_t)(j * GN_THREADS + tid) * V, gv[j]);
            }
        if (edge) {
            eg = mask_f(eo, eg);
            if (dres != nullptr) dres[ei] = eg;
        }
        if (dx == nullptr) return;
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
    float gm = 0.f, bt = 0.f;
    if constexpr (EP != EP_NONE) {
        gm = gamma[c];
        bt = beta[c];
    }
#pragma unroll
    for (int j = 0; j < NV; j++) {
        const int vi = j * GN_THREADS + tid;
        if (vi < s.nvec) {
            float o[V];
#pragma unroll
            for (int k = 0; k < V; k++) {
                if constexpr (EP != EP_NONE) gv[j][k] = mask_f(GN_Y(xv[j][k], mu, rs, gm, bt), gv[j][k]);
                o[k] = GN_DX(kd, gv[j][k], c1, xv[j][k] - mu, c2);
            }
            Storage<DT>::store(dx + s.v0 + (size_t)vi * V, o);
        }
    }
    if (edge) {
        if constexpr (EP != EP_NONE) eg = mask_f(GN_Y(ex, mu, rs, gm, bt), eg);
        Storage<DT>::store1(dx + ei, GN_DX(kd, eg, c1, ex - mu, c2));
    }
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

// common argument checks: 0 = go on, 1 = nothing to do, < 0 = refused
int gn_check(int dtype, int N, int C, int G, int HW) {
    if (N < 0 || C < 0 || HW < 0 || G <= 0 || !dtype_ok(dtype) || C % G != 0) return GPSGS_E_INVALID;
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

namespace {

template <int DT, int EP>
void launch_forward(const void *x, const float *gamma, const float *beta, const float *res, int N, int C, int G, int HW, float eps, float *out,
                    float *mean, float *rstd, void *scratch, hipStream_t s) {
    typedef const typename Storage<DT>::T *XP;
    const int cpg = C / G, L = cpg * HW, chunks = (int)cdiv(L, GN_CHUNK);
    const dim3 grid((unsigned)((size_t)N * G * chunks)), block(GN_THREADS);
    float2 *partial = (float2 *)scratch + (size_t)N * C;
    hipLaunchKernelGGL((k_gn_moments<DT>), grid, block, 0, s, (XP)x, L, chunks, partial);
    hipLaunchKernelGGL((k_gn_apply<DT, EP>), grid, block, 0, s, (XP)x, gamma, beta, (const float2 *)partial, L, chunks, HW, cpg, G, eps, out, mean, rstd,
                       res);
}

template <int DT, int EP>
void launch_backward(const void *x, const float *dout, const float *out, const float *gamma, const float *beta, const float *mean, const float *rstd,
                     int N, int C, int G, int HW, void *dx, float *dres, float *dgamma, float *dbeta, void *scratch, hipStream_t s) {
    typedef typename Storage<DT>::T X;
    const int cpg = C / G, chunks = (int)cdiv(HW, GN_CHUNK), gchunks = dx || dres ? chunks : 1;
    const dim3 block(GN_THREADS);
    float2 *sums = (float2 *)scratch, *partial = sums + (size_t)N * C;
    const unsigned planes = (unsigned)N * (unsigned)C;
    hipLaunchKernelGGL((k_gn_bwd_sums<DT, EP>), dim3(planes * chunks), block, 0, s, (const X *)x, dout, mean, HW, chunks, C, cpg, G, partial, gamma, beta,
                       rstd, out);
    hipLaunchKernelGGL((k_gn_bwd_apply<DT, EP>), dim3(planes * gchunks), block, 0, s, (const X *)x, dout, gamma, mean, rstd, (const float2 *)partial, HW,
                       chunks, gchunks, C, cpg, G, (X *)dx, sums, beta, out, dres);
    if (dgamma)
        hipLaunchKernelGGL(k_gn_param_grad, dim3((unsigned)cdiv(C, GN_THREADS)), block, 0, s, (const float2 *)sums, rstd, N, C, cpg, G, dgamma, dbeta);
}

// f(dt, ep) with the run-time dtype and epilogue as compile-time constants: the six <DT, EP> instantiations of whatever f launches
template <class F> void dispatch(int dtype, int ep, F f) {
    with_dtype(dtype, [&](auto dt) {
        if (ep == EP_NONE)
            f(dt, std::integral_constant<int, EP_NONE>());
        else if (ep == EP_RELU)
            f(dt, std::integral_constant<int, EP_RELU>());
        else
            f(dt, std::integral_constant<int, EP_RELU_ADD_RELU>());
    });
}

// gn_forward (EP_NONE, no residual) and gne_forward (EP_RELU, or EP_RELU_ADD_RELU with a residual)
int forward(int ep, const void *x, int dtype, const float *gamma, const float *beta, const float *residual, int N, int C, int G, int HW, float eps,
            float *out, float *mean, float *rstd, void *scratch, void *stream) {
    const int rc = gn_check(dtype, N, C, G, HW);
    if (rc != 0) return rc < 0 ? rc : GPSGS_OK;
    if (!x || !gamma || !beta || !out || !mean || !rstd || !scratch) return GPSGS_E_INVALID;
    if (!aligned(x, 16) || !aligned(out, 16) || !aligned(residual, 16) || !aligned(scratch, 8)) return GPSGS_E_INVALID;
    dispatch(dtype, ep, [&](auto dt, auto e) {
        launch_forward<decltype(dt)::DT, decltype(e)::value>(x, gamma, beta, residual, N, C, G, HW, eps, out, mean, rstd, scratch, (hipStream_t)stream);
    });
    return launched();
}

// gn_backward (EP_NONE: no beta, out or dres) and gne_backward (EP_RELU, or EP_RELU_ADD_RELU with the forward's out).  An invalid argument is
// reported even where there is nothing to do.
int backward(int ep, const void *x, int dtype, const float *dout, const float *out, const float *gamma, const float *beta, const float *mean,
             const float *rstd, int N, int C, int G, int HW, void *dx, float *dres, float *dgamma, float *dbeta, void *scratch, void *stream) {
    const int rc = gn_check(dtype, N, C, G, HW);
    if (rc < 0) return rc;
    if ((dgamma != nullptr) != (dbeta != nullptr)) return GPSGS_E_INVALID;
    if (dres && !out) return GPSGS_E_INVALID;  // only the residual form has a residual to differentiate
    if (rc != 0) return GPSGS_OK;
    if (!x || !dout || !gamma || (ep != EP_NONE && !beta) || !mean || !rstd || !scratch) return GPSGS_E_INVALID;
    if (!aligned(x, 16) || !aligned(dout, 16) || !aligned(out, 16) || !aligned(dx, 16) || !aligned(dres, 16) || !aligned(scratch, 8))
        return GPSGS_E_INVALID;
    if (!dx && !dres && !dgamma) return GPSGS_OK;
    dispatch(dtype, ep, [&](auto dt, auto e) {
        launch_backward<decltype(dt)::DT, decltype(e)::value>(x, dout, out, gamma, beta, mean, rstd, N, C, G, HW, dx, dres, dgamma, dbeta, scratch,
                                                                 (hipStream_t)stream);
    });
    return launched();
}

}  // namespace

extern "C" int gn_forward(const void *x, int dtype, const float *gamma, const float *beta, int N, int C, int G, int HW, float eps, float *y,
                          float *mean, float *rstd, void *scratch, void *stream) {
    return forward(EP_NONE, x, dtype, gamma, beta, nullptr, N, C, G, HW, eps, y, mean, rstd, scratch, stream);
}

extern "C" int gn_backward(const void *x, int dtype, const float *dy, const float *gamma, const float *mean, const float *rstd, int N, int C, int G,
                           int HW, void *dx, float *dgamma, float *dbeta, void *scratch, void *stream) {
    return backward(EP_NONE, x, dtype, dy, nullptr, gamma, nullptr, mean, rstd, N, C, G, HW, dx, nullptr, dgamma, dbeta, scratch, stream);
}

// ---- the same with the epilogue fused (see the top of the file): residual == NULL / out == NULL select EP_RELU, otherwise EP_RELU_ADD_RELU ----
extern "C" int gne_forward(const void *x, int dtype, const float *gamma, const float *beta, const float *residual, int N, int C, int G, int HW,
                           float eps, float *out, float *mean, float *rstd, void *scratch, void *stream) {
    return forward(residual ? EP_RELU_ADD_RELU : EP_RELU, x, dtype, gamma, beta, residual, N, C, G, HW, eps, out, mean, rstd, scratch, stream);
}

extern "C" int gne_backward(const void *x, int dtype, const float *dout, const float *out, const float *gamma, const float *beta, const float *mean,
                            const float *rstd, int N, int C, int G, int HW, void *dx, float *dres, float *dgamma, float *dbeta, void *scratch,
                            void *stream) {
    return backward(out ? EP_RELU_ADD_RELU : EP_RELU, x, dtype, dout, out, gamma, beta, mean, rstd, N, C, G, HW, dx, dres, dgamma, dbeta, scratch,
                    stream);
}
