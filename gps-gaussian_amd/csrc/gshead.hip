// gshead.hip -- the tail of a Gaussian-parameter head, ReLU -> 1x1 convolution -> activation, as one streaming op, forward and backward, for gfx950
// (DESIGN.md "Gaussian heads").
//
//     y[n,k,p] = act( b[k] + sum_c w[k,c] * max(h[n,c,p], 0) )        h [N,C,H,W] fp32 NCHW, w [K,C], p over the H*W pixels of a plane
//
// The reference's three heads end in Conv2d(32, 4 | 3 | 1, 1) on a full-resolution [N,32,H,W] tensor (lib/gs_parm_network.py:34-50): per pixel 32
// loads against at most 128 multiply-adds, so the op is a stream over h.  The kernels work in NCHW as it lies: a lane owns 4 pixels of one sample
// (2 at C = 64) and holds all C channels of them in registers (every load issued before the first multiply-add), the weights and the bias are
// wave-uniform (scalar loads), z = bias, then fmaf over c in index order.  Templated on <C, K, VEC>; instantiated for C in {16, 32, 64} x K in 1..4.
//
//   VEC    H*W % 4 == 0 and every tensor 16-byte aligned: the lane's pixels are consecutive, one 16-byte (C = 64: 8-byte) access per channel.
//          Otherwise plane bases are off 16-byte boundaries for n, c > 0 and the lane takes the pixels tid, tid + 256, ... of the pass with 4-byte
//          accesses (still one contiguous 256-byte row per wave instruction).
//   k_gh_fwd   one 256-thread workgroup per tile of GH_TILE = 1024 pixels of one sample, in one pass (C = 64: two passes over halves of the tile, so
//              that the channels of a lane's pixels stay in registers); reads h once, writes the K planes of y once.
//   k_gh_bwd   the same tile: h and dy are read once, z is RECOMPUTED from h with the forward's arithmetic (no saved y is read), dz = dy * act'(z);
//              then dh[c] = (h[c] > 0) * sum_k w[k,c] dz[k] (when wanted) and the tile's K*C + K sums of dz[k] * max(h[c], 0) and of dz[k] (when
//              wanted): a lane's pixels in index order, the wave by wave_sums(), the 4 waves in index order through LDS -> scratch[tile][K*C + K].
//              One pass over h serves both: the weight sums need no accumulator that outlives a pass (DESIGN.md has the register figures).
//   k_sum_partials   (op_reduce.h) adds the tiles' partials in index order, in groups of GH_GROUP and then the groups.
// No atomics; every sum has a fixed order: the same bits on every run.  Element offsets into h, y, dy, dh are 64-bit; a pixel index inside a plane
// is an int (H*W is refused above INT_MAX - GH_TILE).  Guarded loads are unconditional loads from a clamped address followed by a select, as in
// stem_conv.hip.
#include <type_traits>

#include "op_reduce.h"

namespace {

constexpr int GH_THREADS = 256, GH_TILE = 1024;
constexpr int GH_GROUP = 64;  // tiles per first-stage group of the reduction
enum { GH_ACT_NONE = 0, GH_ACT_SOFTPLUS = 1, GH_ACT_SIGMOID = 2 };

// pixels per lane and pass: 4 (16-byte accesses) while the C channels of them fit the register file twice over; 2 at C = 64, where the workgroup
// makes two passes over halves of its tile
template <int C> struct Shape {
    static constexpr int PX = C <= 32 ? 4 : 2, PASS = GH_THREADS * PX, PASSES = GH_TILE / PASS;
};

struct Act {
    int kind;
    float beta, threshold;
};

// torch's definitions: softplus(z) = z where beta z > threshold, else log1p(exp(beta z)) / beta; sigmoid(z) = 1 / (1 + exp(-z))
__device__ __forceinline__ float sigmoidf(float z) { return 1.f / (1.f + expf(-z)); }
__device__ __forceinline__ float act_value(float z, const Act a) {
    if (a.kind == GH_ACT_SOFTPLUS) {
        const float bz = a.beta * z;
        return bz > a.threshold ? z : log1pf(expf(bz)) / a.beta;
    }
    return a.kind == GH_ACT_SIGMOID ? sigmoidf(z) : z;
}
__device__ __forceinline__ float act_slope(float z, const Act a) {
    if (a.kind == GH_ACT_SOFTPLUS) {
        const float bz = a.beta * z;
        return bz > a.threshold ? 1.f : sigmoidf(bz);
    }
    if (a.kind == GH_ACT_SIGMOID) {
        const float s = sigmoidf(z);
        return s * (1.f - s);
    }
    return 1.f;
}

__device__ __forceinline__ float relu(float v) { return v < 0.f ? 0.f : v; }  // NaN stays NaN, as ATen's

// the PX pixels of a lane in the pass that starts at pixel t0 of a plane of HW pixels: index p[j], inside the plane ok[j]; q[j] = p[j] where ok, else
// 0 (a valid address).  VEC: consecutive pixels (HW % 4 == 0: inside or outside together), one 16- or 8-byte access; else 4-byte accesses, the lanes
// of a wave on consecutive pixels.
template <bool VEC, int PX> struct Pixels {
    int p[PX], q[PX];
    bool ok[PX];
    __device__ __forceinline__ Pixels(int t0, int HW) {
#pragma unroll
        for (int j = 0; j < PX; j++) {
            p[j] = VEC ? t0 + (int)threadIdx.x * PX + j : t0 + j * GH_THREADS + (int)threadIdx.x;
            ok[j] = (VEC ? p[j] - j : p[j]) < HW;
            q[j] = ok[j] ? p[j] : 0;   // (VEC reads q[0] alone)
        }
    }
    // raw loads (from the clamped address), all in flight; mask with ok[] after
    __device__ __forceinline__ void load(const float *__restrict__ plane, float (&v)[PX]) const {
        if constexpr (VEC && PX == 4) {
            const float4 f = *reinterpret_cast<const float4 *>(plane + q[0]);
            v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
        } else if constexpr (VEC) {
            const float2 f = *reinterpret_cast<const float2 *>(plane + q[0]);
            v[0] = f.x; v[1] = f.y;
        } else {
#pragma unroll
            for (int j = 0; j < PX; j++) v[j] = plane[q[j]];
        }
    }
    __device__ __forceinline__ void store(float *__restrict__ plane, const float (&v)[PX]) const {
        if constexpr (VEC && PX == 4) {
            if (ok[0]) *reinterpret_cast<float4 *>(plane + p[0]) = make_float4(v[0], v[1], v[2], v[3]);
        } else if constexpr (VEC) {
            if (ok[0]) *reinterpret_cast<float2 *>(plane + p[0]) = make_float2(v[0], v[1]);
        } else {
#pragma unroll
            for (int j = 0; j < PX; j++)
                if (ok[j]) plane[p[j]] = v[j];
        }
    }
};

// z[k][j] = bias[k] + sum_c w[k,c] r[c][j] for the rectified activations r: fmaf in index order from the bias
template <int C, int K, int PX>
__device__ __forceinline__ void pre_activation(const float (&r)[C][PX], const float *__restrict__ w, const float *__restrict__ bias, float (&z)[K][PX]) {
#pragma unroll
    for (int k = 0; k < K; k++) {
        const float bv = bias[k];
#pragma unroll
        for (int j = 0; j < PX; j++) z[k][j] = bv;
    }
#pragma unroll
    for (int c = 0; c < C; c++)
#pragma unroll
        for (int k = 0; k < K; k++) {
            const float wv = w[k * C + c];
#pragma unroll
            for (int j = 0; j < PX; j++) z[k][j] = __fmaf_rn(wv, r[c][j], z[k][j]);
        }
}

template <int C, int K, bool VEC>
__global__ __launch_bounds__(GH_THREADS) void k_gh_fwd(const float *__restrict__ h, const float *__restrict__ w, const float *__restrict__ bias,
                                                       float *__restrict__ y, int HW, int tiles, Act a) {
    typedef Shape<C> S;
    const unsigned b = blockIdx.x;
    const size_t n = b / (unsigned)tiles;
    const int t0 = (int)(b % (unsigned)tiles) * GH_TILE;
    const float *hn = h + n * C * (size_t)HW;
#pragma unroll 1
    for (int pass = 0; pass < S::PASSES; pass++) {
        const Pixels<VEC, S::PX> px(t0 + pass * S::PASS, HW);
        float v[C][S::PX];
#pragma unroll
        for (int c = 0; c < C; c++) px.load(hn + (size_t)c * HW, v[c]);
#pragma unroll
        for (int c = 0; c < C; c++)
#pragma unroll
            for (int j = 0; j < S::PX; j++) v[c][j] = relu(v[c][j]);
        float z[K][S::PX];
        pre_activation<C, K, S::PX>(v, w, bias, z);
#pragma unroll
        for (int k = 0; k < K; k++) {
#pragma unroll
            for (int j = 0; j < S::PX; j++) z[k][j] = act_value(z[k][j], a);
            px.store(y + (n * K + k) * (size_t)HW, z[k]);
        }
    }
}

// The sums over the 64 lanes of a wave of the N values s[0..N) of each lane, N a power of two <= 64: at every step a lane hands half of what it
// holds to the lane `MASK` away and adds what it receives to the half it keeps, until one value is left (then plain xor steps).  N - 1 + (6 - log2 N)
// shuffles instead of 6 N.  Returns, in lane L, the sum of value number L / (64 / N).  The order of every sum is fixed.
template <int N, int MASK> __device__ __forceinline__ float wave_sums(float *s, int lane) {
    if constexpr (MASK == 0) {
        return s[0];
    } else if constexpr (N > 1) {
        const bool up = (lane & MASK) != 0;
#pragma unroll
        for (int i = 0; i < N / 2; i++) {
            const float mine = up ? s[i + N / 2] : s[i], theirs = up ? s[i] : s[i + N / 2];
            s[i] = mine + __shfl_xor(theirs, MASK, 64);
        }
        return wave_sums<N / 2, MASK / 2>(s, lane);
    } else {
        s[0] += __shfl_xor(s[0], MASK, 64);
        return wave_sums<1, MASK / 2>(s, lane);
    }
}

// partial[tile][k * C + c] for the weight, then partial[tile][K * C + k] for the bias; dh == NULL / partial == NULL: not wanted (wave-uniform)
template <int C, int K, bool VEC>
__global__ __launch_bounds__(GH_THREADS) void k_gh_bwd(const float *__restrict__ h, const float *__restrict__ w, const float *__restrict__ bias,
                                                       const float *__restrict__ dy, float *__restrict__ dh, float *__restrict__ partial, int HW,
                                                       int tiles, Act a) {
    typedef Shape<C> S;
    constexpr int PX = S::PX, M = K * C + K, WAVES = GH_THREADS / 64;
    __shared__ float red[WAVES * M];  // the waves' sums of this tile
    const unsigned b = blockIdx.x;
    const size_t n = b / (unsigned)tiles;
    const int t0 = (int)(b % (unsigned)tiles) * GH_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *hn = h + n * C * (size_t)HW;
#pragma unroll 1
    for (int pass = 0; pass < S::PASSES; pass++) {
        const Pixels<VEC, PX> px(t0 + pass * S::PASS, HW);
        float v[C][PX], dz[K][PX];
#pragma unroll
        for (int c = 0; c < C; c++) px.load(hn + (size_t)c * HW, v[c]);
#pragma unroll
        for (int k = 0; k < K; k++) px.load(dy + (n * K + k) * (size_t)HW, dz[k]);
        // rectified once, and zero outside the plane: h > 0 is v > 0 from here on (one copy of the C channels in registers, not two)
#pragma unroll
        for (int c = 0; c < C; c++)
#pragma unroll
            for (int j = 0; j < PX; j++) v[c][j] = px.ok[j] ? relu(v[c][j]) : 0.f;
        if (a.kind != GH_ACT_NONE) {
            float z[K][PX];
            pre_activation<C, K, PX>(v, w, bias, z);
#pragma unroll
            for (int k = 0; k < K; k++)
#pragma unroll
                for (int j = 0; j < PX; j++) dz[k][j] *= act_slope(z[k][j], a);
        }
#pragma unroll
        for (int k = 0; k < K; k++)
#pragma unroll
            for (int j = 0; j < PX; j++) dz[k][j] = px.ok[j] ? dz[k][j] : 0.f;  // a pixel outside the plane contributes nothing, whatever was loaded for it

        if (dh != nullptr) {
            float *dhn = dh + n * C * (size_t)HW;
#pragma unroll
            for (int c = 0; c < C; c++) {
                float g[PX];
#pragma unroll
                for (int j = 0; j < PX; j++) g[j] = w[c] * dz[0][j];
#pragma unroll
                for (int k = 1; k < K; k++) {
                    const float wv = w[k * C + c];
#pragma unroll
                    for (int j = 0; j < PX; j++) g[j] = __fmaf_rn(wv, dz[k][j], g[j]);
                }
#pragma unroll
                for (int j = 0; j < PX; j++) g[j] = v[c][j] > 0.f ? g[j] : 0.f;  // zero at h == 0, as ATen's ReLU
                px.store(dhn + (size_t)c * HW, g);
            }
        }

        if (partial != nullptr) {
#pragma unroll
            for (int k = 0; k < K; k++) {
                float s[C];  // the lane's pixels, in index order; then the wave, a row of the weight at a time
#pragma unroll
                for (int c = 0; c < C; c++) {
                    s[c] = dz[k][0] * v[c][0];
#pragma unroll
                    for (int j = 1; j < PX; j++) s[c] = __fmaf_rn(dz[k][j], v[c][j], s[c]);
                }
                const float t = wave_sums<C, 32>(s, lane);
                float d = dz[k][0];
#pragma unroll
                for (int j = 1; j < PX; j++) d += dz[k][j];
                float one[1] = {d};
                const float tb = wave_sums<1, 32>(one, lane);
                // (a later pass adds to what the same thread stored in the pass before)
                if (lane % (64 / C) == 0) {
                    float *r = red + wave * M + k * C + lane / (64 / C);
                    *r = pass == 0 ? t : *r + t;
                }
                if (lane == 0) {
                    float *r = red + wave * M + K * C + k;
                    *r = pass == 0 ? tb : *r + tb;
                }
            }
        }
    }
    if (partial != nullptr) {
        __syncthreads();
        float *out = partial + (size_t)b * M;
        for (int i = threadIdx.x; i < M; i += GH_THREADS) {
            float s = red[i];
#pragma unroll
            for (int q = 1; q < WAVES; q++) s += red[q * M + i];
            out[i] = s;
        }
    }
}

bool supported(int C, int K, int act) { return (C == 16 || C == 32 || C == 64) && K >= 1 && K <= 4 && act >= GH_ACT_NONE && act <= GH_ACT_SIGMOID; }

struct Dims {
    int N, HW, tiles;   // tiles per plane
    long long parts;    // N * tiles: workgroups of one launch, partials of the weight gradient
};

// fills d; false = refused: an unsupported (C, K, act), a non-positive size, a plane whose pixel index (plus one tile) does not fit an int, or more
// workgroups than a grid's x holds.  Element offsets are 64-bit, so N * C * H * W itself has no limit below the address space.
bool make_dims(int N, int C, int K, int H, int W, int act, Dims &d) {
    if (!supported(C, K, act) || N <= 0 || H <= 0 || W <= 0) return false;
    const long long HW = (long long)H * W;
    if (HW > 0x7fffffffLL - GH_TILE) return false;
    d.N = N;
    d.HW = (int)HW;
    d.tiles = (int)cdiv((size_t)HW, GH_TILE);
    d.parts = (long long)N * d.tiles;
    return d.parts <= 0x7fffffffLL;
}

bool act_ok(int act, float beta) { return act != GH_ACT_SOFTPLUS || beta > 0.f; }  // (a NaN beta fails the comparison too)

template <int C, int K>
void launch_fwd(bool vec, const float *h, const float *w, const float *bias, float *y, const Dims &d, Act a, hipStream_t s) {
    const dim3 grid((unsigned)d.parts), block(GH_THREADS);
    if (vec)
        hipLaunchKernelGGL((k_gh_fwd<C, K, true>), grid, block, 0, s, h, w, bias, y, d.HW, d.tiles, a);
    else
        hipLaunchKernelGGL((k_gh_fwd<C, K, false>), grid, block, 0, s, h, w, bias, y, d.HW, d.tiles, a);
}

template <int C, int K>
void launch_bwd(bool vec, const float *h, const float *w, const float *bias, const float *dy, float *dh, float *dw, float *db, float *scratch,
                const Dims &d, Act a, hipStream_t s) {
    const dim3 grid((unsigned)d.parts), block(GH_THREADS);
    float *partial = dw ? scratch : nullptr;
    if (vec)
        hipLaunchKernelGGL((k_gh_bwd<C, K, true>), grid, block, 0, s, h, w, bias, dy, dh, partial, d.HW, d.tiles, a);
    else
        hipLaunchKernelGGL((k_gh_bwd<C, K, false>), grid, block, 0, s, h, w, bias, dy, dh, partial, d.HW, d.tiles, a);
    if (!dw) return;
    constexpr int MW = K * C, M = MW + K;
    sum_partials(scratch, (int)d.parts, GH_GROUP, M, MW, dw, db, s);
}

// f(<C>, <K>) for a supported (C, K): the run-time pair as compile-time constants
template <int C, class F> void with_k(int K, F f) {
    switch (K) {
    case 1: f(std::integral_constant<int, C>(), std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, C>(), std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, C>(), std::integral_constant<int, 3>()); break;
    default: f(std::integral_constant<int, C>(), std::integral_constant<int, 4>()); break;
    }
}
template <class F> void with_ck(int C, int K, F f) {
    if (C == 16)
        with_k<16>(K, f);
    else if (C == 32)
        with_k<32>(K, f);
    else
        with_k<64>(K, f);
}

}  // namespace

extern "C" int gsr_head_supported(int C_in, int C_out, int act) { return supported(C_in, C_out, act) ? 1 : 0; }

extern "C" int gsr_head_tile(void) { return GH_TILE; }

extern "C" size_t gsr_head_scratch_bytes(int N, int C_in, int C_out, int H, int W) {
    Dims d;
    if (!make_dims(N, C_in, C_out, H, W, GH_ACT_NONE, d)) return 0;
    const size_t M = (size_t)C_out * C_in + C_out;
    return partials_scratch_bytes((size_t)d.parts, GH_GROUP, M);
}

extern "C" int gsr_head_forward(const float *h, const float *w, const float *bias, int N, int C_in, int C_out, int H, int W, int act, float beta,
                                float threshold, float *y, void *stream) {
    Dims d;
    if (!make_dims(N, C_in, C_out, H, W, act, d) || !act_ok(act, beta)) return GPSGS_E_INVALID;
    if (!h || !w || !bias || !y) return GPSGS_E_INVALID;
    if (!aligned(h, 4) || !aligned(w, 4) || !aligned(bias, 4) || !aligned(y, 4)) return GPSGS_E_INVALID;
    const bool vec = d.HW % 4 == 0 && aligned(h, 16) && aligned(y, 16);
    const Act a = {act, beta, threshold};
    with_ck(C_in, C_out, [&](auto c, auto k) { launch_fwd<decltype(c)::value, decltype(k)::value>(vec, h, w, bias, y, d, a, (hipStream_t)stream); });
    return launched();
}

extern "C" int gsr_head_backward(const float *h, const float *w, const float *bias, const float *y, const float *dy, int N, int C_in, int C_out, int H,
                                 int W, int act, float beta, float threshold, float *dh, float *dw, float *dbias, void *scratch, void *stream) {
    Dims d;
    (void)y;  // act' comes from z recomputed from h (DESIGN.md "Gaussian heads"): the forward's output is not read and may be NULL
    if (!make_dims(N, C_in, C_out, H, W, act, d) || !act_ok(act, beta)) return GPSGS_E_INVALID;
    if ((dw != nullptr) != (dbias != nullptr)) return GPSGS_E_INVALID;
    if (!h || !w || !bias || !dy || (dw && !scratch)) return GPSGS_E_INVALID;
    if (!aligned(h, 4) || !aligned(w, 4) || !aligned(bias, 4) || !aligned(dy, 4) || !aligned(dh, 4) || !aligned(dw, 4) || !aligned(dbias, 4) ||
        !aligned(scratch, 4))
        return GPSGS_E_INVALID;
    if (!dh && !dw) return GPSGS_OK;
    const bool vec = d.HW % 4 == 0 && aligned(h, 16) && aligned(dy, 16) && aligned(dh, 16);
    const Act a = {act, beta, threshold};
    with_ck(C_in, C_out, [&](auto c, auto k) {
        launch_bwd<decltype(c)::value, decltype(k)::value>(vec, h, w, bias, dy, dh, dw, dbias, (float *)scratch, d, a, (hipStream_t)stream);
    });
    return launched();
}
