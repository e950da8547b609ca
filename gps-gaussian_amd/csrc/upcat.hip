// upcat.hip -- the regresser's decoder glue, bilinear 2x upsample + channel concatenation, as one streaming op, forward and backward, for gfx950
// (DESIGN.md "Decoder glue").
//
//     out[n, c, :, :]        = upsample2x(a[n, c])     c in [0, Ca)        a [N,Ca,h,w] fp32 NCHW, out [N, Ca + sum C_k, 2h, 2w]
//     out[n, c0_k + c, :, :] = s_k[n, c]               c in [0, C_k)       s_k [N,C_k,2h,2w], K <= 3 of them, c0_k = Ca + C_0 + .. + C_{k-1}
//
// The reference runs nn.Upsample(scale_factor=2, mode="bilinear") and torch.cat three times in GSRegresser.forward (lib/gs_parm_network.py:56-67).
// With align_corners=False and a scale of exactly 2 the interpolation is separable with fixed taps per axis (n = the axis' input length):
//     o[2i]     = 0.25 a[max(i - 1, 0)] + 0.75 a[i]
//     o[2i + 1] = 0.75 a[i] + 0.25 a[min(i + 1, n - 1)]
// so a clamped index IS the border rule: o[0] = a[0], o[2n - 1] = a[n - 1], an axis of length 1 is duplicated.
//
// THE EVALUATION ORDER (exact fp32 in this order; every multiplication by 0.25 is exact):
//   forward    along x first, then along y, each as   near_far(p, q) = fmaf(0.75, p, 0.25 * q)   with p the 0.75 tap: one rounding per axis, two on
//              the path of every tap.
//   backward   da[i,j] is the gather of the (at most) 4 x 4 taps of dout[:, :Ca] that the forward scattered from a[i,j]: rows 2i-1 .. 2i+2, columns
//              2j-1 .. 2j+2, both clamped to the plane, weights 0.25, 0.75, 0.75, 0.25 per axis -- the clamp lands the outer tap of a border element
//              on its own first / last row a second time, which is the tap the forward's clamp folded onto it.  Along x first, then along y, each as
//              gather(d0, d1, d2, d3) = fmaf(0.75, d1 + d2, 0.25 * (d0 + d3)):  two roundings per axis, four on the path of every tap.
//
//   k_uc_fwd   one launch.  The first N * Ca * tiles workgroups each produce a UC_TH x UC_TW tile of one upsampled plane: the (UC_TH/2 + 2) x
//              (UC_TW/2 + 2) input elements under it go to LDS once (loads from clamped addresses: the value at the clamped address is the one the
//              border rule asks for, so there is nothing to select), then a lane makes 4 consecutive x of 4 consecutive rows from 4 x 4 of them --
//              the two output rows that share an input-row pair come from the same reads.  The workgroups behind them copy the skips, UC_COPY
//              elements of one sample of one skip each (its channels are one contiguous run on both sides), every load issued before the first store.
//              VEC (w even, every pointer 16-byte aligned): 16-byte stores and copies; planes are 16-byte aligned relative to the base because
//              (2h)(2w) = 4hw.  Otherwise 4-byte accesses, a wave on one contiguous 256-byte run per instruction.
//   k_uc_bwd   one thread per element of a, 64 x 4 of them per workgroup; the two middle columns of a row as one 8-byte load where dout is 8-byte
//              aligned (2j is even, rows and planes are even).  Every element of da is written exactly once: no atomics, no memset, the same bits
//              on every run.  The skips' gradients are slices of dout and need no kernel.
// Element offsets are 64-bit; a coordinate inside a plane is an int.
#include "op_common.h"

namespace {

constexpr int UC_THREADS = 256;
constexpr int UC_TH = 16, UC_TW = 256;                      // output tile of a workgroup of the upsampled part
constexpr int UC_IH = UC_TH / 2 + 2, UC_IW = UC_TW / 2 + 2;  // the input elements under it, with the one-element rim
constexpr int UC_COPY = 4096;                                // elements of a skip one workgroup copies
constexpr int UC_BW = 64, UC_BH = 4;                         // elements of a (columns, rows) per workgroup of the backward
constexpr int UC_MAX_SKIPS = 3;

struct Skips {
    const float *p[UC_MAX_SKIPS];
    int C[UC_MAX_SKIPS], c0[UC_MAX_SKIPS];   // channels, first output channel
    unsigned first[UC_MAX_SKIPS];            // first copy workgroup of skip k (counted from the first copy workgroup of the launch)
    unsigned chunks[UC_MAX_SKIPS];           // copy workgroups per sample of skip k
};

__device__ __forceinline__ float near_far(float p, float q) { return __fmaf_rn(0.75f, p, 0.25f * q); }
__device__ __forceinline__ float gather(float d0, float d1, float d2, float d3) { return __fmaf_rn(0.75f, d1 + d2, 0.25f * (d0 + d3)); }
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// 4 consecutive outputs of an axis from the inputs v[0..3] = a[J-1], a[J], a[J+1], a[J+2] (clamped): o[2J], o[2J+1], o[2J+2], o[2J+3]
__device__ __forceinline__ void up4(const float (&v)[4], float (&o)[4]) {
    o[0] = near_far(v[1], v[0]);
    o[1] = near_far(v[1], v[2]);
    o[2] = near_far(v[2], v[1]);
    o[3] = near_far(v[2], v[3]);
}

template <bool VEC>
__global__ __launch_bounds__(UC_THREADS) void k_uc_fwd(const float *__restrict__ a, const Skips sk, float *__restrict__ out, int Ca, int Ctot, int h,
                                                       int w, int tx, int ty, unsigned up_blocks, int K) {
    __shared__ float t[UC_IH][UC_IW];
    const unsigned b = blockIdx.x;
    const int tid = threadIdx.x;
    const int H2 = 2 * h, W2 = 2 * w;
    const size_t plane = (size_t)H2 * W2;
    if (b < up_blocks) {
        unsigned r = b;
        const int bx = (int)(r % (unsigned)tx);
        r /= (unsigned)tx;
        const int by = (int)(r % (unsigned)ty);
        r /= (unsigned)ty;   // n * Ca + c: the plane of a
        const size_t n = r / (unsigned)Ca, c = r % (unsigned)Ca;
        const float *ap = a + (size_t)r * ((size_t)h * w);
        float *op = out + (n * Ctot + c) * plane;
        const int i0 = by * (UC_TH / 2) - 1, j0 = bx * (UC_TW / 2) - 1;   // the rim's corner
        for (int e = tid; e < UC_IH * UC_IW; e += UC_THREADS) {
            const int li = e / UC_IW, lj = e % UC_IW;
            t[li][lj] = ap[(size_t)clampi(i0 + li, h - 1) * w + clampi(j0 + lj, w - 1)];
        }
        __syncthreads();
        const int cx = tid & 63, rg = tid >> 6;
        float hx[4][4];   // rows I-1 .. I+2 of a, interpolated along x
#pragma unroll
        for (int q = 0; q < 4; q++) {
            float v[4];
#pragma unroll
            for (int s = 0; s < 4; s++) v[s] = t[2 * rg + q][2 * cx + s];
            up4(v, hx[q]);
        }
        const int X = bx * UC_TW + 4 * cx, Y = by * UC_TH + 4 * rg;
        float o[4][4];   // [x][row]
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const float v[4] = {hx[0][s], hx[1][s], hx[2][s], hx[3][s]};
            up4(v, o[s]);
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (Y + q >= H2) break;
            float *row = op + (size_t)(Y + q) * W2;
            if constexpr (VEC) {
                if (X < W2) *reinterpret_cast<float4 *>(row + X) = make_float4(o[0][q], o[1][q], o[2][q], o[3][q]);
            } else {
#pragma unroll
                for (int s = 0; s < 4; s++)
                    if (X + s < W2) row[X + s] = o[s][q];
            }
        }
        return;
    }
    unsigned cb = b - up_blocks;
    int k = 0;
    if (K > 1 && cb >= sk.first[1]) k = 1;
    if (K > 2 && cb >= sk.first[2]) k = 2;
    cb -= sk.first[k];
    const size_t n = cb / sk.chunks[k], len = (size_t)sk.C[k] * plane;
    const size_t base = (size_t)(cb % sk.chunks[k]) * UC_COPY;
    const float *src = sk.p[k] + n * len;
    float *dst = out + (n * Ctot + sk.c0[k]) * plane;
    if constexpr (VEC) {
        constexpr int Q = UC_COPY / (4 * UC_THREADS);
        float4 v[Q];
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const size_t e = base + (size_t)(q * UC_THREADS + tid) * 4;   // len is a multiple of 4: the four are inside or outside together
            v[q] = *reinterpret_cast<const float4 *>(src + (e < len ? e : 0));
        }
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const size_t e = base + (size_t)(q * UC_THREADS + tid) * 4;
            if (e < len) *reinterpret_cast<float4 *>(dst + e) = v[q];
        }
    } else {
        constexpr int Q = UC_COPY / UC_THREADS;
        float v[Q];
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const size_t e = base + (size_t)(q * UC_THREADS + tid);
            v[q] = src[e < len ? e : 0];
        }
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const size_t e = base + (size_t)(q * UC_THREADS + tid);
            if (e < len) dst[e] = v[q];
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(UC_THREADS) void k_uc_bwd(const float *__restrict__ dout, float *__restrict__ da, int Ca, int Ctot, int h, int w, int tx,
                                                       int ty) {
    unsigned r = blockIdx.x;
    const int bx = (int)(r % (unsigned)tx);
    r /= (unsigned)tx;
    const int by = (int)(r % (unsigned)ty);
    r /= (unsigned)ty;   // n * Ca + c
    const size_t n = r / (unsigned)Ca, c = r % (unsigned)Ca;
    const int j = bx * UC_BW + ((int)threadIdx.x & 63), i = by * UC_BH + ((int)threadIdx.x >> 6);
    const int jj = j < w ? j : w - 1, ii = i < h ? i : h - 1;   // a thread outside a reads what the last one inside reads, and stores nothing
    const int H2 = 2 * h, W2 = 2 * w;
    const float *dp = dout + (n * Ctot + c) * ((size_t)H2 * W2);
    const int x0 = clampi(2 * jj - 1, W2 - 1), x3 = clampi(2 * jj + 2, W2 - 1);
    float hs[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const float *row = dp + (size_t)clampi(2 * ii - 1 + q, H2 - 1) * W2;
        float d1, d2;
        if constexpr (VEC) {
            const float2 m = *reinterpret_cast<const float2 *>(row + 2 * jj);
            d1 = m.x;
            d2 = m.y;
        } else {
            d1 = row[2 * jj];
            d2 = row[2 * jj + 1];
        }
        hs[q] = gather(row[x0], d1, d2, row[x3]);
    }
    if (j < w && i < h) da[(size_t)r * ((size_t)h * w) + (size_t)i * w + j] = gather(hs[0], hs[1], hs[2], hs[3]);
}

struct Dims {
    int Ctot, tx, ty;
    long long up_blocks, copy_blocks;
    Skips sk;
};

bool skips_ok(int K, const int *C) {
    if (K < 0 || K > UC_MAX_SKIPS || (K > 0 && !C)) return false;
    for (int k = 0; k < K; k++)
        if (C[k] < 1) return false;
    return true;
}

// fills d (but for the skip pointers); false = refused: a non-positive size, K outside 0..3, a skip channel count below 1, or 2^31 elements or more
// in a, in out or (therefore) in a skip.  No intermediate product overflows: every factor is checked against the limit before the next one.
bool make_dims(int K, const int *C, int N, int Ca, int h, int w, Dims &d) {
    const long long LIM = 0x7fffffffLL;
    if (!skips_ok(K, C) || N <= 0 || Ca <= 0 || h <= 0 || w <= 0) return false;
    long long Ctot = Ca;
    for (int k = 0; k < K; k++) Ctot += C[k];   // < 2^33
    const long long hw = (long long)h * w;        // < 2^62
    if (hw > LIM / 4 || Ctot > LIM) return false;
    const long long plane = 4 * hw;
    if ((long long)N * Ctot > LIM || (long long)N * Ctot * plane > LIM) return false;   // out; a and the skips are smaller
    d.Ctot = (int)Ctot;
    d.tx = (int)cdiv((size_t)(2 * w), UC_TW);
    d.ty = (int)cdiv((size_t)(2 * h), UC_TH);
    d.up_blocks = (long long)N * Ca * d.tx * d.ty;   // each covers an element of out of its own: < 2^31
    d.copy_blocks = 0;
    int c0 = Ca;
    for (int k = 0; k < UC_MAX_SKIPS; k++) {
        d.sk.p[k] = nullptr;
        d.sk.C[k] = k < K ? C[k] : 0;
        d.sk.c0[k] = c0;
        d.sk.first[k] = (unsigned)d.copy_blocks;
        d.sk.chunks[k] = k < K ? (unsigned)cdiv((size_t)C[k] * (size_t)plane, UC_COPY) : 1;
        if (k < K) {
            d.copy_blocks += (long long)N * d.sk.chunks[k];
            c0 += C[k];
        }
    }
    return d.up_blocks + d.copy_blocks <= LIM;
}

}  // namespace

extern "C" int uc_supported(int K, const int *skip_channels) { return skips_ok(K, skip_channels) ? 1 : 0; }

extern "C" int uc_tile(int *tile_h, int *tile_w) {
    if (!tile_h || !tile_w) return GPSGS_E_INVALID;
    *tile_h = UC_TH;
    *tile_w = UC_TW;
    return GPSGS_OK;
}

extern "C" int uc_forward(const float *a, const float *const *skips, const int *skip_channels, int K, int N, int Ca, int h, int w, float *out,
                          void *stream) {
    Dims d;
    if (!make_dims(K, skip_channels, N, Ca, h, w, d)) return GPSGS_E_INVALID;
    if (!a || !out || (K > 0 && !skips) || !aligned(a, 4) || !aligned(out, 4)) return GPSGS_E_INVALID;
    bool vec = w % 2 == 0 && aligned(out, 16);
    for (int k = 0; k < K; k++) {
        if (!skips[k] || !aligned(skips[k], 4)) return GPSGS_E_INVALID;
        d.sk.p[k] = skips[k];
        vec = vec && aligned(skips[k], 16);
    }
    const dim3 grid((unsigned)(d.up_blocks + d.copy_blocks)), block(UC_THREADS);
    if (vec)
        hipLaunchKernelGGL((k_uc_fwd<true>), grid, block, 0, (hipStream_t)stream, a, d.sk, out, Ca, d.Ctot, h, w, d.tx, d.ty, (unsigned)d.up_blocks, K);
    else
        hipLaunchKernelGGL((k_uc_fwd<false>), grid, block, 0, (hipStream_t)stream, a, d.sk, out, Ca, d.Ctot, h, w, d.tx, d.ty, (unsigned)d.up_blocks, K);
    return launched();
}

extern "C" int uc_backward(const float *dout, const int *skip_channels, int K, int N, int Ca, int h, int w, float *da, void *stream) {
    Dims d;
    if (!make_dims(K, skip_channels, N, Ca, h, w, d)) return GPSGS_E_INVALID;
    if (!dout || !aligned(dout, 4) || !aligned(da, 4)) return GPSGS_E_INVALID;
    if (!da) return GPSGS_OK;
    const int tx = (int)cdiv((size_t)w, UC_BW), ty = (int)cdiv((size_t)h, UC_BH);
    const dim3 grid((unsigned)((long long)N * Ca * tx * ty)), block(UC_THREADS);   // each covers an element of a of its own: < 2^31
    if (aligned(dout, 8))
        hipLaunchKernelGGL((k_uc_bwd<true>), grid, block, 0, (hipStream_t)stream, dout, da, Ca, d.Ctot, h, w, tx, ty);
    else
        hipLaunchKernelGGL((k_uc_bwd<false>), grid, block, 0, (hipStream_t)stream, dout, da, Ca, d.Ctot, h, w, tx, ty);
    return launched();
}
