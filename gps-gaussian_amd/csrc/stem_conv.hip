// stem_conv.hip -- direct 2-D convolution for layers with almost no input channels, forward and backward, for gfx950 (DESIGN.md "Stem convolution").
//
// The reference's two full-resolution stems are Conv2d(3, 32, 5, stride 2, padding 2) and Conv2d(1, 32, 5, stride 2, padding 2): K = C_in * 25 is
// far too short for a GEMM pipeline (the library picks an implicit-GEMM tile whose K step is 4 and transposes to NHWC and back around it).  Here the
// layer is what it looks like: contiguous NCHW, the weights wave-uniform (scalar loads), the input patch of an output tile in LDS, fp32 FMAs.
// Templated on <CIN, K, S> (S = stride; padding is a runtime argument); instantiated for <1, 5, 2> and <3, 5, 2> -- another small-C_in layer is one
// more instantiation in sc_forward / sc_backward.
//
//   k_sc_fwd         one 256-thread workgroup per TH x TW = 8 x 64 output tile of one sample.  The (TH*S + K - S) x (TW*S + K - S) x CIN input patch
//                    is staged in LDS, taps outside the image as zeros.  A lane holds 4 pixels along x times 8 output channels (32 accumulators);
//                    waves 0-1 take the even blocks of 8 channels, waves 2-3 the odd ones.  acc = bias, then fmaf in (ci, ky, kx) order; one rounding
//                    at the store (fp32 or fp16), 16 / 8 bytes per lane where the row allows it.
//   k_sc_bwd_input   gather form over input pixels; a wave holds pixels of ONE (y, x) parity class, so the <= ceil(K/S)^2 taps a pixel needs
//                    ((y + pad - ky) % S == 0) and their weights are wave-uniform.  A lane owns 4 pixels of its class in one column (they share
//                    dy rows).  Sums over C_out in index order.
//   k_sc_bwd_weight  one workgroup per tile: the input patch and, per block of 8 output channels, the dy tile in LDS.  Lane = (tap (ci, ky, kx),
//                    pixel slice); it accumulates dy * x over its slice's pixels for the 8 channels, the slices are added in index order, and the
//                    tile's C_out * CIN * K^2 sums + C_out bias sums go to scratch.
//   k_sum_partials   (op_reduce.h) adds the tiles' partials in index order, in groups of SC_GROUP and then the groups.
// No atomics; every sum has a fixed order: the same bits on every run.  Element offsets into x, y, dy, dx are 64-bit.
// Guarded global loads are written as an unconditional load from a clamped (always valid) address followed by a select: a branch around each load
// makes the compiler wait for every one of them in turn (measured: the fp16 backward ran 3x slower that way).
#include "op_reduce.h"

namespace {

constexpr int SC_TH = 8, SC_TW = 64;  // output tile
constexpr int SC_THREADS = 256;
constexpr int SC_CB = 8;      // output channels per block
constexpr int SC_PX = 4;      // pixels per lane along x (forward)
constexpr int SC_GROUP = 64;  // tiles per first-stage group of the reduction

template <int CIN, int K, int S> struct Patch {
    static constexpr int PH = SC_TH * S + K - S, PW = SC_TW * S + K - S;
    static constexpr int PITCH = (PW + 3) / 4 * 4;  // rows start on 16 bytes
    static constexpr int ELEMS = CIN * PH * PITCH;
};

// the input patch of the tile at output (oy0, ox0): xs[ci][r][c] = x[n, ci, oy0*S - pad + r, ox0*S - pad + c], or 0 outside the image
template <int CIN, int K, int S>
__device__ __forceinline__ void stage_patch(float *xs, const float *__restrict__ x, size_t n, int H, int W, int oy0, int ox0, int pad) {
    typedef Patch<CIN, K, S> P;
    const int iy0 = oy0 * S - pad, ix0 = ox0 * S - pad;
    constexpr int IT = (P::ELEMS + SC_THREADS - 1) / SC_THREADS, BATCH = 10;  // loads in flight per thread before the first LDS store waits for one
#pragma unroll 1
    for (int i0 = 0; i0 < IT; i0 += BATCH) {
        float v[BATCH];
#pragma unroll
        for (int i = 0; i < BATCH; i++) {
            const int e = (int)threadIdx.x + (i0 + i) * SC_THREADS;
            const int ci = e / (P::PH * P::PITCH), rem = e - ci * (P::PH * P::PITCH), r = rem / P::PITCH, c = rem - r * P::PITCH;
            const int iy = iy0 + r, ix = ix0 + c;
            // an unconditional load from a clamped address, then a select: no branch around the load, so the batch is in flight together
            const bool in = e < P::ELEMS && c < P::PW && iy >= 0 && iy < H && ix >= 0 && ix < W;
            const float t = x[in ? ((n * CIN + ci) * (size_t)H + iy) * (size_t)W + ix : 0];
            v[i] = in ? t : 0.f;
        }
#pragma unroll
        for (int i = 0; i < BATCH; i++) {
            const int e = (int)threadIdx.x + (i0 + i) * SC_THREADS;
            if (e < P::ELEMS) xs[e] = v[i];
        }
    }
}

struct Dims {
    int N, C_out, H, W, Ho, Wo, pad, tiles_x, tiles_y;
};

// (launch bound 4 waves per SIMD, and the ci loop kept a loop: left alone the compiler hoists all CIN * K patch rows of a lane out of the channel-block
// loop, 250 registers and one wave per SIMD for CIN = 3)
template <int CIN, int K, int S, int DT>
__global__ __launch_bounds__(SC_THREADS, 4) void k_sc_fwd(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias,
                                                       typename Storage<DT>::T *__restrict__ y, Dims d) {
    typedef Patch<CIN, K, S> P;
    typedef typename Storage<DT>::T Y;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *xs = reinterpret_cast<float *>(smem);
    const unsigned b = blockIdx.x, tx = b % (unsigned)d.tiles_x, ty = (b / (unsigned)d.tiles_x) % (unsigned)d.tiles_y;
    const size_t n = b / ((unsigned)d.tiles_x * (unsigned)d.tiles_y);
    const int oy0 = (int)ty * SC_TH, ox0 = (int)tx * SC_TW;
    stage_patch<CIN, K, S>(xs, x, n, d.H, d.W, oy0, ox0, d.pad);
    __syncthreads();

    const int tid = threadIdx.x, lx = tid & 15, ly = (tid >> 4) & 7;
    const int half = __builtin_amdgcn_readfirstlane(tid >> 7);  // wave-uniform: the weight loads stay scalar
    const int oy = oy0 + ly, ox = ox0 + lx * SC_PX;
    const float *xl = xs + (ly * S) * P::PITCH + lx * SC_PX * S;
    constexpr int NX = (SC_PX - 1) * S + K;  // input columns a lane's pixels touch in one row
    for (int cb = half; cb < d.C_out / SC_CB; cb += 2) {
        const int co0 = cb * SC_CB;
        float acc[SC_CB][SC_PX];
#pragma unroll
        for (int c = 0; c < SC_CB; c++) {
            const float bv = bias[co0 + c];
#pragma unroll
            for (int j = 0; j < SC_PX; j++) acc[c][j] = bv;
        }
#pragma unroll 1
        for (int ci = 0; ci < CIN; ci++) {
#pragma unroll
            for (int ky = 0; ky < K; ky++) {
                const float *row = xl + (ci * P::PH + ky) * P::PITCH;
                float xr[NX];
#pragma unroll
                for (int q = 0; q < NX / 4; q++) {
                    const float4 f = reinterpret_cast<const float4 *>(row)[q];
                    xr[4 * q] = f.x; xr[4 * q + 1] = f.y; xr[4 * q + 2] = f.z; xr[4 * q + 3] = f.w;
                }
#pragma unroll
                for (int q = NX / 4 * 4; q < NX; q++) xr[q] = row[q];
#pragma unroll
                for (int c = 0; c < SC_CB; c++) {
                    const float *wr = w + ((size_t)(co0 + c) * CIN + ci) * (K * K) + ky * K;
#pragma unroll
                    for (int kx = 0; kx < K; kx++) {
                        const float wv = wr[kx];
#pragma unroll
                        for (int j = 0; j < SC_PX; j++) acc[c][j] = __fmaf_rn(wv, xr[j * S + kx], acc[c][j]);
                    }
                }
            }
        }
        if (oy < d.Ho && ox < d.Wo) {
#pragma unroll
            for (int c = 0; c < SC_CB; c++) {
                const size_t o = ((n * d.C_out + co0 + c) * (size_t)d.Ho + oy) * (size_t)d.Wo + ox;
                Y *p = y + o;
                if (ox + SC_PX <= d.Wo && ((uintptr_t)p & (SC_PX * sizeof(Y) - 1)) == 0) {
                    Storage<DT>::store4(p, acc[c]);
                } else {
#pragma unroll
                    for (int j = 0; j < SC_PX; j++)
                        if (ox + j < d.Wo) Storage<DT>::store1(p + j, acc[c][j]);
                }
            }
        }
    }
}

// Input pixels of one parity class: with ry = (y + pad) % S the taps of a pixel are ky = ry + S * a, reading dy row (y + pad) / S - a; likewise in x.
// The block covers SC_IR * S rows x 64 * S columns of one (sample, input channel) plane; wave w holds the class (w / S, w % S) (S = 2: four waves), a
// lane SC_IR pixels of its class in one column, S rows apart: their taps share dy rows (SC_IR + T - 1 rows loaded instead of SC_IR * T), and the
// lanes of a wave read consecutive dy columns.
constexpr int SC_IR = 4;
template <int CIN, int K, int S, int DT>
__global__ __launch_bounds__(S * S * 64) void k_sc_bwd_input(const typename Storage<DT>::T *__restrict__ dy, const float *__restrict__ w,
                                                             float *__restrict__ dx, Dims d, int bx, int by) {
    typedef typename Storage<DT>::T Y;
    constexpr int T = (K + S - 1) / S;  // taps per axis at most
    constexpr int R = SC_IR, M = R + T - 1;
    const unsigned b = blockIdx.x, ibx = b % (unsigned)bx, iby = (b / (unsigned)bx) % (unsigned)by;
    const unsigned plane = b / ((unsigned)bx * (unsigned)by);  // n * CIN + ci
    const unsigned n = plane / CIN, ci = plane - n * CIN;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int iy0 = (int)iby * (S * R) + wave / S, ix = ((int)ibx * 64 + lane) * S + wave % S;  // the lane's rows: iy0 + S * r
    const int ry = (iy0 + d.pad) % S, rx = (wave % S + d.pad) % S;                              // wave-uniform, the same for every r
    const int qy = (iy0 + d.pad) / S, qx = (ix + d.pad) / S;                                    // row r, tap a reads dy row qy + r - a
    int off[M][T];
    bool ok[M][T];
#pragma unroll
    for (int m = 0; m < M; m++)
#pragma unroll
        for (int c = 0; c < T; c++) {
            const int oy = qy + m - (T - 1), ox = qx - c;
            ok[m][c] = rx + S * c < K && oy >= 0 && oy < d.Ho && ox >= 0 && ox < d.Wo;
            off[m][c] = ok[m][c] ? oy * d.Wo + ox : 0;  // inside one (sample, channel) plane: below 2^31
        }
    const size_t HoWo = (size_t)d.Ho * d.Wo;
    const Y *dyn = dy + (size_t)n * d.C_out * HoWo;
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = 0.f;
#pragma unroll 2
    for (int co = 0; co < d.C_out; co++) {
        const float *wp = w + ((size_t)co * CIN + ci) * (K * K);
        const Y *dp = dyn + (size_t)co * HoWo;
        Y raw[M][T];  // unconditional loads (off = 0 where !ok: a valid element), all in flight; converted and masked after
        float g[M][T];
#pragma unroll
        for (int m = 0; m < M; m++)
#pragma unroll
            for (int c = 0; c < T; c++) raw[m][c] = dp[off[m][c]];
#pragma unroll
        for (int m = 0; m < M; m++)
#pragma unroll
            for (int c = 0; c < T; c++) g[m][c] = ok[m][c] ? Storage<DT>::load1(&raw[m][c]) : 0.f;
#pragma unroll
        for (int a = 0; a < T; a++)
#pragma unroll
            for (int c = 0; c < T; c++) {
                const int ky = ry + S * a, kx = rx + S * c;  // wave-uniform
                if (ky < K && kx < K) {
                    const float wv = wp[ky * K + kx];
#pragma unroll
                    for (int r = 0; r < R; r++)
                        if (ok[r - a + T - 1][c]) acc[r] = __fmaf_rn(wv, g[r - a + T - 1][c], acc[r]);
                }
            }
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int iy = iy0 + S * r;
        if (iy < d.H && ix < d.W) dx[((size_t)plane * d.H + iy) * (size_t)d.W + ix] = acc[r];
    }
}

// partial[tile][co * (CIN*K*K) + tap] for co < C_out, then partial[tile][C_out * CIN*K*K + co] = the tile's sum of dy[co]
template <int CIN, int K, int S, int DT>
__global__ __launch_bounds__(SC_THREADS) void k_sc_bwd_weight(const float *__restrict__ x, const typename Storage<DT>::T *__restrict__ dy,
                                                              float *__restrict__ partial, Dims d) {
    typedef Patch<CIN, K, S> P;
    constexpr int TAPS = CIN * K * K, NSL = SC_THREADS / TAPS, NPIX = SC_TH * SC_TW;
    static_assert(NSL >= 1 && NSL * SC_CB * TAPS <= NPIX * SC_CB, "the slices' sums reuse the dy tile's LDS");
    static_assert(NPIX % SC_THREADS == 0, "dy staging: whole pixels per thread");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *xs = reinterpret_cast<float *>(smem);
    float *gs = xs + P::ELEMS;  // dy tile [pixel][SC_CB], later the slices' sums [slice][SC_CB][TAPS]
    const unsigned b = blockIdx.x, tx = b % (unsigned)d.tiles_x, ty = (b / (unsigned)d.tiles_x) % (unsigned)d.tiles_y;
    const size_t n = b / ((unsigned)d.tiles_x * (unsigned)d.tiles_y);
    const int oy0 = (int)ty * SC_TH, ox0 = (int)tx * SC_TW;
    const int tid = threadIdx.x;
    stage_patch<CIN, K, S>(xs, x, n, d.H, d.W, oy0, ox0, d.pad);

    const int tap = tid % TAPS, slice = tid / TAPS;
    const int ci = tap / (K * K), ky = (tap - ci * K * K) / K, kx = tap - ci * K * K - ky * K;
    const float *xt = xs + (ci * P::PH + ky) * P::PITCH + kx;
    const int ph = min(SC_TH, d.Ho - oy0), pw = min(SC_TW, d.Wo - ox0);  // the tile's pixels inside the output
    const size_t HoWo = (size_t)d.Ho * d.Wo;
    const size_t M = (size_t)d.C_out * (TAPS + 1);
    float *out = partial + (size_t)b * M;
    for (int co0 = 0; co0 < d.C_out; co0 += SC_CB) {
        __syncthreads();  // the patch is staged (first round); the previous round's sums have been read
        {  // a thread stages NPIX / 256 pixels x 8 channels: every load issued before the first LDS store, zeros outside the output
            float g[NPIX / SC_THREADS][SC_CB];
            typename Storage<DT>::T raw[NPIX / SC_THREADS][SC_CB];  // unconditional loads from a clamped address, masked after
#pragma unroll
            for (int q = 0; q < NPIX / SC_THREADS; q++) {
                const int p = tid + q * SC_THREADS, py = p / SC_TW, px = p - py * SC_TW;
                const bool in = py < ph && px < pw;
                const typename Storage<DT>::T *src = dy + (n * d.C_out + co0) * HoWo + (in ? (size_t)(oy0 + py) * d.Wo + (ox0 + px) : 0);
#pragma unroll
                for (int c = 0; c < SC_CB; c++) raw[q][c] = src[(size_t)c * HoWo];
            }
#pragma unroll
            for (int q = 0; q < NPIX / SC_THREADS; q++) {
                const int p = tid + q * SC_THREADS, py = p / SC_TW, px = p - py * SC_TW;
                const bool in = py < ph && px < pw;
#pragma unroll
                for (int c = 0; c < SC_CB; c++) g[q][c] = in ? Storage<DT>::load1(&raw[q][c]) : 0.f;
            }
#pragma unroll
            for (int q = 0; q < NPIX / SC_THREADS; q++) {
                float4 *dst = reinterpret_cast<float4 *>(gs + (tid + q * SC_THREADS) * SC_CB);
                dst[0] = make_float4(g[q][0], g[q][1], g[q][2], g[q][3]);
                dst[1] = make_float4(g[q][4], g[q][5], g[q][6], g[q][7]);
            }
        }
        __syncthreads();
        float acc[SC_CB];
#pragma unroll
        for (int c = 0; c < SC_CB; c++) acc[c] = 0.f;
        if (slice < NSL) {
#pragma unroll 4
            for (int p = slice; p < NPIX; p += NSL) {
                const int py = p / SC_TW, px = p - py * SC_TW;
                {   // a pixel outside the output contributes 0 * 0, whatever x holds there (its dy is staged as zero)
                    const float xv = py < ph && px < pw ? xt[py * S * P::PITCH + px * S] : 0.f;
                    const float4 g0 = reinterpret_cast<const float4 *>(gs + p * SC_CB)[0], g1 = reinterpret_cast<const float4 *>(gs + p * SC_CB)[1];
                    acc[0] = __fmaf_rn(g0.x, xv, acc[0]); acc[1] = __fmaf_rn(g0.y, xv, acc[1]);
                    acc[2] = __fmaf_rn(g0.z, xv, acc[2]); acc[3] = __fmaf_rn(g0.w, xv, acc[3]);
                    acc[4] = __fmaf_rn(g1.x, xv, acc[4]); acc[5] = __fmaf_rn(g1.y, xv, acc[5]);
                    acc[6] = __fmaf_rn(g1.z, xv, acc[6]); acc[7] = __fmaf_rn(g1.w, xv, acc[7]);
                }
            }
        }
        // the bias gradient: 32 lanes per channel, each its pixels in index order, then an xor tree
        {
            const int c = tid >> 5, part = tid & 31;
            float s = 0.f;
            for (int p = part; p < NPIX; p += 32) s += gs[p * SC_CB + c];
#pragma unroll
            for (int m = 16; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
            if (part == 0) out[(size_t)d.C_out * TAPS + co0 + c] = s;
        }
        __syncthreads();  // every read of the dy tile is done
        if (slice < NSL) {
#pragma unroll
            for (int c = 0; c < SC_CB; c++) gs[(slice * SC_CB + c) * TAPS + tap] = acc[c];
        }
        __syncthreads();
        for (int j = tid; j < SC_CB * TAPS; j += SC_THREADS) {
            float s = gs[j];
            for (int q = 1; q < NSL; q++) s += gs[q * SC_CB * TAPS + j];
            out[(size_t)co0 * TAPS + j] = s;  // j = c * TAPS + tap
        }
    }
}

bool supported(int C_in, int C_out, int K, int stride, int pad) {
    return (C_in == 1 || C_in == 3) && K == 5 && stride == 2 && pad == 2 && C_out >= 8 && C_out <= 64 && C_out % 8 == 0;
}

// fills d; false = refused (unsupported configuration, a non-positive size, no output, 2^31 elements or more in x or y)
bool make_dims(int N, int C_in, int C_out, int H, int W, int K, int stride, int pad, Dims &d) {
    if (!supported(C_in, C_out, K, stride, pad) || N <= 0 || H <= 0 || W <= 0) return false;
    if (H + 2 * pad < K || W + 2 * pad < K) return false;
    d.N = N; d.C_out = C_out; d.H = H; d.W = W; d.pad = pad;
    d.Ho = (H + 2 * pad - K) / stride + 1;
    d.Wo = (W + 2 * pad - K) / stride + 1;
    d.tiles_y = (int)cdiv(d.Ho, SC_TH);
    d.tiles_x = (int)cdiv(d.Wo, SC_TW);
    const size_t lim = (size_t)1 << 31;
    if ((size_t)N * C_in * H * W >= lim || (size_t)N * C_out * d.Ho * d.Wo >= lim) return false;
    return true;
}

template <int CIN, int K, int S>
void launch_fwd(const float *x, const float *w, const float *bias, void *y, int y_dtype, const Dims &d, hipStream_t s) {
    const dim3 grid((unsigned)((size_t)d.N * d.tiles_y * d.tiles_x)), block(SC_THREADS);
    const size_t lds = sizeof(float) * Patch<CIN, K, S>::ELEMS;
    with_dtype(y_dtype, [&](auto t) {
        typedef decltype(t) Y;
        hipLaunchKernelGGL((k_sc_fwd<CIN, K, S, Y::DT>), grid, block, lds, s, x, w, bias, (typename Y::T *)y, d);
    });
}

template <int CIN, int K, int S>
void launch_bwd(const float *x, const float *w, const void *dy, int dy_dtype, const Dims &d, float *dx, float *dw, float *db, float *scratch,
                hipStream_t s) {
    if (dx) {
        const int bx = (int)cdiv(d.W, 64 * S), by = (int)cdiv(d.H, S * SC_IR);
        const dim3 grid((unsigned)((size_t)d.N * CIN * by * bx)), block(S * S * 64);
        with_dtype(dy_dtype, [&](auto t) {
            typedef decltype(t) Y;
            hipLaunchKernelGGL((k_sc_bwd_input<CIN, K, S, Y::DT>), grid, block, 0, s, (const typename Y::T *)dy, w, dx, d, bx, by);
        });
    }
    if (dw) {
        const int tiles = d.N * d.tiles_y * d.tiles_x, MW = d.C_out * CIN * K * K, M = MW + d.C_out;
        const size_t lds = sizeof(float) * (Patch<CIN, K, S>::ELEMS + SC_CB * SC_TH * SC_TW);
        with_dtype(dy_dtype, [&](auto t) {
            typedef decltype(t) Y;
            hipLaunchKernelGGL((k_sc_bwd_weight<CIN, K, S, Y::DT>), dim3(tiles), dim3(SC_THREADS), lds, s, x, (const typename Y::T *)dy, scratch, d);
        });
        sum_partials(scratch, tiles, SC_GROUP, M, MW, dw, db, s);
    }
}

}  // namespace

extern "C" int sc_supported(int C_in, int C_out, int K, int stride, int pad) { return supported(C_in, C_out, K, stride, pad) ? 1 : 0; }

extern "C" int sc_tile(int *tile_h, int *tile_w) {
    if (!tile_h || !tile_w) return GPSGS_E_INVALID;
    *tile_h = SC_TH;
    *tile_w = SC_TW;
    return GPSGS_OK;
}

extern "C" size_t sc_scratch_bytes(int N, int C_in, int C_out, int H, int W, int K, int stride, int pad) {
    Dims d;
    if (!make_dims(N, C_in, C_out, H, W, K, stride, pad, d)) return 0;
    const size_t tiles = (size_t)N * d.tiles_y * d.tiles_x, M = (size_t)C_out * ((size_t)C_in * K * K + 1);
    return partials_scratch_bytes(tiles, SC_GROUP, M);
}

extern "C" int sc_forward(const float *x, const float *w, const float *bias, int N, int C_in, int C_out, int H, int W, int K, int stride, int pad,
                          void *y, int y_dtype, void *stream) {
    Dims d;
    if (!make_dims(N, C_in, C_out, H, W, K, stride, pad, d)) return GPSGS_E_INVALID;
    if (!dtype_ok(y_dtype)) return GPSGS_E_INVALID;
    if (!x || !w || !bias || !y) return GPSGS_E_INVALID;
    if (!aligned(x, 16) || !aligned(y, 16) || !aligned(w, 4) || !aligned(bias, 4)) return GPSGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (C_in == 1)
        launch_fwd<1, 5, 2>(x, w, bias, y, y_dtype, d, s);
    else
        launch_fwd<3, 5, 2>(x, w, bias, y, y_dtype, d, s);
    return launched();
}

extern "C" int sc_backward(const float *x, const float *w, const void *dy, int dy_dtype, int N, int C_in, int C_out, int H, int W, int K, int stride,
                           int pad, float *dx, float *dw, float *dbias, void *scratch, void *stream) {
    Dims d;
    if (!make_dims(N, C_in, C_out, H, W, K, stride, pad, d)) return GPSGS_E_INVALID;
    if (!dtype_ok(dy_dtype)) return GPSGS_E_INVALID;
    if ((dw != nullptr) != (dbias != nullptr)) return GPSGS_E_INVALID;
    if (!x || !w || !dy || (dw && !scratch)) return GPSGS_E_INVALID;
    if (!aligned(x, 16) || !aligned(dy, 16) || !aligned(dx, 16) || !aligned(w, 4) || !aligned(dw, 4) || !aligned(dbias, 4) || !aligned(scratch, 16))
        return GPSGS_E_INVALID;
    if (!dx && !dw) return GPSGS_OK;
    hipStream_t s = (hipStream_t)stream;
    if (C_in == 1)
        launch_bwd<1, 5, 2>(x, w, dy, dy_dtype, d, dx, dw, dbias, (float *)scratch, s);
    else
        launch_bwd<3, 5, 2>(x, w, dy, dy_dtype, d, dx, dw, dbias, (float *)scratch, s);
    return launched();
}
