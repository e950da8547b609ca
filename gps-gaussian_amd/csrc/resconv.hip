// resconv.hip -- 3x3 convolution, stride 1, padding 1, with a bias, C_in -> C_out channels, on the fp32 matrix cores of gfx950, forward and backward
// (DESIGN.md "Residual-block 3x3 convolutions").
//
// conv1 and conv2 of every stride-1 ResidualBlock (core/extractor.py:10-11) are Conv2d(C_in, C_out, 3, padding=1) in fp32 wherever the block runs
// outside autocast.  Here they are implicit GEMMs on v_mfma_f32_32x32x2_f32 -- exact fp32, bit for bit an fmaf chain -- over contiguous NCHW as it
// lies: no layout transposes.  C_in a multiple of 4 in [4, 192], C_out a multiple of 16 in [16, 96], both run-time values.  The engine is
// conv3x3.hip's c3_engine with the 32-wide side made a run-time width; it is a second copy, not a shared header: the forward's weight staging gains
// a block offset and a guard, and the ReLU / mask forms go, so k_c3_* would not come out with the registers and code they have.
//
//   k_rc_fwd         one 256-thread workgroup per TH x TW = 8 x 64 output tile of one sample and one block of 32 output channels (grid y): M = 32
//                    channels, N = the tile's pixels, K = 9 C_in.  The input is walked in chunks of 4 channels: the chunk's (TH + 2) x (TW + 2) patch
//                    (taps outside the image as zeros) and its 4 x 9 x 32 weights are staged in LDS while the matrix cores work on the previous
//                    chunk.  A wave owns two rows of the tile = four 32 x 32 accumulators.  Epilogue: + bias, one store (lanes on consecutive x).
//                    A last block of 16 channels (C_out 16, 48, 80) runs half empty: the 16 x 16 x 4 form that would fill it was not built, so
//                    nothing is recorded about its cost.
//   k_rc_bwd_input   the same engine with the roles swapped: dx = conv(dy, w flipped and transposed), C_out -> C_in channels.
//   k_rc_bwd_weight  dw[co][ci, ky, kx] = sum over pixels dy[co] x[ci] shifted: M = 32 co, N = (tap, ci), K = pixels.  The grid is (pixel partition,
//                    block of 32 co, block of 64 ci).  A workgroup walks the 4 x 32 pixel tiles b, b + P, b + 2P, ... of its partition b in index
//                    order with its 32 x 9 x 64 sums in accumulators (18 blocks of 32 x 32 over 4 waves), dy [32][128] and the patch of 32 input
//                    channels in LDS; it writes its block of partial b (the ci = 0 blocks also the bias sums) to scratch.
//   k_sum_partials   (op_reduce.h) adds the partials in index order, in groups of RC_GROUP and then the groups.
// No atomics, no memset; every sum has a fixed order: the same bits on every run.  Element offsets are 64-bit.  Guarded global loads are an
// unconditional load from a clamped (always valid) address followed by a select (stem_conv.hip).
//
// Scratch: parts = min(RC_WGS / (ceil(C_out / 32) ceil(C_in / 64)), N ceil(H / 4) ceil(W / 32)) partials of M = C_out (9 C_in + 1) floats and their
// ceil(parts / 32) group sums: 4 M (parts + ceil(parts / 32)) bytes, at most 39.0 MB (C_out 96, C_in 64: 170 partials) -- under 64 MiB for every
// supported call.
//
// Compiler figures (hipcc -O3, gfx950; VGPRs include the accumulation registers; no kernel uses scratch memory):
//   k_rc_fwd         151 VGPRs, 0 spilled, 16,384 B LDS   3 waves per SIMD by registers; launch bound 2 workgroups per CU
//   k_rc_bwd_input   151 VGPRs, 0 spilled, 16,384 B LDS   likewise
//   k_rc_bwd_weight  143 VGPRs + 96 accumulation registers = 239, 0 spilled (36 SGPRs kept in VGPR lanes), 43,008 B LDS: 2 waves per SIMD by
//                    registers, three workgroups per CU by LDS
// Accumulator layout of the MFMA (corr_pyramid.hip tile_gemm): register v of lane l is row (v / 4) * 8 + (l / 32) * 4 + v % 4, column l % 32; the
// A operand of lane l is A[l % 32][l / 32], the B operand B[l / 32][l % 32].
#include "op_reduce.h"

namespace {

typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int RC_MINCI = 4, RC_MAXCI = 192, RC_MINCO = 16, RC_MAXCO = 96;
constexpr int RC_TH = 8, RC_TW = 64;       // output tile of the forward and of the input gradient
constexpr int RC_THREADS = 256;
constexpr int RC_CK = 4;                   // reduction channels staged per step
constexpr int RC_PH = RC_TH + 2, RC_PW = RC_TW + 2, RC_PITCH = 68;
constexpr int RC_PLANE = 736;              // >= PH * PITCH, and 32 banks past a multiple of 64: the two lane halves (two channels) never collide
static_assert(RC_PLANE >= RC_PH * RC_PITCH && RC_PLANE % 64 == 32, "patch plane");

constexpr int RC_WTH = 4, RC_WTW = 32, RC_WPIX = RC_WTH * RC_WTW;  // pixel tile of the weight gradient
constexpr int RC_WPW = RC_WTW + 2, RC_WPE = (RC_WTH + 2) * RC_WPW;  // its patch: 6 x 34
constexpr int RC_WPLANE = 206;             // >= 204; 2 * odd: 32 channels (lanes) x 2 neighbouring pixels (lane halves) hit 64 different banks
constexpr int RC_GP = RC_WPIX + 2;         // pitch of the dy tile, likewise
constexpr int RC_WCI = 64;                 // input channels of a workgroup of the weight gradient
constexpr int RC_WGS = 512;                // workgroups of k_rc_bwd_weight at most: partitions x blocks
constexpr int RC_GROUP = 32;               // partials per first-stage group of the reduction
static_assert(RC_WPLANE >= RC_WPE && (RC_WPLANE / 2) % 2 == 1 && (RC_GP / 2) % 2 == 1, "weight-gradient LDS pitches");

struct RcDims {
    int N, Ci, Co, H, W, tiles_x, tiles_y;  // the layer's C_in and C_out; tiles of TH x TW
};

// One TH x TW tile of out[n, cob .. cob + 32) = conv3x3(in[n, 0..CI)), cob = 32 blockIdx.y: forward CI = C_in, CO = C_out, weights w[co][ci][tap];
// BWD CI = C_out, CO = C_in, the weight of (out ci, in co, tap) is w[co][ci][8 - tap].  Output channels past CO are zero weights, never stored.
template <bool BWD>
__device__ __forceinline__ void rc_engine(const float *__restrict__ in, const float *__restrict__ w, const float *__restrict__ bias,
                                          float *__restrict__ out, const RcDims &d, float *xs, float *ws) {
    constexpr int COP = 32;
    constexpr int WPL = 9 * COP;  // per staged channel: consecutive channels 32 banks apart
    static_assert(WPL % 64 == 32, "weight plane");
    constexpr int XE = RC_CK * RC_PH * RC_PW, XI = (XE + RC_THREADS - 1) / RC_THREADS;
    constexpr int WE = RC_CK * 9 * COP, WI = (WE + RC_THREADS - 1) / RC_THREADS;
    const int CI = BWD ? d.Co : d.Ci, CO = BWD ? d.Ci : d.Co, cob = (int)blockIdx.y * 32;
    const unsigned b = blockIdx.x, tx = b % (unsigned)d.tiles_x, ty = (b / (unsigned)d.tiles_x) % (unsigned)d.tiles_y;
    const size_t n = b / ((unsigned)d.tiles_x * (unsigned)d.tiles_y);
    const int oy0 = (int)ty * RC_TH, ox0 = (int)tx * RC_TW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const size_t HW = (size_t)d.H * d.W;
    const float *inn = in + n * CI * HW;

    float xv[XI], wv[WI];
    auto load = [&](int c0) {
#pragma unroll
        for (int i = 0; i < XI; i++) {
            const int e = tid + i * RC_THREADS;
            const int cl = e / (RC_PH * RC_PW), rem = e - cl * (RC_PH * RC_PW), r = rem / RC_PW, c = rem - r * RC_PW;
            const int iy = oy0 - 1 + r, ix = ox0 - 1 + c;
            const bool ok = e < XE && iy >= 0 && iy < d.H && ix >= 0 && ix < d.W;
            const size_t off = ok ? (size_t)(c0 + cl) * HW + (size_t)iy * d.W + ix : 0;
            const float t = inn[off];
            xv[i] = ok ? t : 0.f;
        }
#pragma unroll
        for (int i = 0; i < WI; i++) {
            const int e = tid + i * RC_THREADS;
            bool ok = e < WE;
            size_t src;
            if (BWD) {
                const int cl = e / (COP * 9), rem = e - cl * (COP * 9), ci = rem / 9;
                ok = ok && cob + ci < CO;
                src = ((size_t)(c0 + cl) * CO + cob) * 9 + rem;  // w[c0 + cl][cob + ci][tap], rem = ci * 9 + tap
            } else {
                const int co = e / (RC_CK * 9), r = e - co * (RC_CK * 9);
                ok = ok && cob + co < CO;
                src = ((size_t)(cob + co) * CI + c0) * 9 + r;  // w[cob + co][c0 + cl][tap], r = cl * 9 + tap
            }
            const float t = w[ok ? src : 0];
            wv[i] = ok ? t : 0.f;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < XI; i++) {
            const int e = tid + i * RC_THREADS;
            const int cl = e / (RC_PH * RC_PW), rem = e - cl * (RC_PH * RC_PW), r = rem / RC_PW, c = rem - r * RC_PW;
            if (e < XE) xs[cl * RC_PLANE + r * RC_PITCH + c] = xv[i];
        }
#pragma unroll
        for (int i = 0; i < WI; i++) {
            const int e = tid + i * RC_THREADS;
            if (e < WE) {
                if (BWD) {
                    const int cl = e / (COP * 9), rem = e - cl * (COP * 9), ci = rem / 9, tap = rem - ci * 9;
                    ws[cl * WPL + (8 - tap) * COP + ci] = wv[i];
                } else {
                    const int co = e / (RC_CK * 9), r = e - co * (RC_CK * 9), cl = r / 9, tap = r - cl * 9;
                    ws[cl * WPL + tap * COP + co] = wv[i];
                }
            }
        }
    };

    v16f acc[4];  // [row of the wave's two * half of the 64 columns]
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int v = 0; v < 16; v++) acc[t][v] = 0.f;
    const int r0 = wave * 2;
    load(0);
#pragma unroll 1
    for (int c0 = 0; c0 < CI; c0 += RC_CK) {
        __syncthreads();  // every wave is done reading the previous chunk
        store();
        __syncthreads();
        if (c0 + RC_CK < CI) load(c0 + RC_CK);  // in flight while the matrix cores work on this chunk
#pragma unroll
        for (int pair = 0; pair < RC_CK; pair += 2) {
            const float *xp = xs + (pair + half) * RC_PLANE + r0 * RC_PITCH + l31;
            const float *wp = ws + (pair + half) * WPL + l31;
#pragma unroll
            for (int tap = 0; tap < 9; tap++) {
                const int ky = tap / 3, kx = tap - ky * 3;
                float p[4];
                const float a = wp[tap * COP];
#pragma unroll
                for (int t = 0; t < 4; t++) p[t] = xp[((t >> 1) + ky) * RC_PITCH + (t & 1) * 32 + kx];
#pragma unroll
                for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, p[t], acc[t], 0, 0, 0);
            }
        }
    }
    float *outn = out + n * CO * HW;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int oy = oy0 + r0 + (t >> 1), ox = ox0 + (t & 1) * 32 + l31;
        if (oy < d.H && ox < d.W) {
            float *o = outn + (size_t)oy * d.W + ox;
#pragma unroll
            for (int v = 0; v < 16; v++) {
                const int co = cob + (v >> 2) * 8 + half * 4 + (v & 3);
                if (co < CO) {
                    float val = acc[t][v];
                    if (!BWD) val += bias[co];
                    o[(size_t)co * HW] = val;
                }
            }
        }
    }
}

// (launch bounds: read against the compiler's register counts -- 64 accumulator registers + the staged chunk + addresses: 3 waves per SIMD)
__global__ __launch_bounds__(RC_THREADS, 2) void k_rc_fwd(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias,
                                                          float *__restrict__ y, RcDims d) {
    __shared__ float xs[RC_CK * RC_PLANE];
    __shared__ float ws[RC_CK * 9 * 32];
    rc_engine<false>(x, w, bias, y, d, xs, ws);
}

__global__ __launch_bounds__(RC_THREADS, 2) void k_rc_bwd_input(const float *__restrict__ dy, const float *__restrict__ w, float *__restrict__ dx,
                                                                RcDims d) {
    __shared__ float xs[RC_CK * RC_PLANE];
    __shared__ float ws[RC_CK * 9 * 32];
    rc_engine<true>(dy, w, nullptr, dx, d, xs, ws);
}

// partial[b][(co * C_in + ci) * 9 + tap], then partial[b][C_out * 9 * C_in + co] = partition b's sum of dy[co]; b = blockIdx.x, co in the block of 32
// from 32 blockIdx.y, ci in the block of 64 from 64 blockIdx.z (the bias sums from the blockIdx.z = 0 workgroups)
// (launch bound: the 96 accumulator registers + staging and addresses, two waves per SIMD; 43 KB of LDS allow three workgroups per CU)
__global__ __launch_bounds__(RC_THREADS, 1) void k_rc_bwd_weight(const float *__restrict__ x, const float *__restrict__ dy, float *__restrict__ partial,
                                                                 RcDims d, int wtx, int wty, int tiles) {
    __shared__ float xs[32 * RC_WPLANE];
    __shared__ float gs[32 * RC_GP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const size_t HW = (size_t)d.H * d.W;
    const int Ci = d.Ci, Co = d.Co, cob = (int)blockIdx.y * 32, cib = (int)blockIdx.z * RC_WCI;
    v16f acc[2][3];  // [block of 32 input channels][slot]: block cc, slot s holds tap ((wave + 3 cc) & 3) + 4 s where that is < 9 -- 5, 5, 4, 4 per wave
#pragma unroll
    for (int cc = 0; cc < 2; cc++)
#pragma unroll
        for (int s = 0; s < 3; s++)
#pragma unroll
            for (int v = 0; v < 16; v++) acc[cc][s][v] = 0.f;
    float dbsum = 0.f;
#pragma unroll 1
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int tx = t % wtx, ty = (t / wtx) % wty;
        const size_t n = (size_t)(t / (wtx * wty));
        const int oy0 = ty * RC_WTH, ox0 = tx * RC_WTW;
        __syncthreads();  // the previous tile has been read
        {
            constexpr int GI = 32 * RC_WPIX / RC_THREADS;  // 16
            float g[GI];
#pragma unroll
            for (int i = 0; i < GI; i++) {
                const int e = tid + i * RC_THREADS, co = e / RC_WPIX, p = e - co * RC_WPIX, py = p / RC_WTW, px = p - py * RC_WTW;
                const bool ok = cob + co < Co && oy0 + py < d.H && ox0 + px < d.W;
                const size_t off = ok ? (n * Co + cob + co) * HW + (size_t)(oy0 + py) * d.W + (ox0 + px) : 0;
                const float v = dy[off];
                g[i] = ok ? v : 0.f;
            }
#pragma unroll
            for (int i = 0; i < GI; i++) {
                const int e = tid + i * RC_THREADS, co = e / RC_WPIX, p = e - co * RC_WPIX;
                gs[co * RC_GP + p] = g[i];
            }
        }
#pragma unroll
        for (int cc = 0; cc < 2; cc++) {
            const int c0 = cib + cc * 32;
            if (c0 < Ci) {  // (uniform)
                if (cc > 0) __syncthreads();  // the first block's patch has been read
                constexpr int XE = 32 * RC_WPE, BATCH = 13, IT = (XE + RC_THREADS - 1) / RC_THREADS;  // 26 loads per thread, 13 in flight
                static_assert(IT % BATCH == 0, "patch staging batches");
#pragma unroll 1
                for (int i0 = 0; i0 < IT; i0 += BATCH) {
                    float v[BATCH];
#pragma unroll
                    for (int i = 0; i < BATCH; i++) {
                        const int e = tid + (i0 + i) * RC_THREADS, ci = e / RC_WPE, rem = e - ci * RC_WPE, r = rem / RC_WPW, c = rem - r * RC_WPW;
                        const int iy = oy0 - 1 + r, ix = ox0 - 1 + c;
                        const bool ok = e < XE && c0 + ci < Ci && iy >= 0 && iy < d.H && ix >= 0 && ix < d.W;
                        const float tv = x[ok ? (n * Ci + c0 + ci) * HW + (size_t)iy * d.W + ix : 0];
                        v[i] = ok ? tv : 0.f;
                    }
#pragma unroll
                    for (int i = 0; i < BATCH; i++) {
                        const int e = tid + (i0 + i) * RC_THREADS, ci = e / RC_WPE, rem = e - ci * RC_WPE;
                        if (e < XE) xs[ci * RC_WPLANE + rem] = v[i];
                    }
                }
                __syncthreads();
                if (cc == 0) {  // the bias gradient: 8 lanes per channel, each 16 pixels in index order, then an xor tree
                    const int co = tid >> 3, part = tid & 7;
                    float s = 0.f;
#pragma unroll
                    for (int q = 0; q < RC_WPIX / 8; q++) s += gs[co * RC_GP + part * (RC_WPIX / 8) + q];
#pragma unroll
                    for (int m = 4; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
                    dbsum += s;
                }
                const int tap0 = (wave + 3 * cc) & 3;
                int xo[3];
#pragma unroll
                for (int s = 0; s < 3; s++) {
                    const int tap = min(tap0 + 4 * s, 8), ky = tap / 3, kx = tap - ky * 3;
                    xo[s] = l31 * RC_WPLANE + ky * RC_WPW + kx;
                }
                const bool third = tap0 + 8 < 9;  // (wave-uniform)
                const float *gp = gs + l31 * RC_GP + half;
#pragma unroll 4
                for (int p = 0; p < RC_WPIX; p += 2) {
                    const int q = p + half, py = q / RC_WTW, px = q - py * RC_WTW, po = py * RC_WPW + px;
                    const float a = gp[p];
                    const float b0 = xs[xo[0] + po], b1 = xs[xo[1] + po];
                    acc[cc][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc[cc][0], 0, 0, 0);
                    acc[cc][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc[cc][1], 0, 0, 0);
                    if (third) {
                        const float b2 = xs[xo[2] + po];
                        acc[cc][2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b2, acc[cc][2], 0, 0, 0);
                    }
                }
            }
        }
    }
    const size_t MW = (size_t)Co * 9 * Ci;
    float *out = partial + (size_t)blockIdx.x * (MW + Co);
#pragma unroll
    for (int cc = 0; cc < 2; cc++) {
        const int ci = cib + cc * 32 + l31, tap0 = (wave + 3 * cc) & 3;
#pragma unroll
        for (int s = 0; s < 3; s++) {
            const int tap = tap0 + 4 * s;
            if (tap < 9 && ci < Ci) {
#pragma unroll
                for (int v = 0; v < 16; v++) {
                    const int co = cob + (v >> 2) * 8 + half * 4 + (v & 3);
                    if (co < Co) out[((size_t)co * Ci + ci) * 9 + tap] = acc[cc][s][v];
                }
            }
        }
    }
    if (cib == 0 && (tid & 7) == 0 && cob + (tid >> 3) < Co) out[MW + cob + (tid >> 3)] = dbsum;
}

bool supported(int C_in, int C_out) {
    return C_in >= RC_MINCI && C_in <= RC_MAXCI && C_in % 4 == 0 && C_out >= RC_MINCO && C_out <= RC_MAXCO && C_out % 16 == 0;
}

// fills d; false = refused (unsupported channel counts, a non-positive size, 2^31 elements or more in x or y)
bool make_dims(int N, int C_in, int C_out, int H, int W, RcDims &d) {
    if (!supported(C_in, C_out) || N <= 0 || H <= 0 || W <= 0) return false;
    const size_t lim = (size_t)1 << 31;
    const size_t plane = (size_t)H * W;  // < 2^62
    if (plane >= lim || (size_t)N * plane >= lim) return false;  // N * plane < 2^62
    const size_t np = (size_t)N * plane;                          // < 2^31: times 192 channels at most cannot overflow
    if (np * C_in >= lim || np * C_out >= lim) return false;
    d.N = N; d.Ci = C_in; d.Co = C_out; d.H = H; d.W = W;
    d.tiles_y = (int)cdiv(H, RC_TH);
    d.tiles_x = (int)cdiv(W, RC_TW);
    return true;
}

size_t weight_tiles(const RcDims &d) { return (size_t)d.N * cdiv(d.H, RC_WTH) * cdiv(d.W, RC_WTW); }
size_t weight_parts(const RcDims &d) {
    const size_t t = weight_tiles(d), cap = (size_t)RC_WGS / (cdiv(d.Co, 32) * cdiv(d.Ci, RC_WCI));  // >= 512 / 9
    return t < cap ? t : cap;
}

}  // namespace

extern "C" int rc_supported(int C_in, int C_out) { return supported(C_in, C_out) ? 1 : 0; }

extern "C" int rc_tile(int *tile_h, int *tile_w) {
    if (!tile_h || !tile_w) return GPSGS_E_INVALID;
    *tile_h = RC_TH;
    *tile_w = RC_TW;
    return GPSGS_OK;
}

extern "C" size_t rc_scratch_bytes(int N, int C_in, int C_out, int H, int W) {
    RcDims d;
    if (!make_dims(N, C_in, C_out, H, W, d)) return 0;
    return partials_scratch_bytes(weight_parts(d), RC_GROUP, (size_t)C_out * (9 * (size_t)C_in + 1));
}

extern "C" int rc_forward(const float *x, const float *w, const float *bias, int N, int C_in, int C_out, int H, int W, float *y, void *stream) {
    RcDims d;
    if (!make_dims(N, C_in, C_out, H, W, d)) return GPSGS_E_INVALID;
    if (!x || !w || !bias || !y) return GPSGS_E_INVALID;
    if (!aligned(x, 16) || !aligned(y, 16) || !aligned(w, 4) || !aligned(bias, 4)) return GPSGS_E_INVALID;
    const dim3 grid((unsigned)((size_t)d.N * d.tiles_y * d.tiles_x), (unsigned)cdiv(C_out, 32)), block(RC_THREADS);
    hipLaunchKernelGGL(k_rc_fwd, grid, block, 0, (hipStream_t)stream, x, w, bias, y, d);
    return launched();
}

extern "C" int rc_backward(const float *x, const float *w, const float *dy, int N, int C_in, int C_out, int H, int W, float *dx, float *dw,
                           float *dbias, void *scratch, void *stream) {
    RcDims d;
    if (!make_dims(N, C_in, C_out, H, W, d)) return GPSGS_E_INVALID;
    if ((dw != nullptr) != (dbias != nullptr)) return GPSGS_E_INVALID;
    if (!x || !w || !dy || (dw && !scratch)) return GPSGS_E_INVALID;
    if (!aligned(x, 16) || !aligned(dy, 16) || !aligned(dx, 16) || !aligned(w, 4) || !aligned(dw, 4) || !aligned(dbias, 4) || !aligned(scratch, 16))
        return GPSGS_E_INVALID;
    if (!dx && !dw) return GPSGS_OK;
    hipStream_t s = (hipStream_t)stream;
    if (dx) {
        const dim3 grid((unsigned)((size_t)d.N * d.tiles_y * d.tiles_x), (unsigned)cdiv(C_in, 32)), block(RC_THREADS);
        hipLaunchKernelGGL(k_rc_bwd_input, grid, block, 0, s, dy, w, dx, d);
    }
    if (dw) {
        const int tiles = (int)weight_tiles(d), parts = (int)weight_parts(d), wtx = (int)cdiv(d.W, RC_WTW), wty = (int)cdiv(d.H, RC_WTH);
        const int MW = C_out * 9 * C_in, M = MW + C_out;
        float *part = (float *)scratch;
        const dim3 grid((unsigned)parts, (unsigned)cdiv(C_out, 32), (unsigned)cdiv(C_in, RC_WCI));
        hipLaunchKernelGGL(k_rc_bwd_weight, grid, dim3(RC_THREADS), 0, s, x, dy, part, d, wtx, wty, tiles);
        sum_partials(part, parts, RC_GROUP, M, MW, dw, dbias, s);
    }
    return launched();
}
