// conv3x3.hip -- 3x3 convolution, stride 1, padding 1, to or from 32 channels, on the fp32 matrix cores of gfx950, forward and backward
// (DESIGN.md "Full-resolution 3x3 convolutions").
//
// The regresser's full-resolution stage is Conv2d(52, 32, 3, padding=1) + ReLU and, at the top of each head, Conv2d(32, 32, 3, padding=1), all in
// fp32.  Here they are implicit GEMMs on v_mfma_f32_32x32x2_f32 -- exact fp32, bit for bit an fmaf chain -- over contiguous NCHW as it lies: no
// layout transposes.  C_out = 32, C_in a multiple of 4 in [4, 64].
//
//   k_c3_fwd         one 256-thread workgroup per TH x TW = 8 x 64 output tile of one sample: M = 32 channels, N = the tile's pixels, K = 9 C_in.
//                    The input is walked in chunks of 4 channels: the chunk's (TH + 2) x (TW + 2) patch (taps outside the image as zeros) and its
//                    4 x 9 x 32 weights are staged in LDS while the matrix cores work on the previous chunk.  A wave owns two rows of the tile =
//                    four 32 x 32 accumulators, so one weight fetch serves four MFMAs; the pixel operand is read per tap from the patch, consecutive
//                    lanes on consecutive x.  Epilogue: + bias, the optional ReLU, one store (lanes on consecutive x: 128-byte rows).
//   k_c3_bwd_input   the same engine with the roles swapped: dx = conv(g, w flipped and transposed), 32 -> C_in channels (one workgroup per block of
//                    32 of them: grid y); for the ReLU form g = dy [y > 0], the mask taken from the saved y while dy is staged.
//   k_c3_bwd_weight  dw[co][ci, ky, kx] = sum over pixels g[co] x[ci] shifted: M = 32 co, N = (tap, ci), K = pixels.  A workgroup walks the 4 x 32
//                    pixel tiles b, b + G, b + 2G, ... in index order with all 32 x 9 C_in sums in accumulators (18 blocks of 32 x 32 over 4 waves),
//                    g [32][128] and the patch of 32 input channels in LDS; it writes ONE partial (and its bias sums) to scratch.
//   k_sum_partials   (op_reduce.h) adds the workgroups' partials in index order, in groups of C3_GROUP and then the groups.
// No atomics; every sum has a fixed order: the same bits on every run.  Element offsets are 64-bit.  Guarded global loads are an unconditional load
// from a clamped (always valid) address followed by a select (stem_conv.hip).
// Accumulator layout of the MFMA (corr_pyramid.hip tile_gemm): register v of lane l is row (v / 4) * 8 + (l / 32) * 4 + v % 4, column l % 32; the
// A operand of lane l is A[l % 32][l / 32], the B operand B[l / 32][l % 32].
#include "op_reduce.h"

namespace {

typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int C3_CO = 32;                  // the channel count on the 32-wide side
constexpr int C3_TH = 8, C3_TW = 64;       // output tile of the forward and of the input gradient
constexpr int C3_THREADS = 256;
constexpr int C3_CK = 4;                   // input channels staged per step
constexpr int C3_PH = C3_TH + 2, C3_PW = C3_TW + 2, C3_PITCH = 68;
constexpr int C3_PLANE = 736;              // >= PH * PITCH, and 32 banks past a multiple of 64: the two lane halves (two channels) never collide
static_assert(C3_PLANE >= C3_PH * C3_PITCH && C3_PLANE % 64 == 32, "patch plane");

constexpr int C3_WTH = 4, C3_WTW = 32, C3_WPIX = C3_WTH * C3_WTW;  // pixel tile of the weight gradient
constexpr int C3_WPW = C3_WTW + 2, C3_WPE = (C3_WTH + 2) * C3_WPW;  // its patch: 6 x 34
constexpr int C3_WPLANE = 206;             // >= 204; 2 * odd: 32 channels (lanes) x 2 neighbouring pixels (lane halves) hit 64 different banks
constexpr int C3_GP = C3_WPIX + 2;         // pitch of the g tile, likewise
constexpr int C3_PARTS = 512;              // partials of the weight gradient at most (workgroups of k_c3_bwd_weight)
constexpr int C3_GROUP = 32;               // partials per first-stage group of the reduction
static_assert(C3_WPLANE >= C3_WPE && (C3_WPLANE / 2) % 2 == 1 && (C3_GP / 2) % 2 == 1, "weight-gradient LDS pitches");

struct C3Dims {
    int N, C, H, W, tiles_x, tiles_y;  // C = the layer's C_in; tiles of TH x TW
};

// One TH x TW tile of out[n, 0..CO) = conv3x3(in[n, 0..CI)): forward CI = C, CO = 32, weights w[co][ci][tap]; BWD CI = 32, CO = C, the weight of
// (out ci, in co, tap) is w[co][ci][8 - tap].  MASK: in = dy where ym > 0, else 0.  A workgroup computes the 32 output channels from 32 blockIdx.y on
// (BWD with C > 32: two blocks, the second partly empty; holding both in one workgroup took 264 registers, one wave per SIMD: measured 1,057 us
// against 740 us this way for dx of [2,52,1024,1024]).
template <bool BWD, bool MASK, bool RELU>
__device__ __forceinline__ void c3_engine(const float *__restrict__ in, const float *__restrict__ ym, const float *__restrict__ w,
                                          const float *__restrict__ bias, float *__restrict__ out, const C3Dims &d, float *xs, float *ws) {
    constexpr int COP = 32;
    constexpr int WPL = 9 * COP;  // per staged channel: consecutive channels 32 banks apart
    static_assert(WPL % 64 == 32, "weight plane");
    constexpr int XE = C3_CK * C3_PH * C3_PW, XI = (XE + C3_THREADS - 1) / C3_THREADS;
    constexpr int WE = C3_CK * 9 * COP, WI = (WE + C3_THREADS - 1) / C3_THREADS;
    const int CI = BWD ? C3_CO : d.C, CO = BWD ? d.C : C3_CO, cob = (int)blockIdx.y * 32;
    const unsigned b = blockIdx.x, tx = b % (unsigned)d.tiles_x, ty = (b / (unsigned)d.tiles_x) % (unsigned)d.tiles_y;
    const size_t n = b / ((unsigned)d.tiles_x * (unsigned)d.tiles_y);
    const int oy0 = (int)ty * C3_TH, ox0 = (int)tx * C3_TW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const size_t HW = (size_t)d.H * d.W;
    const float *inn = in + n * CI * HW;
    const float *ymn = MASK ? ym + n * CI * HW : nullptr;

    float xv[XI], wv[WI];
    auto load = [&](int c0) {
#pragma unroll
        for (int i = 0; i < XI; i++) {
            const int e = tid + i * C3_THREADS;
            const int cl = e / (C3_PH * C3_PW), rem = e - cl * (C3_PH * C3_PW), r = rem / C3_PW, c = rem - r * C3_PW;
            const int iy = oy0 - 1 + r, ix = ox0 - 1 + c;
            const bool ok = e < XE && iy >= 0 && iy < d.H && ix >= 0 && ix < d.W;
            const size_t off = ok ? (size_t)(c0 + cl) * HW + (size_t)iy * d.W + ix : 0;
            float t = inn[off];
            if (MASK) t = ymn[off] > 0.f ? t : 0.f;
            xv[i] = ok ? t : 0.f;
        }
#pragma unroll
        for (int i = 0; i < WI; i++) {
            const int e = tid + i * C3_THREADS;
            bool ok = e < WE;
            size_t src;
            if (BWD) {
                const int cl = e / (COP * 9), rem = e - cl * (COP * 9), ci = rem / 9;
                ok = ok && cob + ci < CO;
                src = ((size_t)(c0 + cl) * CO + cob) * 9 + rem;  // w[c0 + cl][cob + ci][tap], rem = ci * 9 + tap
            } else {
                const int co = e / (C3_CK * 9), r = e - co * (C3_CK * 9);
                src = ((size_t)co * CI + c0) * 9 + r;  // w[co][c0 + cl][tap], r = cl * 9 + tap
            }
            const float t = w[ok ? src : 0];
            wv[i] = ok ? t : 0.f;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < XI; i++) {
            const int e = tid + i * C3_THREADS;
            const int cl = e / (C3_PH * C3_PW), rem = e - cl * (C3_PH * C3_PW), r = rem / C3_PW, c = rem - r * C3_PW;
            if (e < XE) xs[cl * C3_PLANE + r * C3_PITCH + c] = xv[i];
        }
#pragma unroll
        for (int i = 0; i < WI; i++) {
            const int e = tid + i * C3_THREADS;
            if (e < WE) {
                if (BWD) {
                    const int cl = e / (COP * 9), rem = e - cl * (COP * 9), ci = rem / 9, tap = rem - ci * 9;
                    ws[cl * WPL + (8 - tap) * COP + ci] = wv[i];
                } else {
                    const int co = e / (C3_CK * 9), r = e - co * (C3_CK * 9), cl = r / 9, tap = r - cl * 9;
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
    for (int c0 = 0; c0 < CI; c0 += C3_CK) {
        __syncthreads();  // every wave is done reading the previous chunk
        store();
        __syncthreads();
        if (c0 + C3_CK < CI) load(c0 + C3_CK);  // in flight while the matrix cores work on this chunk
#pragma unroll
        for (int pair = 0; pair < C3_CK; pair += 2) {
            const float *xp = xs + (pair + half) * C3_PLANE + r0 * C3_PITCH + l31;
            const float *wp = ws + (pair + half) * WPL + l31;
#pragma unroll
            for (int tap = 0; tap < 9; tap++) {
                const int ky = tap / 3, kx = tap - ky * 3;
                float p[4];
                const float a = wp[tap * COP];
#pragma unroll
                for (int t = 0; t < 4; t++) p[t] = xp[((t >> 1) + ky) * C3_PITCH + (t & 1) * 32 + kx];
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
                    if (RELU) val = val < 0.f ? 0.f : val;
                    o[(size_t)co * HW] = val;
                }
            }
        }
    }
}

// (launch bounds: read against the compiler's register counts -- 64 accumulator registers + the staged chunk + addresses: about 150, 3 waves per SIMD)
template <bool RELU>
__global__ __launch_bounds__(C3_THREADS, 2) void k_c3_fwd(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias,
                                                          float *__restrict__ y, C3Dims d) {
    __shared__ float xs[C3_CK * C3_PLANE];
    __shared__ float ws[C3_CK * 9 * 32];
    c3_engine<false, false, RELU>(x, nullptr, w, bias, y, d, xs, ws);
}

template <bool MASK>
__global__ __launch_bounds__(C3_THREADS, 2) void k_c3_bwd_input(const float *__restrict__ dy, const float *__restrict__ y, const float *__restrict__ w,
                                                                float *__restrict__ dx, C3Dims d) {
    __shared__ float xs[C3_CK * C3_PLANE];
    __shared__ float ws[C3_CK * 9 * 32];
    c3_engine<true, MASK, false>(dy, y, w, nullptr, dx, d, xs, ws);
}

// partial[b][(co * C + ci) * 9 + tap], then partial[b][32 * 9 * C + co] = the workgroup's sum of g[co]
// (launch bound: 126 VGPRs + the 96 accumulator registers = 222, two waves per SIMD; 43 KB of LDS allow three workgroups per CU)
template <bool MASK>
__global__ __launch_bounds__(C3_THREADS, 1) void k_c3_bwd_weight(const float *__restrict__ x, const float *__restrict__ dy, const float *__restrict__ y,
                                                                 float *__restrict__ partial, C3Dims d, int wtx, int wty, int tiles) {
    __shared__ float xs[32 * C3_WPLANE];
    __shared__ float gs[C3_CO * C3_GP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const size_t HW = (size_t)d.H * d.W;
    const int C = d.C;
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
        const int oy0 = ty * C3_WTH, ox0 = tx * C3_WTW;
        __syncthreads();  // the previous tile has been read
        {
            constexpr int GI = C3_CO * C3_WPIX / C3_THREADS;  // 16
            float g[GI];
#pragma unroll
            for (int i = 0; i < GI; i++) {
                const int e = tid + i * C3_THREADS, co = e / C3_WPIX, p = e - co * C3_WPIX, py = p / C3_WTW, px = p - py * C3_WTW;
                const bool ok = oy0 + py < d.H && ox0 + px < d.W;
                const size_t off = ok ? (n * C3_CO + co) * HW + (size_t)(oy0 + py) * d.W + (ox0 + px) : 0;
                float v = dy[off];
                if (MASK) v = y[off] > 0.f ? v : 0.f;
                g[i] = ok ? v : 0.f;
            }
#pragma unroll
            for (int i = 0; i < GI; i++) {
                const int e = tid + i * C3_THREADS, co = e / C3_WPIX, p = e - co * C3_WPIX;
                gs[co * C3_GP + p] = g[i];
            }
        }
#pragma unroll
        for (int cc = 0; cc < 2; cc++) {
            const int c0 = cc * 32;
            if (c0 < C) {  // (uniform)
                if (cc > 0) __syncthreads();  // the first block's patch has been read
                constexpr int XE = 32 * C3_WPE, BATCH = 13, IT = (XE + C3_THREADS - 1) / C3_THREADS;  // 26 loads per thread, 13 in flight
                static_assert(IT % BATCH == 0, "patch staging batches");
#pragma unroll 1
                for (int i0 = 0; i0 < IT; i0 += BATCH) {
                    float v[BATCH];
#pragma unroll
                    for (int i = 0; i < BATCH; i++) {
                        const int e = tid + (i0 + i) * C3_THREADS, ci = e / C3_WPE, rem = e - ci * C3_WPE, r = rem / C3_WPW, c = rem - r * C3_WPW;
                        const int iy = oy0 - 1 + r, ix = ox0 - 1 + c;
                        const bool ok = e < XE && c0 + ci < C && iy >= 0 && iy < d.H && ix >= 0 && ix < d.W;
                        const float tv = x[ok ? (n * C + c0 + ci) * HW + (size_t)iy * d.W + ix : 0];
                        v[i] = ok ? tv : 0.f;
                    }
#pragma unroll
                    for (int i = 0; i < BATCH; i++) {
                        const int e = tid + (i0 + i) * C3_THREADS, ci = e / C3_WPE, rem = e - ci * C3_WPE;
                        if (e < XE) xs[ci * C3_WPLANE + rem] = v[i];
                    }
                }
                __syncthreads();
                if (cc == 0) {  // the bias gradient: 8 lanes per channel, each 16 pixels in index order, then an xor tree
                    const int co = tid >> 3, part = tid & 7;
                    float s = 0.f;
#pragma unroll
                    for (int q = 0; q < C3_WPIX / 8; q++) s += gs[co * C3_GP + part * (C3_WPIX / 8) + q];
#pragma unroll
                    for (int m = 4; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
                    dbsum += s;
                }
                const int tap0 = (wave + 3 * cc) & 3;
                int xo[3];
#pragma unroll
                for (int s = 0; s < 3; s++) {
                    const int tap = min(tap0 + 4 * s, 8), ky = tap / 3, kx = tap - ky * 3;
                    xo[s] = l31 * C3_WPLANE + ky * C3_WPW + kx;
                }
                const bool third = tap0 + 8 < 9;  // (wave-uniform)
                const float *gp = gs + l31 * C3_GP + half;
#pragma unroll 4
                for (int p = 0; p < C3_WPIX; p += 2) {
                    const int q = p + half, py = q / C3_WTW, px = q - py * C3_WTW, po = py * C3_WPW + px;
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
    const size_t M = (size_t)C3_CO * 9 * C + C3_CO;
    float *out = partial + (size_t)blockIdx.x * M;
#pragma unroll
    for (int cc = 0; cc < 2; cc++) {
        const int ci = cc * 32 + l31, tap0 = (wave + 3 * cc) & 3;
#pragma unroll
        for (int s = 0; s < 3; s++) {
            const int tap = tap0 + 4 * s;
            if (tap < 9 && ci < C) {
#pragma unroll
                for (int v = 0; v < 16; v++) {
                    const int co = (v >> 2) * 8 + half * 4 + (v & 3);
                    out[((size_t)co * C + ci) * 9 + tap] = acc[cc][s][v];
                }
            }
        }
    }
    if ((tid & 7) == 0) out[(size_t)C3_CO * 9 * C + (tid >> 3)] = dbsum;
}

bool supported(int C_in, int C_out) { return C_out == C3_CO && C_in >= 4 && C_in <= 64 && C_in % 4 == 0; }

// fills d; false = refused (unsupported channel counts, a non-positive size, 2^31 elements or more in x or y)
bool make_dims(int N, int C_in, int H, int W, C3Dims &d) {
    if (!supported(C_in, C3_CO) || N <= 0 || H <= 0 || W <= 0) return false;
    const size_t lim = (size_t)1 << 31;
    const size_t plane = (size_t)H * W;  // < 2^62
    if (plane >= lim || (size_t)N * plane >= lim) return false;  // N * plane < 2^62
    const size_t np = (size_t)N * plane;                          // < 2^31: times 64 channels at most cannot overflow
    if (np * C_in >= lim || np * C3_CO >= lim) return false;
    d.N = N; d.C = C_in; d.H = H; d.W = W;
    d.tiles_y = (int)cdiv(H, C3_TH);
    d.tiles_x = (int)cdiv(W, C3_TW);
    return true;
}

size_t weight_tiles(const C3Dims &d) { return (size_t)d.N * cdiv(d.H, C3_WTH) * cdiv(d.W, C3_WTW); }
size_t weight_parts(const C3Dims &d) { const size_t t = weight_tiles(d); return t < (size_t)C3_PARTS ? t : (size_t)C3_PARTS; }

}  // namespace

extern "C" int c3_supported(int C_in, int C_out) { return supported(C_in, C_out) ? 1 : 0; }

extern "C" int c3_tile(int *tile_h, int *tile_w) {
    if (!tile_h || !tile_w) return GPSGS_E_INVALID;
    *tile_h = C3_TH;
    *tile_w = C3_TW;
    return GPSGS_OK;
}

extern "C" size_t c3_scratch_bytes(int N, int C_in, int H, int W) {
    C3Dims d;
    if (!make_dims(N, C_in, H, W, d)) return 0;
    const size_t parts = weight_parts(d), M = (size_t)C3_CO * (9 * (size_t)C_in + 1);
    return partials_scratch_bytes(parts, C3_GROUP, M);
}

extern "C" int c3_forward(const float *x, const float *w, const float *bias, int N, int C_in, int H, int W, int relu, float *y, void *stream) {
    C3Dims d;
    if (!make_dims(N, C_in, H, W, d)) return GPSGS_E_INVALID;
    if (relu != 0 && relu != 1) return GPSGS_E_INVALID;
    if (!x || !w || !bias || !y) return GPSGS_E_INVALID;
    if (!aligned(x, 16) || !aligned(y, 16) || !aligned(w, 4) || !aligned(bias, 4)) return GPSGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((size_t)d.N * d.tiles_y * d.tiles_x)), block(C3_THREADS);
    if (relu)
        hipLaunchKernelGGL(k_c3_fwd<true>, grid, block, 0, s, x, w, bias, y, d);
    else
        hipLaunchKernelGGL(k_c3_fwd<false>, grid, block, 0, s, x, w, bias, y, d);
    return launched();
}

extern "C" int c3_backward(const float *x, const float *w, const float *y, const float *dy, int N, int C_in, int H, int W, int relu, float *dx,
                           float *dw, float *dbias, void *scratch, void *stream) {
    C3Dims d;
    if (!make_dims(N, C_in, H, W, d)) return GPSGS_E_INVALID;
    if (relu != 0 && relu != 1) return GPSGS_E_INVALID;
    if ((dw != nullptr) != (dbias != nullptr)) return GPSGS_E_INVALID;
    if (!x || !w || !dy || (relu && !y) || (dw && !scratch)) return GPSGS_E_INVALID;
    if (!aligned(x, 16) || !aligned(y, 16) || !aligned(dy, 16) || !aligned(dx, 16) || !aligned(w, 4) || !aligned(dw, 4) || !aligned(dbias, 4) ||
        !aligned(scratch, 16))
        return GPSGS_E_INVALID;
    if (!dx && !dw) return GPSGS_OK;
    hipStream_t s = (hipStream_t)stream;
    if (dx) {
        const dim3 grid((unsigned)((size_t)d.N * d.tiles_y * d.tiles_x), (unsigned)cdiv(C_in, 32)), block(C3_THREADS);
        if (relu)
            hipLaunchKernelGGL(k_c3_bwd_input<true>, grid, block, 0, s, dy, y, w, dx, d);
        else
            hipLaunchKernelGGL(k_c3_bwd_input<false>, grid, block, 0, s, dy, y, w, dx, d);
    }
    if (dw) {
        const int tiles = (int)weight_tiles(d), parts = (int)weight_parts(d), wtx = (int)cdiv(d.W, C3_WTW), wty = (int)cdiv(d.H, C3_WTH);
        const int MW = C3_CO * 9 * C_in, M = MW + C3_CO;
        float *part = (float *)scratch;
        if (relu)
            hipLaunchKernelGGL(k_c3_bwd_weight<true>, dim3(parts), dim3(C3_THREADS), 0, s, x, dy, y, part, d, wtx, wty, tiles);
        else
            hipLaunchKernelGGL(k_c3_bwd_weight<false>, dim3(parts), dim3(C3_THREADS), 0, s, x, dy, y, part, d, wtx, wty, tiles);
        sum_partials(part, parts, C3_GROUP, M, MW, dw, dbias, s);
    }
    return launched();
}
