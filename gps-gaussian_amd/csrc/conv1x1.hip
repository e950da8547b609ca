// conv1x1.hip -- 1x1 convolution, stride 1 or 2, padding 0, with a bias, on the fp32 matrix cores of gfx950, forward and backward
// (DESIGN.md "Residual-shortcut 1x1 convolutions").
//
// The shortcut of every ResidualBlock whose input and output differ opens with Conv2d(in, planes, 1, stride) (core/extractor.py:43-45), in fp32
// wherever the block runs outside autocast.  Over contiguous NCHW that is one GEMM per image, Y[C_out x P] = W[C_out x C_in] X[C_in x P], with
// the pixel axis contiguous in X and in Y: no im2col, no layout change, no halo.  Here it runs on v_mfma_f32_32x32x2_f32 -- exact fp32, bit for
// bit an fmaf chain.  C_in a multiple of 4 in [4, 256], C_out a multiple of 16 in [16, 128], stride 1 or 2.
//
//   k_c1_fwd         one 256-thread workgroup per C1_TP = 256 consecutive output pixels of one image: M = the output channels (up to four blocks
//                    of 32, all in one wave's accumulators), N = pixels, K = C_in.  A wave owns 64 pixels = two 32-pixel columns of blocks.  The
//                    pixel operand never touches LDS: lane l of the MFMA's B operand is (channel k + l / 32, pixel l % 32), so a wave's operand
//                    IS one coalesced global load of 32 consecutive pixels of two channels (stride 2: every other element of the even rows).
//                    K is walked in chunks of 16 channels; the next chunk's 16 loads per lane are in flight while the matrix cores work on this
//                    one.  Only the weights go through LDS (a [16][C_out] slice per chunk, transposed on the way in, swizzled so that neither the
//                    write nor the read collides).  Epilogue: + bias, one store per element, lanes on consecutive pixels.
//   k_c1_bwd_input   the same engine with the roles swapped: dx = W^T dy, M = C_in (grid y over groups of up to four blocks of 32), K = C_out.
//                    It writes ALL of dx: for stride 2 a lane writes the 2 x 2 quad of its pixel, +0.0 at the three positions the forward never
//                    sampled (clipped to the plane), so no memset runs in front.
//   k_c1_bwd_weight  dw[co][ci] = sum over pixels dy[co] x[ci]: M = co, N = ci, K = pixels.  A workgroup walks the 32-pixel tiles b, b + G, ... in
//                    index order with its share of the up to 4 x 8 blocks of 32 x 32 sums in accumulators (block b of the list on wave b % 4),
//                    dy [C_out][32] and x [C_in][32] in LDS; it writes ONE partial (and its bias sums) to scratch.
//   k_sum_partials   (op_reduce.h) adds the workgroups' partials in index order, in groups of C1_GROUP and then the groups.
// No atomics; every sum has a fixed order: the same bits on every run.  Guarded global loads are an unconditional load from a clamped (always
// valid) address followed by a select (stem_conv.hip).  Accumulator layout of the MFMA as in conv3x3.hip: register v of lane l is row
// (v / 4) * 8 + (l / 32) * 4 + v % 4, column l % 32; the A operand of lane l is A[l % 32][l / 32], the B operand B[l / 32][l % 32].
#include <type_traits>

#include "op_reduce.h"

namespace {

typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int C1_THREADS = 256;
constexpr int C1_TP = 256;                 // pixels per workgroup of the forward and of the input gradient: 4 waves x 2 columns of 32
constexpr int C1_CK = 16;                  // reduction channels per step
constexpr int C1_MB = 4;                   // blocks of 32 output channels a wave holds at most
constexpr int C1_WPITCH = 160;             // pitch of a staged weight row: >= 128 and 32 banks past a multiple of 64 (rows k, k + 1 never collide)
static_assert(C1_WPITCH >= C1_MB * 32 && C1_WPITCH % 64 == 32, "weight pitch");

constexpr int C1_WP = 32;                  // pixel tile of the weight gradient
constexpr int C1_GP = C1_WP + 2;           // pitch of its LDS rows: 2 * odd -- 32 channels (lanes) x 2 neighbouring pixels (lane halves) hit 64 banks
constexpr int C1_MAXCO = 128, C1_MAXCI = 256;
constexpr int C1_WSLOTS = (C1_MAXCO / 32) * (C1_MAXCI / 32) / 4;  // 32 x 32 blocks of dw per wave at most: 8
constexpr int C1_PARTS = 512;              // partials of the weight gradient at most (workgroups of k_c1_bwd_weight)
constexpr int C1_GROUP = 32;               // partials per first-stage group of the reduction
static_assert((C1_GP / 2) % 2 == 1, "weight-gradient LDS pitch");

struct C1Dims {
    int N, Ci, Co, H, W, Ho, Wo, stride;
};

// where element (k, m) of a staged weight slice lies: the xor moves m inside its block of 32, so a row still fills 32 consecutive banks for the
// MFMA's read (lanes on m), and the forward's transposing write (lanes on 16 k x 4 m) hits 64 different banks
__device__ __forceinline__ int c1_widx(int k, int m) { return k * C1_WPITCH + (m ^ ((k >> 1) << 2)); }

// 256 pixels of out[n, m0 .. m0 + 32 NB) = sum over k of W(m, k) in[n, k], m0 = 32 NB blockIdx.y: forward K = C_in, M = C_out, W(m, k) = w[m][k],
// `in` sampled with the stride, `out` dense; BWD K = C_out, M = C_in, W(m, k) = w[k][m], `in` dense, `out` scattered with the stride and the gaps
// zeroed.  Nothing is selected between a global load and its use (a select would wait for the load where it stands): a pixel past the plane reads
// pixel 0 and its column of sums is never stored -- the columns of a GEMM do not mix -- and a channel pair past K is zeros on both sides.
template <bool BWD, int NB>
__device__ __forceinline__ void c1_engine(const float *__restrict__ in, const float *__restrict__ w, const float *__restrict__ bias,
                                          float *__restrict__ out, const C1Dims &d, int tiles, float *ws) {
    constexpr int KP = C1_CK / 2;                                   // k pairs per chunk
    constexpr int MW = NB * 32;                                     // staged weight columns
    constexpr int WI = C1_CK * MW / C1_THREADS;                     // staged weights per thread: 2 NB
    const int K = BWD ? d.Co : d.Ci, M = BWD ? d.Ci : d.Co;
    const int m0 = (int)blockIdx.y * MW;
    const unsigned b = blockIdx.x;
    const int tile = (int)(b % (unsigned)tiles);
    const size_t n = b / (unsigned)tiles;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int P = d.Ho * d.Wo;
    const size_t HW = (size_t)d.H * d.W;
    const size_t inplane = BWD ? (size_t)P : HW, outplane = BWD ? HW : (size_t)P;
    const float *inn = in + n * K * inplane;

    int p[2], so[2];  // the lane's pixel in each of its two columns, and where the strided side keeps it
    bool ok[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
        p[t] = tile * C1_TP + wave * 64 + t * 32 + l31;
        ok[t] = p[t] < P;
        if (!ok[t]) p[t] = 0;
        const int i = p[t] / d.Wo, j = p[t] - i * d.Wo;
        so[t] = d.stride == 1 ? p[t] : (i * d.W + j) * 2;
    }
    // the lane's two operand elements of a pair of channels (kk, kk + 1), as 32-bit offsets from the uniform address of channel kk's plane: at least
    // four channels and fewer than 2^31 elements in a tensor keep a plane under 2^29 elements, so plane + offset fits
    const unsigned v0 = (unsigned)(half * inplane) + (unsigned)(BWD ? p[0] : so[0]), v1 = (unsigned)(half * inplane) + (unsigned)(BWD ? p[1] : so[1]);

    float wv[WI];
    auto wpos = [&](int i, int &k, int &m) {  // the element of a [16][MW] slice that this thread stages i-th: the global reads run along w's rows
        const int e = tid + i * C1_THREADS;
        if (BWD) { k = e / MW; m = e - k * MW; } else { k = e & 15; m = e >> 4; }
    };
    auto wgood = [&](int c0, int k, int m) { return c0 + k < K && m0 + m < M; };
    auto loadw = [&](int c0) {
#pragma unroll
        for (int i = 0; i < WI; i++) {
            int k, m;
            wpos(i, k, m);
            const size_t src = BWD ? (size_t)(c0 + k) * M + m0 + m : (size_t)(m0 + m) * K + c0 + k;
            wv[i] = w[wgood(c0, k, m) ? src : 0];
        }
    };
    auto storew = [&](int c0) {  // (the zero of an element past K or M is chosen here, where the value is needed)
#pragma unroll
        for (int i = 0; i < WI; i++) {
            int k, m;
            wpos(i, k, m);
            ws[c1_widx(k, m)] = wgood(c0, k, m) ? wv[i] : 0.f;
        }
    };
    float xc[KP][2];  // the chunk's pixel operand; pair kp is reloaded for the next chunk as soon as its MFMAs have been issued
    auto loadx = [&](int c0, int kp, bool guard) {
        const int kk = c0 + 2 * kp;  // (uniform; K is a multiple of 4: whole pairs)
        if (!guard || kk < K) {
            const float *src = inn + (size_t)kk * inplane;
            xc[kp][0] = src[v0];
            xc[kp][1] = src[v1];
        } else {  // a pair past K: zeros against the zero weights staged for it, so the chunk's MFMAs need no condition
            xc[kp][0] = 0.f;
            xc[kp][1] = 0.f;
        }
    };

    v16f acc[NB][2];
#pragma unroll
    for (int mb = 0; mb < NB; mb++)
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int v = 0; v < 16; v++) acc[mb][t][v] = 0.f;

    // one chunk of 16 channels from c0.  NEXT 1: a whole chunk follows; its weights and its 16 pixel loads per lane are issued here, in flight while
    // the matrix cores work.  NEXT 2: the chunk that follows is the last and ends before its 16th channel.  NEXT 0: nothing follows.
    auto chunk = [&](int c0, auto next_) {
        constexpr int NEXT = decltype(next_)::value;
        __syncthreads();  // every wave is done reading the previous slice
        storew(c0);
        __syncthreads();
        if (NEXT) loadw(c0 + C1_CK);
        float a[NB], an[NB];
#pragma unroll
        for (int mb = 0; mb < NB; mb++) a[mb] = ws[c1_widx(half, mb * 32 + l31)];
#pragma unroll
        for (int kp = 0; kp < KP; kp++) {
            if (kp + 1 < KP) {
#pragma unroll
                for (int mb = 0; mb < NB; mb++) an[mb] = ws[c1_widx(2 * kp + 2 + half, mb * 32 + l31)];
            }
#pragma unroll
            for (int mb = 0; mb < NB; mb++) {
                acc[mb][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mb], xc[kp][0], acc[mb][0], 0, 0, 0);
                acc[mb][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mb], xc[kp][1], acc[mb][1], 0, 0, 0);
            }
            if (NEXT) loadx(c0 + C1_CK, kp, NEXT == 2);
#pragma unroll
            for (int mb = 0; mb < NB; mb++) a[mb] = an[mb];
        }
    };
    loadw(0);
#pragma unroll
    for (int kp = 0; kp < KP; kp++) loadx(0, kp, true);
    int c0 = 0;
#pragma unroll 1
    for (; c0 + 2 * C1_CK <= K; c0 += C1_CK) chunk(c0, std::integral_constant<int, 1>());
    if (c0 + C1_CK < K) {
        chunk(c0, std::integral_constant<int, 2>());
        c0 += C1_CK;
    }
    chunk(c0, std::integral_constant<int, 0>());

    float *outn = out + n * M * outplane;
    const bool pairs = BWD && d.stride == 2 && (d.W & 1) == 0;  // every quad is whole in x and starts on an even element: 8-byte stores
#pragma unroll
    for (int t = 0; t < 2; t++) {
        if (!ok[t]) continue;
        const int i = p[t] / d.Wo, j = p[t] - i * d.Wo;
        const bool row1 = 2 * i + 1 < d.H, col1 = 2 * j + 1 < d.W;
#pragma unroll
        for (int mb = 0; mb < NB; mb++) {
#pragma unroll
            for (int v = 0; v < 16; v++) {
                const int m = m0 + mb * 32 + (v >> 2) * 8 + half * 4 + (v & 3);
                if (m < M) {
                    const float val = acc[mb][t][v];
                    if (!BWD) {
                        outn[(size_t)m * outplane + p[t]] = val + bias[m];
                    } else if (d.stride == 1) {
                        outn[(size_t)m * outplane + p[t]] = val;
                    } else {
                        float *o = outn + (size_t)m * outplane + so[t];
                        if (pairs) {
                            *reinterpret_cast<float2 *>(o) = make_float2(val, 0.f);
                            if (row1) *reinterpret_cast<float2 *>(o + d.W) = make_float2(0.f, 0.f);
                        } else {
                            o[0] = val;
                            if (col1) o[1] = 0.f;
                            if (row1) {
                                o[d.W] = 0.f;
                                if (col1) o[d.W + 1] = 0.f;
                            }
                        }
                    }
                }
            }
        }
    }
}

// NB = the blocks of 32 output channels a wave holds: 32 NB accumulator registers, so the narrower layers run at a higher occupancy
// (launch bounds: NB = 4 is 128 accumulator registers + the pixel operand + the staged weights + addresses: under 256, two waves per SIMD; the
// allocator spends what the bound leaves it, so the bound is what sets the occupancy: four, three, two, two workgroups per CU)
constexpr int c1_wgs(int NB) { return NB == 1 ? 4 : NB == 2 ? 3 : 2; }

template <int NB>
__global__ __launch_bounds__(C1_THREADS, c1_wgs(NB)) void k_c1_fwd(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias,
                                                          float *__restrict__ y, C1Dims d, int tiles) {
    __shared__ float ws[C1_CK * C1_WPITCH];
    c1_engine<false, NB>(x, w, bias, y, d, tiles, ws);
}

template <int NB>
__global__ __launch_bounds__(C1_THREADS, c1_wgs(NB)) void k_c1_bwd_input(const float *__restrict__ dy, const float *__restrict__ w, float *__restrict__ dx,
                                                                C1Dims d, int tiles) {
    __shared__ float ws[C1_CK * C1_WPITCH];
    c1_engine<true, NB>(dy, w, nullptr, dx, d, tiles, ws);
}

// f(std::integral_constant<int, nb>()) for nb in [1, C1_MB]: the run-time block count as a compile-time one
template <class F> inline void with_blocks(int nb, F f) {
    switch (nb) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    default: f(std::integral_constant<int, 4>()); break;
    }
}

// partial[b][co * C_in + ci], then partial[b][C_out * C_in + co] = the workgroup's sum of dy[co]
// (51 KB of LDS: three workgroups per CU; 128 accumulator registers: two waves per SIMD)
__global__ __launch_bounds__(C1_THREADS, 2) void k_c1_bwd_weight(const float *__restrict__ x, const float *__restrict__ dy, float *__restrict__ partial,
                                                                 C1Dims d, int wtiles, int tiles) {
    __shared__ float gs[C1_MAXCO * C1_GP];
    __shared__ float xs[C1_MAXCI * C1_GP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int Ci = d.Ci, Co = d.Co, P = d.Ho * d.Wo;
    const size_t HW = (size_t)d.H * d.W;
    const int NBk = (Ci + 31) >> 5, B = ((Co + 31) >> 5) * NBk;  // the blocks of dw: b = (block of co) * NBk + block of ci
    v16f acc[C1_WSLOTS];                                           // slot s: block 4 s + wave
#pragma unroll
    for (int s = 0; s < C1_WSLOTS; s++)
#pragma unroll
        for (int v = 0; v < 16; v++) acc[s][v] = 0.f;
    float dbsum = 0.f;
    // rows past C_out / C_in of a half-used block are read by the MFMAs and never staged: zeros
    for (int e = tid; e < C1_MAXCO * C1_GP; e += C1_THREADS) gs[e] = 0.f;
    for (int e = tid; e < C1_MAXCI * C1_GP; e += C1_THREADS) xs[e] = 0.f;
    const int px = tid & 31, total = (Co + Ci) * C1_WP;
#pragma unroll 1
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const size_t n = (size_t)(t / wtiles);
        const int q = (t % wtiles) * C1_WP + px;  // this thread's pixel in every element it stages (256 is a multiple of 32)
        const bool ok = q < P;
        const int pq = ok ? q : 0, i = pq / d.Wo, j = pq - i * d.Wo;
        const int sq = d.stride == 1 ? pq : (i * d.W + j) * 2;
        const float *gn = dy + n * Co * (size_t)P + pq, *xn = x + n * Ci * HW + sq;
        __syncthreads();  // the previous tile has been read
        constexpr int BATCH = 8;
#pragma unroll 1
        for (int e0 = 0; e0 < total; e0 += BATCH * C1_THREADS) {
            float v[BATCH];
#pragma unroll
            for (int k = 0; k < BATCH; k++) {
                const int e = e0 + k * C1_THREADS + tid, ch = e >> 5;
                const bool in = e < total;
                const float *src = !in ? gn : ch < Co ? gn + (size_t)ch * P : xn + (size_t)(ch - Co) * HW;
                const float tv = *src;
                v[k] = in && ok ? tv : 0.f;
            }
#pragma unroll
            for (int k = 0; k < BATCH; k++) {
                const int e = e0 + k * C1_THREADS + tid, ch = e >> 5;
                if (e < total) {
                    if (ch < Co) gs[ch * C1_GP + px] = v[k]; else xs[(ch - Co) * C1_GP + px] = v[k];
                }
            }
        }
        __syncthreads();
        {  // the bias gradient: 2 lanes per channel, each 16 pixels in index order, then the pair
            const int co = tid >> 1, part = tid & 1;
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < C1_WP / 2; k++) s += gs[co * C1_GP + part * (C1_WP / 2) + k];
            s += __shfl_xor(s, 1, 64);
            dbsum += s;
        }
#pragma unroll
        for (int s = 0; s < C1_WSLOTS; s++) {
            const int blk = 4 * s + wave;
            if (blk < B) {  // (wave-uniform)
                const int mb = blk / NBk, nbk = blk - mb * NBk;
                const float *gp = gs + (mb * 32 + l31) * C1_GP + half, *xp = xs + (nbk * 32 + l31) * C1_GP + half;
#pragma unroll 4
                for (int k = 0; k < C1_WP; k += 2) acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(gp[k], xp[k], acc[s], 0, 0, 0);
            }
        }
    }
    const size_t MW = (size_t)Co * Ci;
    float *out = partial + (size_t)blockIdx.x * (MW + Co);
#pragma unroll
    for (int s = 0; s < C1_WSLOTS; s++) {
        const int blk = 4 * s + wave;
        if (blk < B) {
            const int mb = blk / NBk, nbk = blk - mb * NBk, ci = nbk * 32 + l31;
#pragma unroll
            for (int v = 0; v < 16; v++) {
                const int co = mb * 32 + (v >> 2) * 8 + half * 4 + (v & 3);
                if (co < Co && ci < Ci) out[(size_t)co * Ci + ci] = acc[s][v];
            }
        }
    }
    if ((tid & 1) == 0 && (tid >> 1) < Co) out[MW + (tid >> 1)] = dbsum;
}

bool supported(int C_in, int C_out, int stride) {
    return C_in >= 4 && C_in <= C1_MAXCI && C_in % 4 == 0 && C_out >= 16 && C_out <= C1_MAXCO && C_out % 16 == 0 && (stride == 1 || stride == 2);
}

// fills d; false = refused (an unsupported configuration, a non-positive size, 2^31 elements or more in x or y)
bool make_dims(int N, int C_in, int C_out, int H, int W, int stride, C1Dims &d) {
    if (!supported(C_in, C_out, stride) || N <= 0 || H <= 0 || W <= 0) return false;
    const size_t lim = (size_t)1 << 31;
    const size_t plane = (size_t)H * W;  // < 2^62
    if (plane >= lim || (size_t)N * plane >= lim) return false;  // N * plane < 2^62
    if ((size_t)N * plane * C_in >= lim) return false;           // < 2^31 * 256
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    if ((size_t)N * Ho * Wo * C_out >= lim) return false;        // N * Ho * Wo <= N * plane < 2^31, times 128 at most
    d.N = N; d.Ci = C_in; d.Co = C_out; d.H = H; d.W = W; d.Ho = Ho; d.Wo = Wo; d.stride = stride;
    return true;
}

size_t pixel_tiles(const C1Dims &d) { return cdiv((size_t)d.Ho * d.Wo, C1_TP); }
size_t weight_tiles(const C1Dims &d) { return (size_t)d.N * cdiv((size_t)d.Ho * d.Wo, C1_WP); }
size_t weight_parts(const C1Dims &d) { const size_t t = weight_tiles(d); return t < (size_t)C1_PARTS ? t : (size_t)C1_PARTS; }

}  // namespace

extern "C" int c1_supported(int C_in, int C_out, int stride) { return supported(C_in, C_out, stride) ? 1 : 0; }

extern "C" int c1_tile(int *forward_pixels, int *weight_pixels, int *max_parts) {
    if (!forward_pixels || !weight_pixels || !max_parts) return GPSGS_E_INVALID;
    *forward_pixels = C1_TP;
    *weight_pixels = C1_WP;
    *max_parts = C1_PARTS;
    return GPSGS_OK;
}

extern "C" size_t c1_scratch_bytes(int N, int C_in, int C_out, int H, int W, int stride) {
    C1Dims d;
    if (!make_dims(N, C_in, C_out, H, W, stride, d)) return 0;
    return partials_scratch_bytes(weight_parts(d), C1_GROUP, (size_t)C_out * ((size_t)C_in + 1));
}

extern "C" int c1_forward(const float *x, const float *w, const float *bias, int N, int C_in, int C_out, int H, int W, int stride, float *y,
                          void *stream) {
    C1Dims d;
    if (!make_dims(N, C_in, C_out, H, W, stride, d)) return GPSGS_E_INVALID;
    if (!x || !w || !bias || !y) return GPSGS_E_INVALID;
    if (!aligned(x, 16) || !aligned(y, 16) || !aligned(w, 4) || !aligned(bias, 4)) return GPSGS_E_INVALID;
    const int tiles = (int)pixel_tiles(d);
    with_blocks((int)cdiv(C_out, 32), [&](auto nb) {  // C_out <= 128: one group of blocks
        hipLaunchKernelGGL(k_c1_fwd<decltype(nb)::value>, dim3((unsigned)((size_t)d.N * tiles)), dim3(C1_THREADS), 0, (hipStream_t)stream, x, w, bias, y,
                           d, tiles);
    });
    return launched();
}

extern "C" int c1_backward(const float *x, const float *w, const float *dy, int N, int C_in, int C_out, int H, int W, int stride, float *dx,
                           float *dw, float *dbias, void *scratch, void *stream) {
    C1Dims d;
    if (!make_dims(N, C_in, C_out, H, W, stride, d)) return GPSGS_E_INVALID;
    if ((dw != nullptr) != (dbias != nullptr)) return GPSGS_E_INVALID;
    if (!x || !w || !dy || (dw && !scratch)) return GPSGS_E_INVALID;
    if (!aligned(x, 16) || !aligned(dy, 16) || !aligned(dx, 16) || !aligned(w, 4) || !aligned(dw, 4) || !aligned(dbias, 4) || !aligned(scratch, 16))
        return GPSGS_E_INVALID;
    if (!dx && !dw) return GPSGS_OK;
    hipStream_t s = (hipStream_t)stream;
    if (dx) {
        // the blocks of 32 input channels in as few equal groups of at most C1_MB as there can be: 6 -> 3 + 3, 8 -> 4 + 4
        const int tiles = (int)pixel_tiles(d), blocks = (int)cdiv(C_in, 32), groups = (int)cdiv(blocks, C1_MB), nbg = (int)cdiv(blocks, groups);
        with_blocks(nbg, [&](auto nb) {
            hipLaunchKernelGGL(k_c1_bwd_input<decltype(nb)::value>, dim3((unsigned)((size_t)d.N * tiles), (unsigned)cdiv(blocks, nbg)), dim3(C1_THREADS),
                               0, s, dy, w, dx, d, tiles);
        });
    }
    if (dw) {
        const int tiles = (int)weight_tiles(d), parts = (int)weight_parts(d), wtiles = tiles / d.N;
        const int MW = C_out * C_in, M = MW + C_out;
        float *part = (float *)scratch;
        hipLaunchKernelGGL(k_c1_bwd_weight, dim3(parts), dim3(C1_THREADS), 0, s, x, dy, part, d, wtiles, tiles);
        sum_partials(part, parts, C1_GROUP, M, MW, dw, dbias, s);
    }
    return launched();
}
