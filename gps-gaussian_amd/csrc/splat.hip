// splat.hip -- z-buffer point splat of the stage-1 validation render.
//
// Replaces lib/TaichiRender.py:13-24 (render_respective_color) and, fused, lib/TaichiRender.py:26-60 (flow2render: flow2depth, depth2pc,
// perspective into the novel view, 1 / (z + 1e-8), then one splat per source view).  Result per target pixel: the one of running the points in
// sequence -- view 0's points in index order, then view 1's -- with `if z >= depth[px]: depth[px] = z; colour[px] = rgb`, i.e. the point with the
// largest (z, order) among those reaching the pixel and the pixel's initial value (a tie in z goes to the later point; any point beats the
// initial value).  oracle/aux_oracle.c::zsplat_oracle states the same sequentially.
//
// One 64-bit key per pixel, orderable_bits(z) << 32 | tag, tag = 1 + view * N + i (0 = "what the buffer held before the call"):
//   init     key from the current depth, tag 0
//   scatter  one lane per source point, no-return 64-bit atomic max (global_atomic_umax_x2); max is order-independent, so every view and
//            every sample go into ONE launch
//   resolve  one lane per target pixel: tag 0 leaves the pixel alone, otherwise the winner's z and colour are gathered
// Deterministic: the reference's atomic_max on the depth followed by a separate, non-atomic colour write can keep the colour of the farther of two
// points landing on a pixel at the same time; here the colour always belongs to the key that won.
#include "op_common.h"
#include "unproject_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int NOVEL_FLOATS = 21;  // novel view: intr 3x3 | extr rows 0..2 (3x4, row-major)

// monotone float -> uint map (-0 canonicalised to +0; callers drop NaN points)
__device__ __forceinline__ uint32_t orderable_bits(float z) {
    const uint32_t b = __float_as_uint(z == 0.0f ? 0.0f : z);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// a NaN initial depth: `z >= NaN` is false for every point, so nothing may beat it
__device__ __forceinline__ uint64_t init_key(float d) { return (uint64_t)(d != d ? 0xffffffffu : orderable_bits(d)) << 32; }

// clamp(trunc(v), 0, res - 1) with v_cvt_i32_f32 semantics (saturating, NaN -> 0): fmaxf(NaN, 0) = 0
__device__ __forceinline__ int pixel_index(float v, int res) { return (int)fminf(fmaxf(truncf(v), 0.0f), (float)(res - 1)); }

__device__ __forceinline__ void scatter_key(uint64_t *__restrict__ keys, int b, int res, float x, float y, float z, uint32_t tag) {
    if (z != z) return;  // NaN: `NaN >= d` is false in the sequential form
    const int ix = pixel_index(x, res), iy = pixel_index(y, res);
    const uint64_t key = (uint64_t)orderable_bits(z) << 32 | tag;
    __hip_atomic_fetch_max(keys + ((size_t)b * res + iy) * res + ix, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(TPB) void k_zsplat_init(const float *__restrict__ depth, uint64_t *__restrict__ keys, int R2) {
    const int pix = blockIdx.x * TPB + threadIdx.x;
    const size_t p = (size_t)blockIdx.y * R2 + pix;
    if (pix < R2) keys[p] = init_key(depth[p]);
}

// pts [V][B][N][6] = (x, y, z, r, g, b); mask [V][B][N]
__global__ __launch_bounds__(TPB) void k_zsplat_scatter(const float *__restrict__ pts, const float *__restrict__ mask, int B, int N, int res,
                                                        uint64_t *__restrict__ keys) {
    const int i = blockIdx.x * TPB + threadIdx.x, b = blockIdx.y, v = blockIdx.z;
    if (i >= N) return;
    const size_t p = ((size_t)v * B + b) * N + i;
    if (mask[p] < 0.5f) return;
    const float *q = pts + p * 6;
    scatter_key(keys, b, res, q[0], q[1], q[2], 1u + (uint32_t)v * (uint32_t)N + (uint32_t)i);
}

__global__ __launch_bounds__(TPB) void k_zsplat_resolve(const uint64_t *__restrict__ keys, const float *__restrict__ pts, int B, int N, int res,
                                                        float *__restrict__ depth, float *__restrict__ color) {
    const int pix = blockIdx.x * TPB + threadIdx.x, b = blockIdx.y, R2 = res * res;
    if (pix >= R2) return;
    const uint32_t tag = (uint32_t)keys[(size_t)b * R2 + pix];
    if (tag == 0) return;
    const uint32_t v = (tag - 1) / (uint32_t)N, i = (tag - 1) - v * (uint32_t)N;
    const float *q = pts + (((size_t)v * B + b) * N + i) * 6;
    depth[(size_t)b * R2 + pix] = q[2];  // the winner's own bits (-0 stays -0, as in the sequential form)
#pragma unroll
    for (int k = 0; k < 3; k++) color[((size_t)b * 3 + k) * R2 + pix] = q[3 + k];
}

// ---- flow2render: two source views (0 = lmain, 1 = rmain) of S x S pixels into a res x res novel view -------------------------------------
struct F2RViews {
    const float *flow[2], *mask[2], *img[2];
};

__global__ __launch_bounds__(TPB) void k_f2r_init(uint64_t *__restrict__ keys, int R2) {
    const int pix = blockIdx.x * TPB + threadIdx.x;
    if (pix < R2) keys[(size_t)blockIdx.y * R2 + pix] = init_key(0.0f);  // render_depth = zeros
}

__global__ __launch_bounds__(TPB) void k_f2r_scatter(F2RViews a, int B, int S, int res, int64_t mask_bstride, const float *__restrict__ cams_dev,
                                                     const float *__restrict__ novel_dev, float *__restrict__ pts_out, uint64_t *__restrict__ keys) {
    const int S2 = S * S, pix = blockIdx.x * TPB + threadIdx.x, b = blockIdx.y, view = blockIdx.z;
    if (pix >= S2) return;
    const UnprojCam c = cam_from_device(cams_dev, view * B + b);
    const int v = pix / S, u = pix - v * S;
    const float d = up_inverse_depth(c, a.flow[view][(size_t)b * S2 + pix], a.mask[view][(size_t)b * mask_bstride + pix]);
    float *o = pts_out ? pts_out + (((size_t)view * B + b) * S2 + pix) * 3 : nullptr;
    if (!(d != 0.0f)) {  // valid = depth != 0 (lib/TaichiRender.py:37); invalid points are masked out of the splat
        if (o) o[0] = o[1] = o[2] = __builtin_nanf("");
        return;
    }
    float w[3];
    up_world_point(c, u, v, d, w);
    // perspective (lib/utils.py:122-128) with calib = intr @ extr (lib/TaichiRender.py:27), both products in index order
    const float *K = novel_dev + (size_t)b * NOVEL_FLOATS, *E = K + 9;
    float q[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        float C[4];
#pragma unroll
        for (int j = 0; j < 4; j++) C[j] = K[i * 3] * E[j] + K[i * 3 + 1] * E[4 + j] + K[i * 3 + 2] * E[8 + j];
        q[i] = (C[0] * w[0] + C[1] * w[1] + C[2] * w[2]) + C[3];
    }
    const float x = q[0] / q[2], y = q[1] / q[2], z = 1.0f / (q[2] + 1e-8f);
    if (o) { o[0] = x; o[1] = y; o[2] = z; }
    scatter_key(keys, b, res, x, y, z, 1u + (uint32_t)view * (uint32_t)S2 + (uint32_t)pix);
}

__global__ __launch_bounds__(TPB) void k_f2r_resolve(F2RViews a, const uint64_t *__restrict__ keys, int S, int res, float *__restrict__ img_pred) {
    const int pix = blockIdx.x * TPB + threadIdx.x, b = blockIdx.y, R2 = res * res, S2 = S * S;
    if (pix >= R2) return;
    const uint32_t tag = (uint32_t)keys[(size_t)b * R2 + pix];
    float rgb[3] = {-1.0f, -1.0f, -1.0f};  // render_color = -1 + zeros
    if (tag != 0) {
        const uint32_t view = (tag - 1) >= (uint32_t)S2, i = (tag - 1) - view * (uint32_t)S2;
        const float *img = a.img[view] + (size_t)b * 3 * S2 + i;
#pragma unroll
        for (int k = 0; k < 3; k++) rgb[k] = img[(size_t)k * S2];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) img_pred[((size_t)b * 3 + k) * R2 + pix] = rgb[k];
}

}  // namespace

extern "C" size_t up_splat_scratch_bytes(int B, int res) {
    if (B < 0 || res < 0) return 0;
    return (size_t)B * res * res * sizeof(uint64_t);
}

extern "C" int up_zsplat(int V, int B, int N, int res, const float *pts, const float *mask, float *depth, float *color, void *scratch,
                         size_t scratch_bytes, void *stream) {
    if (V < 0 || B < 0 || N < 0 || res < 0) return GPSGS_E_INVALID;
    if (V == 0 || B == 0 || N == 0) return GPSGS_OK;
    if (res == 0 || res > 32768 || B > 65535 || V > 65535 || (uint64_t)V * N + 1 > 0xffffffffull) return GPSGS_E_INVALID;
    if (!pts || !mask || !depth || !color || !scratch) return GPSGS_E_INVALID;
    if (scratch_bytes < up_splat_scratch_bytes(B, res)) return GPSGS_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    uint64_t *keys = (uint64_t *)scratch;
    const int R2 = res * res;
    hipLaunchKernelGGL(k_zsplat_init, dim3((R2 + TPB - 1) / TPB, B), dim3(TPB), 0, s, depth, keys, R2);
    hipLaunchKernelGGL(k_zsplat_scatter, dim3((N + TPB - 1) / TPB, B, V), dim3(TPB), 0, s, pts, mask, B, N, res, keys);
    hipLaunchKernelGGL(k_zsplat_resolve, dim3((R2 + TPB - 1) / TPB, B), dim3(TPB), 0, s, keys, pts, B, N, res, depth, color);
    return launched();
}

extern "C" int up_flow2render_dev(int B, int S, int res, const float *flow_l, const float *flow_r, const float *mask_l, const float *mask_r,
                                  int64_t mask_batch_stride, const float *img_l, const float *img_r, const float *cams_dev, const float *novel_dev,
                                  void *scratch, size_t scratch_bytes, float *img_pred, float *pts_out, void *stream) {
    if (B < 0 || S < 0 || res < 0) return GPSGS_E_INVALID;
    if (B == 0 || res == 0) return GPSGS_OK;
    if (res > 32768 || S > 32768 || B > 65535 || 2 * (uint64_t)S * S + 1 > 0xffffffffull) return GPSGS_E_INVALID;
    if (!flow_l || !flow_r || !mask_l || !mask_r || !img_l || !img_r || !cams_dev || !novel_dev || !img_pred || !scratch) return GPSGS_E_INVALID;
    if (scratch_bytes < up_splat_scratch_bytes(B, res)) return GPSGS_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    uint64_t *keys = (uint64_t *)scratch;
    const int R2 = res * res, S2 = S * S;
    const F2RViews a = {{flow_l, flow_r}, {mask_l, mask_r}, {img_l, img_r}};
    hipLaunchKernelGGL(k_f2r_init, dim3((R2 + TPB - 1) / TPB, B), dim3(TPB), 0, s, keys, R2);
    if (S2 > 0)
        hipLaunchKernelGGL(k_f2r_scatter, dim3((S2 + TPB - 1) / TPB, B, 2), dim3(TPB), 0, s, a, B, S, res, mask_batch_stride, cams_dev, novel_dev,
                           pts_out, keys);
    hipLaunchKernelGGL(k_f2r_resolve, dim3((R2 + TPB - 1) / TPB, B), dim3(TPB), 0, s, a, keys, S, res, img_pred);
    return launched();
}
