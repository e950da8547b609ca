// unproject_common.h -- the per-pixel flow -> inverse depth -> world point arithmetic shared by unproject.hip (k_unproject_fwd) and
// splat.hip (k_f2r_scatter), so that both give the same bits.  Include only from units built with -ffp-contract=off.
#pragma once
#include "gsr_common.h"

#pragma clang fp contract(off)

namespace {

struct UnprojCam {  // per batch element
    float offset, tf, fx, fy, cx, cy;
    float Rt[9];   // R^T row-major
    float Rtt[3];  // R^T t
};

// Cameras in DEVICE memory: cams[b] = {ref_intr 3x3, intr 3x3, extr 3x4 row-major, Tf_x} = 31 floats (wave-uniform scalar loads; the arithmetic of
// unproject.hip's host fill(), operation for operation, so both forms give the same bits).
constexpr int CAM_FLOATS = 31;
__device__ __forceinline__ UnprojCam cam_from_device(const float *__restrict__ cams, int b) {
    const float *Kr = cams + (size_t)b * CAM_FLOATS, *K = Kr + 9, *E = Kr + 18;
    UnprojCam c;
    c.offset = Kr[2] - K[2]; c.tf = Kr[30]; c.fx = K[0]; c.fy = K[4]; c.cx = K[2]; c.cy = K[5];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) c.Rt[i * 3 + j] = E[j * 4 + i];
#pragma unroll
    for (int i = 0; i < 3; i++) c.Rtt[i] = c.Rt[i * 3] * E[3] + c.Rt[i * 3 + 1] * E[7] + c.Rt[i * 3 + 2] * E[11];
    return c;
}

// flow2depth (lib/utils.py:113-120): the INVERSE depth, times the mask
__device__ __forceinline__ float up_inverse_depth(const UnprojCam &c, float flow, float mask) {
    const float disparity = c.offset - flow;
    const float d = -disparity / c.tf;
    return d * mask;
}

// depth2pc (lib/utils.py:88-110) of pixel (u, v) with inverse depth d, in the reference's operation order
__device__ __forceinline__ void up_world_point(const UnprojCam &c, int u, int v, float d, float o[3]) {
    const float z = 1.0f / (d + 1e-8f);
    const float X = ((float)u + 0.5f - c.cx) * z / c.fx;
    const float Y = ((float)v + 0.5f - c.cy) * z / c.fy;
    o[0] = (c.Rt[0] * X + c.Rt[1] * Y + c.Rt[2] * z) - c.Rtt[0];
    o[1] = (c.Rt[3] * X + c.Rt[4] * Y + c.Rt[5] * z) - c.Rtt[1];
    o[2] = (c.Rt[6] * X + c.Rt[7] * Y + c.Rt[8] * z) - c.Rtt[2];
}

}  // namespace
