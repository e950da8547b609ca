/*
 * gpsgs.h -- C ABI of the MI355X-native render hot path of GPS-Gaussian (libgpsgs_hip.so).
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch types, no exceptions, no allocation and no
 * host synchronisation inside any entry point (all are hipGraph-capture safe).  Every function returns 0 on
 * success or a negative GPSGS_E_* code.  All pointers are DEVICE pointers unless marked host.  `stream` is a
 * hipStream_t passed as void* (NULL = the default stream).
 *
 * What each entry point replaces in the reference (paths relative to /root/reference):
 *
 *   gsr_forward / gsr_backward
 *       the `_C.rasterize_gaussians` / `_C.rasterize_gaussians_backward` calls made by the external CUDA
 *       extension `diff_gaussian_rasterization`, which the reference imports at gaussian_renderer/__init__.py:14
 *       and invokes at gaussian_renderer/__init__.py:51-62 (GaussianRasterizer.forward) and, through autograd,
 *       from train_stage2.py:83 (backward).  Argument meaning follows that call: precomputed colours, scale + rotation.  The other
 *       half of that module's interface -- `shs` (settings fields sh_degree / campos, constructed at gaussian_renderer/__init__.py:46-47)
 *       and `cov3D_precomp`, both passed as None by the reference (:56,:61) -- travels in GsrViewExt.
 *   cs_forward / cs_backward
 *       `corr_sampler.forward` / `corr_sampler.backward` of the external RAFT-Stereo sampler extension, called at
 *       core/corr.py:22 and core/corr.py:28.
 *   cv_build_forward / cv_build_backward, cs_lookup_forward / cs_lookup_backward
 *       CorrBlockFast1D: the all-pairs correlation volume + average-pool pyramid (core/corr.py:31-42, :53-61) and the lookup of
 *       all levels with the concatenation of core/corr.py:44-51 (four corr_sampler.forward calls + torch.cat in the reference).
 *   cu_upsample_forward / cu_upsample_backward
 *       RAFTStereoHuman.upsample_flow, core/raft_stereo_human.py:69-81 (softmax over the 9 taps + unfold + weighted sum).
 *   gsr_pack_views / gsr_pack_views_backward
 *       the per-sample flatten + boolean-mask gather + concat + rgb affine of lib/GaussianRender.py:15-34.
 *   up_unproject_forward / up_unproject_backward (+ _dev: cameras in device memory)
 *       flow2depth + depth2pc + the validity test: lib/utils.py:113-120, :88-110, lib/network.py:66-69.
 *   up_zsplat, up_flow2render_dev (+ up_splat_scratch_bytes)
 *       the z-buffer splat of lib/TaichiRender.py:13-24 and the whole TaichiRenderBatch.flow2render (:26-60), stage-1 validation render.
 *   fl_l1_ssim_forward / fl_l1_ssim_backward
 *       l1_loss + ssim of lib/loss.py:36-83 (and their autograd backward), called at train_stage2.py:70-72.
 *   gn_forward / gn_backward (+ gn_chunk_elems, gn_scratch_bytes)
 *       torch.nn.GroupNorm as the reference's feature extractor builds it (core/extractor.py:17-20, :68: groups of 8 channels x the whole plane)
 *       and its autograd backward: ATen's one-workgroup-per-row moments kernels, the largest single item of a view's GPU time.
 *   gne_forward / gne_backward
 *       the same layers with what the reference runs right after them folded in: `relu_(norm(conv(x)))` (core/extractor.py:51-52, :54-55, the
 *       Conv -> GroupNorm -> ReLU stem at :66-70) and the block's `relu(x + y)` (:60) -- ATen's clamp, add and copy kernels on the largest activations.
 *   sc_forward / sc_backward (+ sc_supported, sc_tile, sc_scratch_bytes)
 *       the two full-resolution stem convolutions, torch.nn.Conv2d(3 | 1, 32, 5, stride 2, padding 2) of core/extractor.py:66-70 (the depth
 *       encoder's through lib/gs_parm_network.py:14) and their autograd backward: the library's implicit-GEMM kernels with a K step of 4 and the
 *       NCHW <-> NHWC transposes around them.
 *   gsr_head_forward / gsr_head_backward (+ gsr_head_supported, gsr_head_tile, gsr_head_scratch_bytes)
 *       the tail of the three Gaussian-parameter heads, nn.ReLU -> nn.Conv2d(32, 4 | 3 | 1, 1) -> nothing | nn.Softplus(beta=100) | nn.Sigmoid of
 *       lib/gs_parm_network.py:34-50 on the full-resolution hidden tensor, and its autograd backward: ATen's clamp pass, the library's 1x1
 *       implicit GEMM between NCHW <-> NHWC transposes, and the elementwise activation.
 *   c3_forward / c3_backward (+ c3_supported, c3_tile, c3_scratch_bytes)
 *       the regresser's full-resolution 3x3 convolutions, nn.Conv2d(52, 32, 3, padding=1) + nn.ReLU (`out_conv`, `out_relu`) and the
 *       nn.Conv2d(32, 32, 3, padding=1) at the top of each head (lib/gs_parm_network.py:27-50), and their autograd backward.
 *   c1_forward / c1_backward (+ c1_supported, c1_tile, c1_scratch_bytes)
 *       the 1x1 convolution that opens the shortcut of every ResidualBlock whose input and output differ, nn.Conv2d(in, planes, 1, stride)
 *       with stride 1 or 2 (core/extractor.py:43-45), and its autograd backward.
 *   rc_forward / rc_backward (+ rc_supported, rc_tile, rc_scratch_bytes)
 *       the two stride-1 3x3 convolutions of a ResidualBlock, `conv1` and `conv2` = nn.Conv2d(in, planes, 3, padding=1) (core/extractor.py:10-11)
 *       at the widths of the depth encoder and the regresser's decoders, and their autograd backward.
 *   uc_forward / uc_backward (+ uc_supported, uc_tile)
 *       the regresser's decoder glue, `self.up(...)` (nn.Upsample(scale_factor=2, mode="bilinear")) followed by torch.cat with the skip
 *       tensors, three times in GSRegresser.forward (lib/gs_parm_network.py:56-67), and its autograd backward: ATen's upsample kernel, the
 *       copies of the concatenations, and the atomics-based upsample backward.
 */
#ifndef GPSGS_H
#define GPSGS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPSGS_ABI_VERSION 4 /* 2: + GsrViewExt, gsr_forward_ex, gsr_backward_ex; header words num_points / row_overflow (additive)
                               3: GsrViewExt grew from 32 to 80 bytes: SH colours and precomputed 3D covariances (the `shs` / `cov3D_precomp`
                                  inputs of the upstream module, + their gradients); zero-initialised it means what version 2 meant
                               4: + gsr_mark_visible (upstream GaussianRasterizer.markVisible); gsr_debug_count_records takes workspace_bytes;
                                  DIRECT bin lists: GsrViewExt.reserved0 became bin_capacity (0 = what version 3 did), gsr_workspace_bytes_ex,
                                  gsr_direct_lists_ok; gsr_export_state / gsr_debug_count_records take bin_capacity
                               still 4 after up_splat_scratch_bytes, up_zsplat, up_flow2render_dev: purely additive, nothing existing changed
                               still 4 after the depth / alpha maps: GsrViewExt.reserved[4] became two pointer slots (out_depth | dL_ddepth,
                                  out_alpha | dL_dalpha; zero = none, what 4 did, same 80-byte struct) + gsr_workspace_bytes_depth_alpha
                               still 4 after the feature maps: GsrFeatures, gsr_workspace_bytes_features, gsr_forward_features,
                                  gsr_backward_features (additive)
                               still 4 after the contribution statistics: GsrContrib, gsr_workspace_bytes_contrib, gsr_forward_contrib (additive)
                               still 4 after the absolute screen-space gradient: GsrAbsGrad, gsr_workspace_bytes_absgrad, gsr_backward_absgrad (additive)
                               still 4 after the depth-distortion map: GsrDistort, gsr_forward_distort, gsr_backward_distort (additive)
                               still 4 after GroupNorm: gn_chunk_elems, gn_scratch_bytes, gn_forward, gn_backward (additive)
                               still 4 after the GroupNorm epilogues: gne_forward, gne_backward (additive)
                               still 4 after the stem convolution: sc_supported, sc_tile, sc_scratch_bytes, sc_forward, sc_backward (additive)
                               still 4 after the Gaussian heads: gsr_head_supported, gsr_head_tile, gsr_head_scratch_bytes, gsr_head_forward,
                                  gsr_head_backward (additive)
                               still 4 after the 3x3 convolutions: c3_supported, c3_tile, c3_scratch_bytes, c3_forward, c3_backward (additive)
                               still 4 after the 1x1 convolutions: c1_supported, c1_tile, c1_scratch_bytes, c1_forward, c1_backward (additive)
                               still 4 after the residual-block 3x3 convolutions: rc_supported, rc_tile, rc_scratch_bytes, rc_forward, rc_backward
                                  (additive)
                               still 4 after the decoder glue: uc_supported, uc_tile, uc_forward, uc_backward (additive) */

enum {
    GPSGS_OK = 0,
    GPSGS_E_INVALID = -1,    /* bad argument (NULL pointer, negative size, unsupported dtype) */
    GPSGS_E_WORKSPACE = -2,  /* workspace_bytes smaller than gsr_workspace_bytes() for these dimensions */
    GPSGS_E_LAUNCH = -3,     /* a HIP launch failed (hipGetLastError != hipSuccess) */
    GPSGS_E_NO_DEVICE = -4,  /* no HIP device */
    GPSGS_E_INTERNAL = -5    /* GSR_FLAG_DEBUG only: the forward's self-check failed (a bin list holds an id that is not a Gaussian of the view, is
                                out of (depth, index) order, or the scatter pass did not fill exactly the slots the count pass reserved) */
};

/* flags for gsr_forward / gsr_backward */
#define GSR_FLAG_DEBUG 1u  /* synchronise and check after every kernel (the reference hard-codes debug=False); the forward also validates its
                              bin lists between the sort and the compositing (GPSGS_E_INTERNAL) */
#define GSR_FLAG_TIMING 2u /* bracket every stage with hipEvents on `stream`; read them with gsr_timing_read() */
#define GSR_FLAG_NO_LARGE_SORT 4u /* the caller expects no bin list longer than 1024 entries: the (normally idle) 1024-thread sort
                                    launch is skipped.  If a longer list does turn up, the scan reports it as an OVERFLOW (nothing is
                                    rendered; max_tile_count > 1024 in the header tells the two cases apart): call again without it */
#define GSR_FLAG_COMPOSITE_TILES 8u /* compositing kernels that take the exponents of all (pixel, splat) pairs from bf16 matrix-core
                                      tiles (gsr_composite_tiles.hip, exact split evaluation) instead of computing them per pair on the
                                      vector ALUs (gsr_composite.hip).  Forward and backward of one view must agree on it. */
#define GSR_FLAG_NO_COLOR_GRAD 256u /* gsr_backward: the caller does not need dL_dcolors (stage 2: the colours are input pixels, which
                                       train_stage2.py never differentiates; torch: colors_precomp.requires_grad is False).  The tile family then
                                       leaves the three colour sums per (pixel, splat) out; dL_dcolors is written as zeros, every other gradient is
                                       bit-identical.  The VALU family ignores the flag (computes everything). */
#define GSR_FLAG_WAVE_PRIORITY 512u /* tile family: the compositing waves set their hardware priority (s_setprio) from the work they still
                                       have in front of them -- forward: more list left = higher priority, so that the waves resident on a SIMD
                                       finish together instead of one after the other (the arbiter serves the oldest wave first); backward:
                                       workgroups dispatched after the first resident generation overtake the leftovers of that generation.
                                       Results are unchanged.  It pays when a view's kernels have the chip to themselves (measured, config 2:
                                       forward 55 -> 51 us, backward 114 -> 110 us); with several views' kernels overlapped on other streams it
                                       costs ~2 % of the aggregate rate, so it is opt-in per call. */
#define GSR_FLAG_ANTIALIAS 1024u /* antialiasing: the opacity-compensated screen-space filter of Mip-Splatting (upstream's `antialiasing=True`).
                                    Each visible splat's opacity becomes opacity * k, k = sqrt(max(rho, 2.5e-5)), rho = (a0 c0 - b^2) /
                                    ((a0 + 0.3)(c0 + 0.3) - b^2) with (a0, b, c0) its 2D covariance before the 0.3 px^2 dilation: compositing,
                                    the alpha >= 1/255 tests and the depth / alpha maps all see that value, and the backward chains dL/dk into
                                    the covariance.  Conic, radii, bin rects and depth order are unchanged.  Forward and backward of one view
                                    must agree on it (the backward also needs `opacities` then).  Check gsr_supported_flags() before relying on
                                    it: libraries before it ignore the bit. */
#define GSR_FLAG_TIMING_STAGE(k) (GSR_FLAG_TIMING | (((unsigned)(k) + 1u) << 4)) /* ... or only stage k (GSR_STAGE_*) */

/* stage ids reported by gsr_timing_read() */
enum {
    GSR_STAGE_PREPROCESS = 0, GSR_STAGE_SCAN, GSR_STAGE_SCATTER, GSR_STAGE_SORT, GSR_STAGE_COMPOSITE_FWD,
    GSR_STAGE_COMPOSITE_BWD, GSR_STAGE_PREPROCESS_BWD, GSR_STAGE_COUNT
};

int gpsgs_abi_version(void);
/* The GSR_FLAG_* bits this library honours (the GSR_FLAG_TIMING_STAGE field, bits 4..7, not included).  Unknown bits are ignored by
 * gsr_forward / gsr_backward, so a host that needs a later flag (GSR_FLAG_ANTIALIAS) checks for it here. */
int gsr_supported_flags(void);
/* Development aid: rows_device = 2 * bins rows of 4 u64 (zeroed by the caller), or NULL to switch it off.  While set, every tile-compositing
 * workgroup that did work records {wall clock at start, at end (100 MHz), shader cycles, HW_ID | XCC_ID << 32 | list length << 40} in row
 * blockIdx (forward) / bins + blockIdx (backward): the per-SIMD timeline tools/wg_trace.py analyses.  Process-wide, not thread-safe. */
int gsr_debug_set_wg_trace(unsigned long long *rows_device);

/* Diagnostic (synchronises `stream`): the shader clock in MHz under a chip-filling VALU load of a few milliseconds, from the ratio of
 * the per-cycle counter (s_memtime) to the constant-rate wall clock.  scratch3_device: 24 bytes of device memory.  bench.py prices the
 * VALU issue rate with it instead of assuming the 2.4 GHz maximum. */
int gpsgs_measure_sclk(unsigned long long *scratch3_device, double *mhz_host, void *stream);
const char *gpsgs_build_info(void); /* "gfx950 <compiler> <date>" */

/* ---- rasteriser ---------------------------------------------------------------------------------------------
 * Workspace: one caller-owned device buffer (>= gsr_workspace_bytes, 256-byte aligned) that carries the forward's
 * state to the backward (what upstream keeps in geomBuffer / binningBuffer / imgBuffer).
 * `instance_capacity` bounds R = number of (Gaussian, 8x8-pixel bin) instances the buffer can hold.  R is data dependent; the
 * forward never reads it back.  Instead the header records the R that was needed and an overflow flag:
 *   - overflow == 0: results are exact;
 *   - overflow != 0: NOTHING was rendered (out_color untouched apart from zero fill); the caller must re-run with
 *     instance_capacity >= max(num_rendered, num_slots) as reported.  (Upstream sizes the buffer with a blocking D2H read of R on every call.)
 */
typedef struct GsrHeader {      /* first bytes of the workspace, device memory */
    uint64_t num_rendered;      /* R needed by the last gsr_forward */
    uint32_t overflow;          /* 1 if R (or, with a backward tail, num_slots) > instance_capacity */
    uint32_t max_tile_count;    /* longest per-bin list (one 8x8-pixel bin = one wave64 work item) */
    uint32_t num_busy_wgs;      /* bins with a non-empty list; they are scheduled first */
    uint32_t num_slots;         /* training workspaces only: bin-rect cells of all Gaussians (one gradient-record slot each); also <= capacity */
    uint32_t num_points;        /* Gaussians of this view: P, or end - begin of GsrViewExt.row_range */
    uint32_t row_overflow;      /* 1 if a row range held more rows than the P (= row capacity) the call was made with: reported as overflow */
    uint32_t reserved[8];       /* scratch of the library (direct lists: the accumulators of the totals workgroups); zeroed by every forward */
} GsrHeader;

/* direct lists (GsrViewExt.bin_capacity): 1 if this image size and capacity can use them (capacity a multiple of 64 in 64..1024, at most 65,536 bins) */
int gsr_direct_lists_ok(int width, int height, uint32_t bin_capacity);
/* workspace size for either list form (bin_capacity 0 = scanned: then equal to the two functions below); 0 on invalid arguments.  With direct lists
 * instance_capacity still bounds the gradient-record slots of a training workspace (header.num_slots); the lists themselves take bins x bin_capacity entries */
size_t gsr_workspace_bytes_ex(int P, int width, int height, int64_t instance_capacity, uint32_t bin_capacity, int forward_only);
size_t gsr_workspace_bytes(int P, int width, int height, int64_t instance_capacity);              /* forward + backward */
/* gsr_workspace_bytes_ex plus room for the depth / alpha backward (GsrViewExt.dL_ddepth / dL_dalpha); forward_only: the same as gsr_workspace_bytes_ex
 * (the forward of the maps needs nothing extra) */
size_t gsr_workspace_bytes_depth_alpha(int P, int width, int height, int64_t instance_capacity, uint32_t bin_capacity, int forward_only);
size_t gsr_workspace_bytes_forward_only(int P, int width, int height, int64_t instance_capacity); /* inference: no backward tail; a forward on
                                                                                                     such a workspace also skips the per-pixel state
                                                                                                     only a backward reads (final T, last contributor) */

/* Forward.  Inputs fp32, contiguous: means3D[P,3], colors[P,3], opacities[P], scales[P,3], rotations[P,4] (w,x,y,z;
 * NOT re-normalised), viewmatrix[16], projmatrix[16] (flat column-major = the transposed tensors the reference
 * passes), bg[3].  Outputs: out_color[3,H,W], radii[P].  P == 0: out_color is zero-filled (not background). */
int gsr_forward(int P, int width, int height, const float *means3D, const float *colors, const float *opacities,
                const float *scales, const float *rotations, float scale_modifier, float tanfovx, float tanfovy,
                const float *viewmatrix, const float *projmatrix, const float *bg, float *out_color, int *radii,
                void *workspace, size_t workspace_bytes, int64_t instance_capacity, unsigned flags, void *stream);

/* gsr_forward with EARLY capacity notification.  `host_header_out` is 32 bytes of PINNED host memory the device can write
 * (hipHostMalloc / hipHostRegister; torch pin_memory()).  As soon as the binning scan knows the instance count -- about a fifth
 * of the way into the forward, before scatter / sort / compositing run -- the device stores the first 28 header bytes
 * {u64 num_rendered; u32 overflow, max_tile_count, num_busy_wgs (0 with direct lists: the work order is made later), num_slots, 0} there and then release-stores `notify_seq`
 * (non-zero, chosen by the caller, different from the word's current value) into the u32 at byte 28.  The host spins on that
 * word instead of waiting for the whole forward: the capacity check of the reference's blocking `num_rendered` readback
 * (rasterizer_impl.cu forward, cudaMemcpy of the scan total) then costs no GPU idle time.  With P == 0 nothing is written.
 * GPSGS_E_INVALID if the pointer is not device-visible pinned memory or notify_seq == 0. */
int gsr_forward_notify(int P, int width, int height, const float *means3D, const float *colors, const float *opacities,
                       const float *scales, const float *rotations, float scale_modifier, float tanfovx, float tanfovy,
                       const float *viewmatrix, const float *projmatrix, const float *bg, float *out_color, int *radii,
                       void *workspace, size_t workspace_bytes, int64_t instance_capacity, unsigned flags, void *stream,
                       void *host_header_out, uint32_t notify_seq);

/* Optional extras of one view (gsr_forward_ex / gsr_backward_ex); zero-initialise, NULL = none.
 *   row_range   DEVICE pointer to two u32 {begin, end}: the Gaussians of this view are rows [begin, end) of the per-Gaussian input
 *               arrays AND of the per-Gaussian outputs (radii, the six gradient arrays) -- the arrays are batch-wide, as
 *               lib/GaussianRender.py:15-34 would leave them if it did not split per sample -- and `P` is only a CAPACITY: it sizes the
 *               workspace and the launches, the kernels read the real count from the device.  The host then never needs the number of
 *               valid pixels of a sample (the reference learns it through ten boolean-mask gathers = ten device syncs per sample).
 *               end - begin > P is reported like an instance overflow (header: row_overflow = 1, num_points = end - begin).
 *   order_hint  longest per-bin list of an earlier, similar view (header.max_tile_count), 0 = unknown.  The scan dispatches the
 *               bins whose list exceeds 1/2 and 1/4 of it first (a bin is one wave's sequential job: longest-processing-time-first).
 *               Decides the ORDER of the work only, never a result. */
typedef struct GsrViewExt {
    const uint32_t *row_range;
    uint32_t order_hint;
    /* ---- ABI 3: appearance / covariance inputs the reference never passes but its rasteriser module accepts ---------------------------
     *   shs            DEVICE [rows, sh_coeffs, 3] real spherical-harmonics coefficients (sh_coeffs <= 16), evaluated up to degree
     *                  sh_degree (0..3, (sh_degree + 1)^2 <= sh_coeffs) in the direction campos -> mean, + 0.5, clamped at 0 (upstream
     *                  computeColorFromSH).  With shs the `colors` argument of the call must be NULL (exactly one of the two), campos
     *                  (DEVICE [3], the settings' camera centre) is required, and the backward writes dL_dsh [rows, sh_coeffs, 3]
     *                  (zeros beyond the active degree and for invisible Gaussians) and adds the view-direction term to dL_dmeans3D;
     *                  its dL_dcolors argument may then be NULL.
     *   cov3D_precomp  DEVICE [rows, 6] upper triangles (xx, xy, xz, yy, yz, zz), used as given (scale_modifier does not apply).  With it
     *                  `scales` and `rotations` must be NULL (exactly one of the two forms); the backward writes dL_dcov3D [rows, 6]
     *                  (upstream's convention: an off-diagonal entry carries both symmetric positions) and leaves dL_dscales / dL_drotations
     *                  untouched (they may be NULL). */
    uint32_t sh_degree;
    uint32_t sh_coeffs;
    /* ---- ABI 4: DIRECT bin lists.  0 = scanned lists (every earlier version).  > 0 (a multiple of 64, <= 1024; gsr_direct_lists_ok()): every 8x8-pixel bin
     *   owns a fixed-capacity segment of bin_capacity list entries, so an instance's slot follows from the base the count atomic of the preprocess returned
     *   without any offsets: the scatter needs no scan in front of it, and what is left of the scan (header, work order, slot prefix) rides in the scatter
     *   launch; with the tile compositing family the forward compositing waves sort their own lists, so there is no sort launch either -- three launches
     *   in front of the compositing instead of five, none of them a latency chain.  The workspace must be sized with gsr_workspace_bytes_ex(..., bin_capacity, ...); forward and backward of a view must
     *   pass the same value.  A view whose longest list exceeds bin_capacity is NOT rendered: header.overflow = 1 with header.max_tile_count >
     *   bin_capacity -- repeat it with a larger capacity or with scanned lists (the capacity question upstream answers with a blocking read of R). */
    uint32_t bin_capacity;
    const float *shs;
    const float *campos;
    const float *cov3D_precomp;
    float *dL_dsh;      /* gsr_backward_ex only */
    float *dL_dcov3D;   /* gsr_backward_ex only */
    /* ---- opt-in DEPTH and ALPHA maps of the view (the former reserved[4]; NULL = none).  Two more channels of the same blend -- same splats, sort order
     *   and power > 0 / alpha < 1/255 / T < 1e-4 decisions -- with background 0:
     *     depth[p] = sum_i z_i alpha_i T_i   (z_i the Gaussian's view-space depth; NOT normalised: divide by alpha for the expected depth)
     *     alpha[p] = sum_i alpha_i T_i       (= 1 - final T, but accumulated as the sum, so that its gradient follows the colour recurrence)
     *   gsr_forward_ex: out_depth / out_alpha, DEVICE [H, W] fp32 (4-byte aligned; either may be NULL).  Both NULL: the plain kernels run, bit for bit.
     *   gsr_backward_ex: dL_ddepth / dL_dalpha, DEVICE [H, W] (either may be NULL = zero).  They reach dL_dopacity, dL_dmeans2D, the conic and
     *   through it dL_dscales / dL_drotations / dL_dcov3D exactly as a colour channel with c = z_i resp. c = 1 would, and dL/dz_i = sum_p dL_ddepth
     *   alpha_i T_i adds dL/dz * viewmatrix[:, 2] to dL_dmeans3D.  The workspace must then be sized with gsr_workspace_bytes_depth_alpha (one more
     *   float per instance slot; GPSGS_E_WORKSPACE otherwise).
     *   The maps are made by the VALU compositing kernels: with either output / gradient set, GSR_FLAG_COMPOSITE_TILES is ignored, so a view whose
     *   forward produced the maps has to run its backward with the VALU family too (pass a depth / alpha gradient, or leave the tiles flag off). */
    union { float *out_depth; const float *dL_ddepth; };
    union { float *out_alpha; const float *dL_dalpha; };
} GsrViewExt;

/* gsr_forward_notify + GsrViewExt (host_header_out may be NULL: no notification, like gsr_forward).  The early header's word 6 carries
 * num_points. */
int gsr_forward_ex(int P, int width, int height, const float *means3D, const float *colors, const float *opacities,
                   const float *scales, const float *rotations, float scale_modifier, float tanfovx, float tanfovy,
                   const float *viewmatrix, const float *projmatrix, const float *bg, float *out_color, int *radii,
                   void *workspace, size_t workspace_bytes, int64_t instance_capacity, unsigned flags, void *stream,
                   void *host_header_out, uint32_t notify_seq, const GsrViewExt *ext);

/* Backward.  Same inputs and the workspace left by the matching gsr_forward, plus dL_dpix[3,H,W] (contiguous).
 * Writes (does not accumulate) dL_dmeans3D[P,3], dL_dmeans2D[P,3], dL_dcolors[P,3], dL_dopacity[P],
 * dL_dscales[P,3], dL_drotations[P,4]. */
int gsr_backward(int P, int width, int height, const float *means3D, const float *colors, const float *opacities,
                 const float *scales, const float *rotations, float scale_modifier, float tanfovx, float tanfovy,
                 const float *viewmatrix, const float *projmatrix, const float *bg, const int *radii,
                 const float *dL_dpix, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dcolors,
                 float *dL_dopacity, float *dL_dscales, float *dL_drotations, void *workspace,
                 size_t workspace_bytes, int64_t instance_capacity, unsigned flags, void *stream);

/* gsr_backward + GsrViewExt (the same row_range the forward was given). */
int gsr_backward_ex(int P, int width, int height, const float *means3D, const float *colors, const float *opacities,
                    const float *scales, const float *rotations, float scale_modifier, float tanfovx, float tanfovy,
                    const float *viewmatrix, const float *projmatrix, const float *bg, const int *radii,
                    const float *dL_dpix, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dcolors,
                    float *dL_dopacity, float *dL_dscales, float *dL_drotations, void *workspace,
                    size_t workspace_bytes, int64_t instance_capacity, unsigned flags, void *stream, const GsrViewExt *ext);

/* Camera gradients (opt-in).  gsr_backward_camera is gsr_backward_ex with the same arguments -- it writes every per-Gaussian gradient with the
 * same bits and honours the same flags and GsrViewExt fields -- and also WRITES (does not accumulate) the gradient of the loss with respect to
 * the camera, each a DEVICE array that may be NULL (not wanted):
 *   dL_dviewmatrix[16], dL_dprojmatrix[16]: flat column-major as viewmatrix / projmatrix are read, element (r, c) at index 4 c + r (the
 *     transposed [4,4] tensor the reference passes, read as tensor.reshape(16)).  Per visible Gaussian, m~ = (x, y, z, 1):
 *       dL/dv[4c+r] += dt[r] m~[c] (r < 3), dt = dL/d(view-space mean), depth-map term included; + (J^T dL/dT)[r][c] (r, c < 3), T = J W and
 *       J the clamped EWA Jacobian the forward used.  Row 3 (indices 3, 7, 11, 15) is never read and is exactly 0.
 *       dL/dp[4c+r] = dh[r] m~[c], h = projmatrix m~, dh = (g0 w, g1 w, 0, -(g0 h0 + g1 h1) w^2), w = 1 / (h3 + 1e-7), g = dL/dmean2D (NDC).
 *       Row 2 (indices 2, 6, 10, 14) is exactly 0.
 *   dL_dcampos[3]: minus the SH view-direction term of dL_dmeans3D; exactly 0 without shs.
 * The conventions are the backward's own (straight-through min(0.99) clamp, 1/(det^2 + 1e-7) conic gradient, clamped view-space x/y constant); all
 * discrete decisions are constants.  An overflowed forward gives zeros.  tanfov, scale_modifier and bg get no gradient.
 * Deterministic: each preprocess-backward workgroup sums its Gaussians' shares in a fixed order into scratch, a second launch sums those in a fixed
 * order -- no atomics, the same bits on every run, stream and view in flight.  scratch: DEVICE, at least gsr_camera_grad_scratch_bytes(P) bytes
 * (one per view in flight; GPSGS_E_WORKSPACE otherwise; may be NULL when P = 0 or no output is wanted).  With all three outputs NULL the call is
 * gsr_backward_ex.  No host synchronisation. */
size_t gsr_camera_grad_scratch_bytes(int P);
int gsr_backward_camera(int P, int width, int height, const float *means3D, const float *colors, const float *opacities,
                        const float *scales, const float *rotations, float scale_modifier, float tanfovx, float tanfovy,
                        const float *viewmatrix, const float *projmatrix, const float *bg, const int *radii,
                        const float *dL_dpix, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dcolors,
                        float *dL_dopacity, float *dL_dscales, float *dL_drotations, void *workspace,
                        size_t workspace_bytes, int64_t instance_capacity, unsigned flags, void *stream, const GsrViewExt *ext,
                        float *dL_dviewmatrix, float *dL_dprojmatrix, float *dL_dcampos, void *scratch, size_t scratch_bytes);

/* F-channel feature maps (opt-in).  A per-Gaussian feature vector f[i, 0..F) is splatted with the image's blend weights:
 *   feat[c, p] = sum_i f[i, c] alpha_i T_i,  background 0
 * -- the image's splats, sort order and power > 0 / alpha < 1/255 / T < 1e-4 decisions (for a feature background, add (1 - alpha) bg_f with the
 * alpha map).  Rendered by the VALU compositing family: with features the tiles flag is ignored for that view's forward and backward, and the image
 * has the bits of a plain VALU render.  Combines with depth / alpha maps, antialiasing, camera gradients, shs, cov3D_precomp, row ranges, both list
 * forms and GSR_FLAG_NO_COLOR_GRAD.
 *   features: DEVICE [rows, F] fp32, 4-byte aligned, rows as GsrViewExt.row_range says (the same rows as means3D).
 *   gsr_forward_features: out_features DEVICE [F, H, W] (written).
 *   gsr_backward_features: dL_dfeaturemap DEVICE [F, H, W], NULL = zero gradient (the per-Gaussian gradients then have the bits of a plain VALU
 *     backward and dL_dfeatures is zero-filled); dL_dfeatures DEVICE [rows, F], WRITTEN for the view's rows (NULL = not wanted):
 *     dL/df[i, c] = sum_p alpha_i T_i dL/dfeat[c, p].  dL/dfeat reaches opacity, means2D, the conic and means3D exactly as F more colour channels
 *     with background 0 would.  No atomics: per (bin, splat) instance the F sums go to the workspace's feature tail, a gather streams each
 *     Gaussian's slots in slot order -- the same bits on every run.  The workspace must be sized with gsr_workspace_bytes_features (the depth /
 *     alpha tail plus cap x F floats); its camera outputs may be NULL, so it serves every combination (it is gsr_backward_camera otherwise).
 * channels = 0 (or a NULL GsrFeatures) is the call without features.  GPSGS_E_INVALID for channels outside 0..GSR_MAX_FEATURES, NULL features with
 * channels > 0 and P > 0 (a view without Gaussians has no rows: NULL is accepted there), pointers that are not 4-byte aligned; GPSGS_E_WORKSPACE for
 * a workspace that is too small. */
#define GSR_MAX_FEATURES 64
typedef struct GsrFeatures {
    int32_t channels;   /* F in 1..GSR_MAX_FEATURES; 0 = none */
    uint32_t reserved0; /* 0 */
    const float *features;                                        /* DEVICE [rows, F]; follows GsrViewExt.row_range */
    union { float *out_features; const float *dL_dfeaturemap; };  /* [F, H, W]; backward: NULL = zero gradient */
    float *dL_dfeatures;                                          /* backward: [rows, F], written; NULL = not wanted */
} GsrFeatures;
/* gsr_workspace_bytes_depth_alpha(...) plus the 256-byte aligned feature tail (instance_capacity x channels floats); forward_only: the forward-only
 * size (the forward writes no tail).  0 for channels outside 1..GSR_MAX_FEATURES or invalid arguments. */
size_t gsr_workspace_bytes_features(int P, int width, int height, int64_t instance_capacity, uint32_t bin_capacity, int channels, int forward_only);
int gsr_forward_features(int P, int width, int height, const float *means3D, const float *colors, const float *opacities,
                         const float *scales, const float *rotations, float scale_modifier, float tanfovx, float tanfovy,
                         const float *viewmatrix, const float *projmatrix, const float *bg, float *out_color, int *radii,
                         void *workspace, size_t workspace_bytes, int64_t instance_capacity, unsigned flags, void *stream,
                         void *host_header_out, uint32_t notify_seq, const GsrViewExt *ext, const GsrFeatures *feat);
int gsr_backward_features(int P, int width, int height, const float *means3D, const float *colors, const float *opacities,
                          const float *scales, const float *rotations, float scale_modifier, float tanfovx, float tanfovy,
                          const float *viewmatrix, const float *projmatrix, const float *bg, const int *radii,
                          const float *dL_dpix, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dcolors,
                          float *dL_dopacity, float *dL_dscales, float *dL_drotations, void *workspace,
                          size_t workspace_bytes, int64_t instance_capacity, unsigned flags, void *stream, const GsrViewExt *ext,
                          float *dL_dviewmatrix, float *dL_dprojmatrix, float *dL_dcampos, void *scratch, size_t scratch_bytes,
                          const GsrFeatures *feat);

/* Per-Gaussian contribution statistics (opt-in).  A (pixel p, Gaussian i) pair is BLENDED when the forward adds i's colour to p -- the image's
 * splats, sort order and power > 0 / alpha < 1/255 / T < 1e-4 decisions -- with the weight w(p, i) = alpha T that the image, the depth / alpha and
 * the feature maps use (alpha from the compensated opacity with GSR_FLAG_ANTIALIAS).  Per Gaussian, indexed like radii:
 *   weight_sum[i]  = sum_p w(p, i)       fp32
 *   weight_max[i]  = max_p w(p, i), or 0 fp32
 *   pixel_count[i] = #{p : (p, i) blended} int32
 * Culled Gaussians (radii 0) and every Gaussian of an overflowed view get zeros.  Not differentiable.  No atomics: per (bin, splat) instance the
 * forward keeps {sum, max, count} in the workspace's contribution tail, a gather streams each Gaussian's slots in slot order -- the same bits on every
 * run.  Rendered by the VALU compositing family (the tiles flag is ignored for the view): the image, final T, the depth / alpha maps and what the
 * backward reads have the bits of a plain VALU forward, so gsr_backward_ex on the same workspace gives the same gradients as without statistics.
 * Each pointer may be NULL (not wanted); with a row range only the view's rows are written.  GPSGS_E_INVALID for pointers that are not 4-byte
 * aligned or a non-NULL `reserved`; GPSGS_E_WORKSPACE for a workspace smaller than gsr_workspace_bytes_contrib (when any pointer is set).  Combines with the depth / alpha
 * maps, antialiasing, shs, cov3D_precomp, row ranges and both list forms; not with feature maps (there is no entry point taking both). */
typedef struct GsrContrib {
    float *weight_sum;    /* DEVICE [rows] or NULL */
    float *weight_max;    /* DEVICE [rows] or NULL */
    int32_t *pixel_count; /* DEVICE [rows] or NULL */
    void *reserved;       /* NULL */
} GsrContrib;
/* gsr_workspace_bytes_depth_alpha(..., 0) plus the 256-byte aligned contribution tail (instance_capacity x 16 bytes).  forward_only: the same size --
 * the statistics need the per-Gaussian slot prefix of the backward tail, which the forward then also fills (such a forward counts the gradient-record
 * slots against instance_capacity, as a training forward does).  0 on invalid arguments. */
size_t gsr_workspace_bytes_contrib(int P, int width, int height, int64_t instance_capacity, uint32_t bin_capacity, int forward_only);
int gsr_forward_contrib(int P, int width, int height, const float *means3D, const float *colors, const float *opacities,
                        const float *scales, const float *rotations, float scale_modifier, float tanfovx, float tanfovy,
                        const float *viewmatrix, const float *projmatrix, const float *bg, float *out_color, int *radii,
                        void *workspace, size_t workspace_bytes, int64_t instance_capacity, unsigned flags, void *stream,
                        void *host_header_out, uint32_t notify_seq, const GsrViewExt *ext, const GsrContrib *contrib);

/* Absolute screen-space gradient (opt-in; AbsGS's "homodirectional gradient", gsplat's absgrad).  dL_dmeans2D[i, 0:2] is a SIGNED sum over the pixels
 * Gaussian i covers and cancels where the loss pulls the two sides of a Gaussian apart; this is the sum of the per-pixel magnitudes.  In the backward's
 * own conventions (straight through min(0.99, .), every discrete decision held constant, d = mean2D_i - pixel): a (pixel p, Gaussian i) pair receives
 * gradient when its list position is in front of p's last contributor, not power > 0, and alpha >= 1/255; with s = opacity_i dL/dalpha G (opacity_i the
 * compensated one with GSR_FLAG_ANTIALIAS; dL/dalpha including the depth / alpha maps' gradients when ext passes them) and the conic (A, B, C)
 *   t_x(p, i) = 0.5 W s (-A d_x - B d_y)        t_y(p, i) = 0.5 H s (-C d_y - B d_x)
 *   dL_dmeans2D[i, 0:2] = ( sum_p t_x , sum_p t_y )          (as without it, bit for bit)
 *   absgrad[i, 0:2]     = ( sum_p |t_x| , sum_p |t_y| )      fp32, in dL_dmeans2D's units (NDC-scaled), never negative
 * indexed like radii; exactly 0 for culled Gaussians (radii 0), for Gaussians no pixel gives gradient to and for every Gaussian of an overflowed view.
 * Every call OVERWRITES the view's rows (with a row range only those).  No atomics: per (bin, splat) record the backward compositing kernel keeps the
 * two sums in the workspace's absgrad tail, a gather streams each Gaussian's flagged slots in slot order -- the same bits on every run.  Made by the VALU
 * compositing family: the tiles flag is ignored by this call, and the FORWARD that filled the workspace must have run without
 * GSR_FLAG_COMPOSITE_TILES too (the two families round the exponent differently).  Every other output of the call -- all gradients -- has the bits of
 * gsr_backward_camera; a NULL `abs` or a NULL abs->absgrad IS gsr_backward_camera.  GPSGS_E_INVALID for a pointer that is not 4-byte aligned or a
 * non-NULL `reserved`; GPSGS_E_WORKSPACE for a workspace smaller than gsr_workspace_bytes_absgrad.  No host synchronisation.  Combines with the depth /
 * alpha gradients, antialiasing, camera gradients, shs, cov3D_precomp, row ranges, both list forms and GSR_FLAG_NO_COLOR_GRAD; not with feature maps
 * (there is no entry point taking both). */
typedef struct GsrAbsGrad {
    float *absgrad; /* DEVICE [rows, 2], written; NULL = not wanted */
    void *reserved; /* NULL */
} GsrAbsGrad;
/* gsr_workspace_bytes_depth_alpha(..., 0) plus the 256-byte aligned absgrad tail (instance_capacity x 8 bytes); size the FORWARD's workspace with it.
 * The tail takes the place of the contribution tail, which is dead once gsr_forward_contrib has returned its statistics: a workspace sized with
 * gsr_workspace_bytes_contrib (never smaller) serves a view that wants both.  0 on invalid arguments. */
size_t gsr_workspace_bytes_absgrad(int P, int width, int height, int64_t instance_capacity, uint32_t bin_capacity);
/* gsr_backward_camera's argument list, then the GsrAbsGrad */
int gsr_backward_absgrad(int P, int width, int height, const float *means3D, const float *colors, const float *opacities,
                         const float *scales, const float *rotations, float scale_modifier, float tanfovx, float tanfovy,
                         const float *viewmatrix, const float *projmatrix, const float *bg, const int *radii,
                         const float *dL_dpix, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dcolors, float *dL_dopacity,
                         float *dL_dscales, float *dL_drotations, void *workspace, size_t workspace_bytes,
                         int64_t instance_capacity, unsigned flags, void *stream, const GsrViewExt *ext,
                         float *dL_dviewmatrix, float *dL_dprojmatrix, float *dL_dcampos, void *scratch, size_t scratch_bytes,
                         const GsrAbsGrad *abs);

/* Depth-distortion map (opt-in; the distortion term of Mip-NeRF 360 / 2DGS, gsplat's distloss).  Per pixel p, over the splats blended into the image at
 * p in list order (front to back; w_i = alpha_i T_i, z_i the view-space depth of the splat record, background 0):
 *   distortion[p] = sum_i sum_j w_i w_j |z_i - z_j| = 2 sum_i w_i (z_i A_<i - D_<i),   A_<i = sum_{j<i} w_j,  D_<i = sum_{j<i} w_j z_j
 * (the two forms agree because the list is ordered by the same fp32 depth).  Depths are RAW view-space units, not normalised -- like the depth map; the
 * value does not change under a shift of z and is accumulated relative to the depth of the bin list's first entry.  It uses the image's own splats,
 * sort order and power > 0 / alpha < 1/255 / T < 1e-4 decisions; an overflowed view and a view without Gaussians give zeros.
 * Backward, with g = dL/ddistortion[p] and A_>i, D_>i the sums behind i:  d dist / d w_i = 2 [z_i (A_<i - A_>i) - D_<i + D_>i] enters the compositing
 * backward's scalar recurrence like one more colour channel (so dL/dopacity, dL/dmeans2D, the conic and through it scales / rotations / cov3D follow),
 * and d dist / d z_i = 2 w_i (A_<i - A_>i) joins the depth map's dL/dz, which reaches dL_dmeans3D through viewmatrix[:, 2] and, with them asked for,
 * the camera gradients.  With an exact depth tie the pairwise form has a kink; the list-order form's one-sided derivative is what is returned.
 * `totals` [2, H, W] is caller-owned scratch the forward writes (per pixel sum w and sum w (z - z0)) and the matching backward reads: hand the same
 * plane to both.  Made by the VALU compositing family, like the depth / alpha maps: the tiles flag is ignored for a view that asks for the map, in the
 * forward and the backward.  No atomics; the same bits on every run; no host synchronisation.
 * A NULL struct or a NULL map pointer IS gsr_forward_ex resp. gsr_backward_camera, bit for bit.  GPSGS_E_INVALID for a pointer that is not 4-byte
 * aligned, a non-NULL `reserved` or a map pointer without `totals`; GPSGS_E_WORKSPACE unless the workspace has the depth / alpha size
 * (gsr_workspace_bytes_depth_alpha with the call's forward_only: the backward needs forward_only = 0) -- there is no new tail and no new size function.
 * Combines with the depth / alpha maps and their gradients, antialiasing, camera gradients, shs, cov3D_precomp, row ranges, both list forms and
 * GSR_FLAG_NO_COLOR_GRAD; not with feature maps, statistics or absgrad (there is no entry point taking two option structs). */
typedef struct GsrDistort {
    union {
        float *out_distort;       /* forward: DEVICE [H, W], written; NULL = not wanted */
        const float *dL_ddistort; /* backward: DEVICE [H, W], read; NULL = not wanted */
    };
    float *totals;     /* DEVICE [2, H, W]: written by the forward, read by the backward */
    void *reserved[2]; /* NULL */
} GsrDistort;
/* gsr_forward_ex's argument list, then the GsrDistort */
int gsr_forward_distort(int P, int width, int height, const float *means3D, const float *colors, const float *opacities,
                        const float *scales, const float *rotations, float scale_modifier, float tanfovx, float tanfovy,
                        const float *viewmatrix, const float *projmatrix, const float *bg, float *out_color, int *radii,
                        void *workspace, size_t workspace_bytes, int64_t instance_capacity, unsigned flags, void *stream,
                        void *host_header_out, uint32_t notify_seq, const GsrViewExt *ext, const GsrDistort *distort);
/* gsr_backward_camera's argument list, then the GsrDistort */
int gsr_backward_distort(int P, int width, int height, const float *means3D, const float *colors, const float *opacities,
                         const float *scales, const float *rotations, float scale_modifier, float tanfovx, float tanfovy,
                         const float *viewmatrix, const float *projmatrix, const float *bg, const int *radii,
                         const float *dL_dpix, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dcolors, float *dL_dopacity,
                         float *dL_dscales, float *dL_drotations, void *workspace, size_t workspace_bytes,
                         int64_t instance_capacity, unsigned flags, void *stream, const GsrViewExt *ext,
                         float *dL_dviewmatrix, float *dL_dprojmatrix, float *dL_dcampos, void *scratch, size_t scratch_bytes,
                         const GsrDistort *distort);

/* Visibility mask (upstream `_C.mark_visible`, reached through GaussianRasterizer.markVisible(positions) of the module the reference imports at
 * gaussian_renderer/__init__.py:14; the reference itself never calls it): present[i] = 1 iff point i passes the near-plane test of the forward
 * (view-space z > 0.2), else 0.  means3D[P,3], viewmatrix[16] / projmatrix[16] as for gsr_forward (projmatrix is accepted for signature parity and
 * not read: upstream's in_frustum() tests the view-space depth only). */
int gsr_mark_visible(int P, const float *means3D, const float *viewmatrix, const float *projmatrix, uint8_t *present, void *stream);

/* Enqueues a copy of the first 32 header bytes {u64 num_rendered, u32 overflow, max_bin_count, num_busy, num_slots, 2 pad} to PINNED host memory on
 * `stream`; does not synchronise (the host reads it after an event / stream sync of its own). */
int gsr_copy_header_async(const void *workspace, void *host_pinned_out, void *stream);

/* Blocking helper for non-torch hosts: copies the header to host memory and synchronises `stream`. */
int gsr_read_header(const void *workspace, GsrHeader *host_out, void *stream);

/* Diagnostic: runs the matrix-core building blocks of the tile compositing kernels (coefficient split, operand arrangement, bf16
 * MFMA tiles, lane exchange) on pseudo-random splats against the quadratic form evaluated per lane in fp64.  out4 (device): {max
 * |error| / (1 + |value|) over 64 splats x 64 pixels, the same over pairs that can pass the alpha test, 1 if v_permlane32_swap behaves
 * as documented else 0, the largest |c0| met}. */
int gsr_selftest(float *out4_device, void *stream);

/* Diagnostic: after a gsr_backward on a training workspace, out2_device[0] = gradient-record slots that hold a record (one per (Gaussian, bin) instance
 * that received gradient), out2_device[1] = slots of the view (header.num_slots).  Enqueues a 16-byte memset + one kernel; does not synchronise. */
int gsr_debug_count_records(const void *workspace, size_t workspace_bytes, int P, int width, int height, int64_t instance_capacity, uint32_t bin_capacity,
                            unsigned long long *out2_device, void *stream); /* GPSGS_E_WORKSPACE for a forward-only workspace (it has no record slots) */

/* Profiling helper (not thread safe, not for use under graph capture): synchronises, then adds up the hipEvent
 * durations recorded by calls that carried GSR_FLAG_TIMING since the last read.  ms_sum[GSR_STAGE_COUNT] receives the
 * total milliseconds per stage, launches[GSR_STAGE_COUNT] the number of timed launches.  Resets the recorder. */
int gsr_timing_read(float *ms_sum_host, int *launches_host);

/* Debug/parity helper: copies selected intermediate arrays out of the workspace into caller DEVICE buffers (any may
 * be NULL): depth[P], xy[P,2], conic_opacity[P,4], rect[P,4] (int32 bx0,by0,bx1,by1: the 8x8-pixel BIN rect the Gaussian
 * is listed in), tile_ranges[NB,2] (int64 list range per bin; NB = (ceil(W/8) rounded up to 4) * ceil(H/8)),
 * point_list[instance_capacity, or NB * bin_capacity with direct lists: indexed by tile_ranges] (uint32, sorted per bin), final_T[H,W], n_contrib[H,W] (the last two are only produced by a
 * forward on a workspace with the backward tail). */
int gsr_export_state(const void *workspace, int P, int width, int height, int64_t instance_capacity, uint32_t bin_capacity, float *depth,
                     float *xy, float *conic_opacity, int *rect, int64_t *tile_ranges, uint32_t *point_list,
                     float *final_T, uint32_t *n_contrib, void *stream);

/* ---- fused mask-compaction + pack of the per-pixel Gaussian maps (lib/GaussianRender.py:15-34) -------------------------
 * For every batch element b and view v (lmain, rmain): the pixels with valid != 0, in raster order, become consecutive
 * rows; row order is sample, then view, then pixel -- exactly the order of the reference's mask-gathers + concats.
 * rgb rows are img * 0.5 + 0.5.  All inputs are described with ELEMENT strides so that permuted views (the reference's xyz
 * is one) need no copy: element (b, pixel, channel) = ptr[b*batch_stride + pixel*pixel_stride + channel*channel_stride].
 * Outputs: packed rows out_xyz[rows,3], out_rgb[rows,3], out_rot[rows,4], out_scale[rows,3], out_opacity[rows] with capacity
 * B*n_views*S2 rows; row_of_pixel[B,n_views,S2] (row index or ~0; kept for the backward); sample_offsets[B+1] (device):
 * sample b owns rows [sample_offsets[b], sample_offsets[b+1]).  No host synchronisation. */
typedef struct GsrStrided {
    const void *ptr;
    int64_t batch_stride, pixel_stride, channel_stride;
} GsrStrided;

size_t gsr_pack_scratch_bytes(int B, int n_views, int S2);
int gsr_pack_views(int B, int n_views, int S2, const GsrStrided *valid /*u8*/, const GsrStrided *xyz, const GsrStrided *img,
                   const GsrStrided *rot, const GsrStrided *scale, const GsrStrided *opacity /* host arrays [n_views] */,
                   float *out_xyz, float *out_rgb, float *out_rot, float *out_scale, float *out_opacity, uint32_t *row_of_pixel,
                   uint32_t *sample_offsets, uint32_t *scratch, void *stream);
/* Backward: packed row gradients (any may be NULL = zero) -> planar map gradients, contiguous: d_xyz[v] is [B,S2,3], the
 * others [B,C,S2]; host arrays of n_views device pointers, entries / arrays may be NULL (not wanted).  Invalid pixels get 0. */
int gsr_pack_views_backward(int B, int n_views, int S2, const uint32_t *row_of_pixel, const float *g_xyz, const float *g_rgb,
                            const float *g_rot, const float *g_scale, const float *g_opacity, float *const *d_xyz,
                            float *const *d_img, float *const *d_rot, float *const *d_scale, float *const *d_opacity, void *stream);

/* ---- Gaussian-parameter heads: ReLU -> 1x1 convolution -> activation in one pass (lib/gs_parm_network.py:34-50) -------------------------
 * y[n,k,p] = act( bias[k] + sum_c w[k,c] * max(h[n,c,p], 0) ),  h [N,C_in,H,W] and y [N,C_out,H,W] contiguous NCHW, w [C_out,C_in] (a 1x1
 * convolution's weight as it lies), p over the H*W pixels of a plane; everything fp32.  z = bias, then fmaf over c in index order.
 * act: 0 = none; 1 = softplus(beta, threshold) with torch's definition, z where beta*z > threshold, else log1p(exp(beta*z)) / beta; 2 = sigmoid.
 * beta and threshold are read for act 1 only.
 * gsr_head_supported: 1 for C_in in {16, 32, 64}, 1 <= C_out <= 4 and act in {0, 1, 2}; otherwise 0.
 * gsr_head_tile: the pixels of one sample one workgroup covers (in both directions; the weight gradient has one partial per workgroup).
 * Any H, W >= 1: where H*W is a multiple of 4 and h, y (backward: h, dy, dh) are 16-byte aligned the kernels move 16 bytes per access, otherwise
 * (plane bases then lie off 16-byte boundaries) 4; 4-byte alignment is all that is required.
 * gsr_head_backward takes dy, the gradient of y, and WRITES dh (NULL = not wanted: nothing is computed for it) and dw [C_out,C_in] / dbias
 * [C_out] (both or neither; NULL = not wanted):
 *     dz = dy * act'(z)      dh[n,c,p] = (h > 0) * sum_k w[k,c] dz_k  (zero at h == 0)      dw[k,c] = sum_{n,p} dz_k max(h_c, 0)      dbias[k] = sum dz_k
 * z is recomputed from h with the forward's arithmetic; `y` (the forward's output) is NOT read and may be NULL -- the argument is kept so that a
 * variant that takes act' from y needs no new entry point.  One launch reads h and dy once for both dh and the sums.  dw and dbias are two-stage
 * sums: per workgroup, then over the workgroups in index order (in groups of 64, then the groups) -- no atomics, the same bits on every run.
 * scratch (needed for dw / dbias only): DEVICE, at least gsr_head_scratch_bytes(...) =
 *     4 * C_out * (C_in + 1) * (parts + ceil(parts / 64))   bytes,  parts = N * ceil(H*W / gsr_head_tile())
 * and 0 for arguments the other entry points would refuse (the activation is not among its arguments).
 * Scratch layout after a backward with dw, here and for sc_backward and c3_backward below (M = the elements of dw plus those of dbias, G = the group
 * size, 64 / 64 / 32): the partials as fp32 [parts][M], each row a workgroup's dw sums followed by its dbias sums; then, where parts > G, the group
 * sums [ceil(parts / G)][M], row g the sum of partials g*G .. min(parts, (g+1)*G) - 1.  Every sum starts from 0 and adds in index order; dw, dbias
 * are the sum of the group sums (of the partials where parts <= G) in the same way.
 * GPSGS_E_INVALID, before any HIP call: a (C_in, C_out, act) gsr_head_supported refuses, a non-positive N, H or W, beta <= 0 (or NaN) with act 1,
 * a NULL required pointer (h, w, bias, y; h, w, bias, dy, and scratch where dw is wanted) or one off a 4-byte boundary, one of dw / dbias without
 * the other, H*W > INT_MAX - gsr_head_tile() (a pixel index inside a plane is an int; offsets into the tensors are 64-bit, so N*C*H*W has no limit
 * of its own) and N * ceil(H*W / tile) > INT_MAX (a grid's width).  A backward that wants neither dh nor dw returns GPSGS_OK and launches nothing. */
int gsr_head_supported(int C_in, int C_out, int act);
int gsr_head_tile(void);
size_t gsr_head_scratch_bytes(int N, int C_in, int C_out, int H, int W);
int gsr_head_forward(const float *h, const float *w, const float *bias, int N, int C_in, int C_out, int H, int W, int act, float beta,
                     float threshold, float *y, void *stream);
int gsr_head_backward(const float *h, const float *w, const float *bias, const float *y, const float *dy, int N, int C_in, int C_out, int H, int W,
                      int act, float beta, float threshold, float *dh, float *dw, float *dbias, void *scratch, void *stream);

/* ---- fused L1 + SSIM loss (lib/loss.py:36-83 as used at train_stage2.py:70-72) ------------------------------------------
 * pred, gt: contiguous fp32 [planes = B*C, H, W].  out2 (device) = {mean |pred - gt|, mean SSIM map} (11x11 Gaussian window,
 * sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2).  m1,m2,m3 [planes,H,W]: derivative maps kept for the backward (all three
 * or none).  scratch: fl_scratch_bytes().  Backward: grad_out2 (device) = {dL/d(mean L1), dL/d(mean SSIM)}; writes d_pred.
 * One workgroup per 32x32 tile, grid = (column tiles, row tiles, planes): GPSGS_E_INVALID for planes > 65535, more than 65535 row tiles,
 * W > INT_MAX - 31, or a tile count planes x row tiles x column tiles above INT_MAX -- as for a negative size, a NULL pointer, m1 / m2 / m3 given in part and
 * (forward only: a mean over nothing) an empty tensor; the backward of an empty tensor returns GPSGS_OK and launches nothing. */
size_t fl_scratch_bytes(int planes, int H, int W);
int fl_l1_ssim_forward(const float *pred, const float *gt, int planes, int H, int W, float *m1, float *m2, float *m3, void *scratch,
                       float *out2, void *stream);
int fl_l1_ssim_backward(const float *pred, const float *gt, const float *m1, const float *m2, const float *m3, int planes, int H, int W,
                        const float *grad_out2, float *d_pred, void *stream);

/* ---- fused disparity -> inverse depth -> world points (lib/utils.py:88-120, lib/network.py:66-69) ---------------------
 * flow [B,1,S,S], mask channel 0 of [B,C,S,S] (mask_batch_stride = C*S*S elements), camera parameters on the HOST:
 * ref_intr/intr [B,3,3], extr [B,3,4] row-major, Tf_x [B] (any B: launched 16 samples at a time).  Outputs depth [B,1,S,S] (inverse depth), xyz [B,S*S,3],
 * valid [B,S*S] (u8).  Backward: g_depth [B,1,S,S] and/or g_xyz (element strides given; either may be NULL) -> d_flow. */
int up_unproject_forward(int B, int S, const float *flow, const float *mask, int64_t mask_batch_stride, const float *ref_intr_host,
                         const float *intr_host, const float *extr_host, const float *tf_host, float *depth, float *xyz,
                         uint8_t *valid, void *stream);
int up_unproject_backward(int B, int S, const float *depth, const float *mask, int64_t mask_batch_stride, const float *ref_intr_host,
                          const float *intr_host, const float *extr_host, const float *tf_host, const float *g_depth,
                          const float *g_xyz, int64_t gx_batch_stride, int64_t gx_pixel_stride, int64_t gx_channel_stride,
                          float *d_flow, void *stream);
/* The same with the cameras in DEVICE memory, cams_dev[B][31] = {ref_intr 3x3, intr 3x3, rows 0..2 of extr (3x4, row-major), Tf_x} per sample: nothing is
 * read on the host (the reference keeps these tensors on the GPU, train_stage2.py:154-156; reading them back would synchronise in the middle of the network
 * forward), one launch for any B, bit-identical results. */
int up_unproject_forward_dev(int B, int S, const float *flow, const float *mask, int64_t mask_batch_stride, const float *cams_dev, float *depth, float *xyz,
                             uint8_t *valid, void *stream);
int up_unproject_backward_dev(int B, int S, const float *depth, const float *mask, int64_t mask_batch_stride, const float *cams_dev, const float *g_depth,
                              const float *g_xyz, int64_t gx_batch_stride, int64_t gx_pixel_stride, int64_t gx_channel_stride, float *d_flow, void *stream);

/* ---- z-buffer point splat (the stage-1 validation render, lib/TaichiRender.py) ---------------------------------------------------------
 * Per target pixel the result of running the points in sequence (view 0 in index order, then view 1, ...) with
 * `if z >= depth[px]: depth[px] = z; colour[px] = rgb`, px = clamp(trunc(x|y), 0, res-1) with saturating truncation (NaN -> 0); points with
 * mask < 0.5 or NaN z are skipped.  Deterministic (the reference's separate colour write races); every view and sample in one scatter launch.
 * Device scratch: up_splat_scratch_bytes(B, res) (one 64-bit key per target pixel).  V * N + 1 must fit in 32 bits.
 * up_zsplat: render_respective_color; pts [V][B][N][6] = (x, y, z, r, g, b), mask [V][B][N]; depth [B][res][res] and color [B][3][res][res]
 *   are updated IN PLACE.
 * up_flow2render_dev: TaichiRenderBatch.flow2render fused -- per source pixel of the two views (l = lmain, r = rmain): flow2depth, valid =
 *   depth != 0, depth2pc (the bits of up_unproject_forward_dev), perspective into the novel view with calib = intr @ extr, z <- 1 / (z + 1e-8),
 *   then the splat; colours straight from img_l / img_r [B][3][S][S].  flow [B][S][S], mask [B][..] with mask_batch_stride; cams_dev[2][B][31] as
 *   up_unproject_forward_dev's (all of lmain, then all of rmain); novel_dev[B][21] = {intr 3x3, extr rows 0..2 (3x4)}: nothing is read on the
 *   host.  Writes all of img_pred [B][3][res][res] (-1 where no point lands).  pts_out (optional, NULL in normal use) [2][B][S*S][3]: each
 *   point's projected (x, y, 1/z), NaN for invalid points. */
size_t up_splat_scratch_bytes(int B, int res);
int up_zsplat(int V, int B, int N, int res, const float *pts, const float *mask, float *depth, float *color, void *scratch, size_t scratch_bytes,
              void *stream);
int up_flow2render_dev(int B, int S, int res, const float *flow_l, const float *flow_r, const float *mask_l, const float *mask_r,
                       int64_t mask_batch_stride, const float *img_l, const float *img_r, const float *cams_dev, const float *novel_dev, void *scratch,
                       size_t scratch_bytes, float *img_pred, float *pts_out, void *stream);

/* ---- 1-D correlation sampler ----------------------------------------------------------------------------------
 * volume[N,H1,W1,W2], coords[N,H1,W1] fp32 (channel 0 of the reference's [N,1,H1,W1]), out[N,2r+1,H1,W1].
 * dtype: 0 = fp32, 1 = fp16 (volume / out / grads; coords always fp32).
 * out[n,k,y,x] = sum_j volume[n,y,x,j] * max(0, 1 - |coords[n,y,x] - radius + k - j|): linear interpolation, zero outside the row; any radius >= 0,
 * the window may be wider than the row.  The backward writes every element of grad_volume (zero fill fused; no gradient to coords).
 * Coordinate range: finite, |c| + radius + 1 < 2^31.  Outside it (NaN, infinities, farther away) no access leaves the tensors, but the values
 * written are unspecified.
 * Empty tensors (N*H1*W1 == 0, for the backward also W2 == 0) return GPSGS_OK, launch nothing and may come with NULL pointers.  GPSGS_E_INVALID:
 * a negative size, a dtype other than 0 / 1, a NULL pointer of a non-empty tensor, radius < 0 or 2*radius + 1 > INT_MAX, N*H1*W1 > INT_MAX
 * (forward and backward: the kernels index the rows in int), and a backward whose block count exceeds 0x7fffffff -- one thread per four elements
 * of grad_volume where W2 % 4 == 0 and grad_volume is 16-byte aligned, else one per element, in blocks of 256.  cs_lookup_forward /
 * cs_lookup_backward below refuse the same (their backward runs one thread per level-0 element), levels outside 1..4, and a NULL level pointer
 * except where W2 >> l == 0. */
int cs_forward(const void *volume, const float *coords, void *out, int N, int H1, int W1, int W2, int radius,
               int dtype, void *stream);
int cs_backward(const float *coords, const void *grad_out, void *grad_volume, int N, int H1, int W1, int W2,
                int radius, int dtype, void *stream);

/* ---- correlation volume + pyramid, fused multi-level lookup, convex upsampling ----------
 * fmap1[N,D,H,W1], fmap2[N,D,H,W2] (contiguous NCHW, the reference's fmap12 / fmap21); pyramid[l] is [N,H,W1,W2>>l] for
 * l < levels (1..4), a HOST array of device pointers.  level 0 = sum_d fmap1 fmap2 / sqrt(D); level l+1 = average of
 * neighbouring pairs of level l along W2 (avg_pool2d([1,2], stride [1,2]): an odd last column is dropped).
 * dtype 0 = fp32, 1 = fp16 (inputs, pyramid and gradients; accumulation is always fp32, one rounding on store). */
int cv_build_forward(const void *fmap1, const void *fmap2, void *const *pyramid, int N, int D, int H, int W1, int W2, int levels,
                     int dtype, void *stream);
/* grad_pyramid[l] may be NULL (level received no gradient); grad_fmap1 / grad_fmap2 may be NULL (not needed); both are
 * written, not accumulated. */
int cv_build_backward(const void *fmap1, const void *fmap2, const void *const *grad_pyramid, void *grad_fmap1, void *grad_fmap2, int N,
                      int D, int H, int W1, int W2, int levels, int dtype, void *stream);
/* out[N, levels*(2r+1), H1, W1]: channel l*(2r+1)+k = tap k of level l sampled at coords / 2^l (cs_forward semantics per level). */
int cs_lookup_forward(const void *const *pyramid, const float *coords, void *out, int N, int H1, int W1, int W2, int levels, int radius,
                      int dtype, void *stream);
/* writes (zero-fills + taps) every grad_pyramid[l][N,H1,W1,W2>>l] */
int cs_lookup_backward(const float *coords, const void *grad_out, void *const *grad_pyramid, int N, int H1, int W1, int W2, int levels,
                       int radius, int dtype, void *stream);
/* flow[N,C,H,W] (C <= 4 forward, <= 2 backward: the reference upsamples a 2-channel flow), mask[N,9*f*f,H,W] logits,
 * out[N,C,f*H,f*W]; fp32.  The backward needs cu_upsample_scratch_bytes() of device scratch when grad_flow is requested
 * (per coarse cell and tap: the sums of softmax weight x upstream gradient); grad_flow / grad_mask may each be NULL, not both.
 * factor in 1..16.  Empty tensors return GPSGS_OK and launch nothing.  GPSGS_E_INVALID where a launch could not hold the work: the forward runs
 * one thread per output pixel N*f*H*f*W and the flow gradient one per flow element N*C*H*W, in blocks of 256, and a block count above 0x7fffffff
 * is refused, as are f*H > INT_MAX and f*W > INT_MAX - 63; the backward also needs N <= 65535 and H <= 65535 (grid z and y). */
int cu_upsample_forward(const float *flow, const float *mask, float *out, int N, int C, int H, int W, int factor, void *stream);
size_t cu_upsample_scratch_bytes(int N, int C, int H, int W);
int cu_upsample_backward(const float *flow, const float *mask, const float *grad_out, float *grad_flow, float *grad_mask, void *scratch,
                         int N, int C, int H, int W, int factor, void *stream);

/* ---- GroupNorm, forward and backward, every row split over the chip ------------------------------------------------------------
 * x[N,C,HW] contiguous (NCHW with HW = H*W), G groups of C/G channels: y = (x - mean) * rstd * gamma[c] + beta[c] with mean / biased variance over
 * the L = (C/G)*HW elements of a (sample, group) ROW, rstd = 1/sqrt(var + eps)  (torch.nn.functional.group_norm).
 * dtype (as cs_forward): 0 = x and dx fp32, 1 = x and dx fp16; y, dy, gamma[C], beta[C], mean[N,G], rstd[N,G], dgamma[C], dbeta[C] are always fp32
 * and every sum is fp32; dx is rounded once, on store.  x, y, dy and dx must be 16-byte aligned (GPSGS_E_INVALID otherwise).
 * Rows (forward) and (sample, channel) planes (backward) are cut into chunks of gn_chunk_elems() elements, one workgroup each; per-chunk partials
 * ({mean, M2}, so a mean far larger than the spread is harmless; {sum dy, sum dy (x - mean)} in the backward) go to `scratch` and are combined in a
 * fixed order: no atomics, the same bits on every run.
 * scratch: DEVICE, 8-byte aligned, at least gn_scratch_bytes(N, C, G, HW) =
 *     8 * N * (C + max(ceil(C*HW / chunk) + G, C * ceil(HW / chunk)))   bytes, chunk = gn_chunk_elems()
 * -- N*C plane sums, then G * ceil(L / chunk) <= ceil(C*HW / chunk) + G partials per sample (forward) or ceil(HW / chunk) per plane (backward);
 * forward and backward share the formula, the backward does not need the forward's contents.  0 for a negative size or G <= 0.
 * gn_forward writes y, mean, rstd.  gn_backward reads x, dy, gamma, mean, rstd (never y: the consumer may have overwritten it in place) and WRITES
 * dx (x's dtype; NULL = not wanted) and dgamma / dbeta (both or neither; NULL = not wanted).
 * GPSGS_E_INVALID, before any HIP call: a negative size, G <= 0, C % G != 0, an unknown dtype, one of dgamma / dbeta without the other, a row of
 * 2^31 elements or more, and -- unless N*C*HW == 0, which returns 0 and launches nothing -- a NULL required pointer or a misaligned one. */
size_t gn_chunk_elems(void);
size_t gn_scratch_bytes(int N, int C, int G, int HW);
int gn_forward(const void *x, int dtype, const float *gamma, const float *beta, int N, int C, int G, int HW, float eps, float *y, float *mean,
               float *rstd, void *scratch, void *stream);
int gn_backward(const void *x, int dtype, const float *dy, const float *gamma, const float *mean, const float *rstd, int N, int C, int G, int HW,
                void *dx, float *dgamma, float *dbeta, void *scratch, void *stream);
/* The same two passes with an epilogue fused in (no further kernel, no further pass over y):
 *     residual == NULL:  out = relu(y)                    residual != NULL:  out = relu(residual + relu(y)),  residual fp32 [N,C,HW]
 * out is bit for bit what relu_ / add / relu applied to gn_forward's y give.  gne_backward takes dout, the gradient of out:
 *     g = dout where out > 0, else +0 (residual form only; `out` non-NULL selects it and must be gne_forward's output)      dres = g
 *     dy = g where y > 0, else +0 -- the sign of y is recomputed from x, mean, rstd, gamma, beta with the forward's arithmetic, so no normalised
 *     activation has to be kept; the plain form needs x, mean, rstd only
 * and then does what gn_backward does with dy, in the same two kernels: dx, dgamma, dbeta are bit for bit gn_backward's on that dy.  dres (fp32
 * [N,C,HW]; NULL = not wanted) needs `out`.  Scratch, alignment (also of residual, out, dout, dres), the empty-tensor rule and the refusals are
 * gn_forward's / gn_backward's; in addition GPSGS_E_INVALID for dres without out, and beta is a required pointer of the backward too. */
int gne_forward(const void *x, int dtype, const float *gamma, const float *beta, const float *residual, int N, int C, int G, int HW, float eps,
                float *out, float *mean, float *rstd, void *scratch, void *stream);
int gne_backward(const void *x, int dtype, const float *dout, const float *out, const float *gamma, const float *beta, const float *mean,
                 const float *rstd, int N, int C, int G, int HW, void *dx, float *dres, float *dgamma, float *dbeta, void *scratch, void *stream);

/* ---- Stem convolution: direct 2-D convolution for layers with almost no input channels, forward and backward ----------------------
 * y[N,C_out,Ho,Wo] = conv2d(x[N,C_in,H,W], w[C_out,C_in,K,K], bias[C_out], stride, padding = pad), zero padding, dilation 1, groups 1, contiguous
 * NCHW, Ho = (H + 2 pad - K) / stride + 1 (floored), Wo likewise  (torch.nn.functional.conv2d).
 * sc_supported: 1 for (C_in, K, stride, pad) in {(1, 5, 2, 2), (3, 5, 2, 2)} with C_out a multiple of 8, 8 <= C_out <= 64; otherwise 0.
 * sc_tile: the output tile (rows, columns) one workgroup of the forward and of the weight gradient computes.
 * x, w, bias, dx, dw, dbias are fp32.  y_dtype / dy_dtype: 0 = fp32, 1 = fp16 (what fp16 autocast makes of this layer's output and its gradient);
 * every sum is fp32, y is rounded once, on store: acc = bias, then fmaf over (ci, ky, kx) in index order.  x, y, dy, dx and scratch must be
 * 16-byte aligned; rows of any width, also ones that start off a 16-byte boundary, are fine.  H, W, Ho, Wo may be anything >= 1.
 * sc_backward WRITES dx (NULL = not wanted: that kernel is not launched) and dw / dbias (both or neither; NULL = not wanted).  dw and dbias are
 * two-stage sums: per tile, then over the tiles in index order (in groups of 64, then the groups) -- no atomics, the same bits on every run.
 * scratch (needed for dw / dbias only): DEVICE, at least sc_scratch_bytes(...) =
 *     4 * C_out * (C_in * K * K + 1) * (tiles + ceil(tiles / 64))   bytes,  tiles = N * ceil(Ho / tile_h) * ceil(Wo / tile_w)
 * and 0 for arguments sc_forward would refuse (layout: the partials, then the group sums, as under gsr_head_scratch_bytes).
 * GPSGS_E_INVALID, before any HIP call: a configuration sc_supported refuses, a non-positive N, H or W, a dtype outside {0, 1}, 2^31 elements or
 * more in x or in y, one of dw / dbias without the other, a NULL required pointer (x, w, bias, y; x, w, dy, and scratch where dw is wanted) or a
 * misaligned one. */
int sc_supported(int C_in, int C_out, int K, int stride, int pad);
int sc_tile(int *tile_h, int *tile_w);
size_t sc_scratch_bytes(int N, int C_in, int C_out, int H, int W, int K, int stride, int pad);
int sc_forward(const float *x, const float *w, const float *bias, int N, int C_in, int C_out, int H, int W, int K, int stride, int pad, void *y,
               int y_dtype, void *stream);
int sc_backward(const float *x, const float *w, const void *dy, int dy_dtype, int N, int C_in, int C_out, int H, int W, int K, int stride, int pad,
                float *dx, float *dw, float *dbias, void *scratch, void *stream);

/* ---- 3x3 convolution to 32 channels on the fp32 matrix cores, forward and backward ---------------------------------------------------
 * y[N,32,H,W] = conv2d(x[N,C_in,H,W], w[32,C_in,3,3], bias[32], stride 1, padding 1), zero padding, contiguous NCHW fp32, followed by ReLU where
 * relu = 1  (torch.nn.functional.conv2d + relu).  Implicit GEMM on v_mfma_f32_32x32x2_f32: exact fp32, every sum an fmaf chain in a fixed order
 * (the products first, the bias added last), no layout transposes, no atomics, the same bits on every run.
 * c3_supported: 1 for C_out == 32 and C_in a multiple of 4 with 4 <= C_in <= 64; otherwise 0.
 * c3_tile: the output tile (rows, columns) one workgroup of the forward and of the input gradient computes.
 * x, y, dy, dx and scratch must be 16-byte aligned; H and W may be anything >= 1, rows may start off 16-byte boundaries.
 * c3_backward takes dy, the gradient of y; relu = 1: g = dy where y > 0, else 0, with y the forward's output (required then; ignored and may be
 * NULL for relu = 0).  It WRITES dx = conv(g, w flipped and transposed) (NULL = not wanted: that kernel is not launched) and dw / dbias (both or
 * neither; NULL = not wanted).  dw and dbias are sums over pixels: at most 512 workgroups each walk a fixed, index-ordered set of 4 x 32 pixel
 * tiles and write one partial; the partials are added in index order, in groups of 32 and then the groups.
 * scratch (needed for dw / dbias only): DEVICE, at least c3_scratch_bytes(N, C_in, H, W) =
 *     4 * 32 * (9 * C_in + 1) * (parts + ceil(parts / 32))   bytes,  parts = min(512, N * ceil(H / 4) * ceil(W / 32))
 * and 0 for arguments c3_forward would refuse (layout: the partials, then the group sums, as under gsr_head_scratch_bytes).
 * GPSGS_E_INVALID, before any HIP call: channel counts c3_supported refuses, a non-positive N, H or W, relu outside {0, 1}, 2^31 elements or more
 * in x or in y, one of dw / dbias without the other, a NULL required pointer (x, w, bias, y; x, w, dy, y where relu = 1, and scratch where dw is
 * wanted) or a misaligned one. */
int c3_supported(int C_in, int C_out);
int c3_tile(int *tile_h, int *tile_w);
size_t c3_scratch_bytes(int N, int C_in, int H, int W);
int c3_forward(const float *x, const float *w, const float *bias, int N, int C_in, int H, int W, int relu, float *y, void *stream);
int c3_backward(const float *x, const float *w, const float *y, const float *dy, int N, int C_in, int H, int W, int relu, float *dx, float *dw,
                float *dbias, void *scratch, void *stream);

/* ---- 1x1 convolution with stride 1 or 2 on the fp32 matrix cores, forward and backward -----------------------------------------------------
 * y[N,C_out,Ho,Wo] = conv2d(x[N,C_in,H,W], w[C_out,C_in,1,1], bias[C_out], stride, padding 0), Ho = (H - 1) / stride + 1, Wo likewise, contiguous
 * NCHW fp32 (torch.nn.functional.conv2d): y[n,co,i,j] = bias[co] + sum over ci of w[co,ci] x[n,ci,stride i,stride j].  One GEMM per image on
 * v_mfma_f32_32x32x2_f32: exact fp32, every sum an fmaf chain in a fixed order (the products in channel order first, the bias added last), no
 * layout transposes, no intermediate tensor, no atomics, the same bits on every run.
 * c1_supported: 1 for C_in a multiple of 4 with 4 <= C_in <= 256, C_out a multiple of 16 with 16 <= C_out <= 128 and stride 1 or 2; otherwise 0.
 * c1_tile: the consecutive output pixels of one image a workgroup of the forward (and of the input gradient) computes, the pixels of one tile of
 * the weight gradient, and the largest number of partials the weight gradient writes.
 * x, y, dy, dx and scratch must be 16-byte aligned; H and W may be anything >= 1.
 * c1_backward takes dy, the gradient of y.  It WRITES ALL of dx (NULL = not wanted: that kernel is not launched): dx[n,ci,stride i,stride j] = sum
 * over co of w[co,ci] dy[n,co,i,j] and, for stride 2, +0.0 at every position the forward did not sample -- nothing has to be cleared in front --
 * and dw / dbias (both or neither; NULL = not wanted).  dw and dbias are sums over pixels: at most 512 workgroups each walk a fixed, index-ordered
 * set of 32-pixel tiles and write one partial; the partials are added in index order, in groups of 32 and then the groups.
 * scratch (needed for dw / dbias only): DEVICE, at least c1_scratch_bytes(N, C_in, C_out, H, W, stride) =
 *     4 * C_out * (C_in + 1) * (parts + ceil(parts / 32))   bytes,  parts = min(512, N * ceil(Ho * Wo / 32))
 * and 0 for arguments c1_forward would refuse (layout: the partials, then the group sums, as under gsr_head_scratch_bytes).
 * GPSGS_E_INVALID, before any HIP call: a configuration c1_supported refuses, a non-positive N, H or W, 2^31 elements or more in x or in y, one of
 * dw / dbias without the other, a NULL required pointer (x, w, bias, y; x, w, dy, and scratch where dw is wanted) or a misaligned one. */
int c1_supported(int C_in, int C_out, int stride);
int c1_tile(int *forward_pixels, int *weight_pixels, int *max_parts);
size_t c1_scratch_bytes(int N, int C_in, int C_out, int H, int W, int stride);
int c1_forward(const float *x, const float *w, const float *bias, int N, int C_in, int C_out, int H, int W, int stride, float *y, void *stream);
int c1_backward(const float *x, const float *w, const float *dy, int N, int C_in, int C_out, int H, int W, int stride, float *dx, float *dw,
                float *dbias, void *scratch, void *stream);

/* ---- 3x3 convolution from C_in to C_out channels on the fp32 matrix cores, forward and backward (the residual blocks) ---------------------
 * y[N,C_out,H,W] = conv2d(x[N,C_in,H,W], w[C_out,C_in,3,3], bias[C_out], stride 1, padding 1), zero padding, contiguous NCHW fp32
 * (torch.nn.functional.conv2d).  Implicit GEMM on v_mfma_f32_32x32x2_f32: exact fp32, every sum an fmaf chain in a fixed order (the products in
 * channel order first, the bias added last), no layout transposes, no atomics, nothing cleared in front, the same bits on every run.
 * rc_supported: 1 for C_in a multiple of 4 with 4 <= C_in <= 192 and C_out a multiple of 16 with 16 <= C_out <= 96; otherwise 0.
 * rc_tile: the output tile (rows, columns) one workgroup of the forward and of the input gradient computes (for 32 output channels).
 * x, y, dy, dx and scratch must be 16-byte aligned; H and W may be anything >= 1, rows may start off 16-byte boundaries.
 * rc_backward takes dy, the gradient of y.  It WRITES dx = conv(dy, w flipped and transposed) (NULL = not wanted: that kernel is not launched)
 * and dw / dbias (both or neither; NULL = not wanted).  dw and dbias are sums over pixels: the 4 x 32 pixel tiles are dealt to `parts` partitions
 * (tile t to partition t mod parts); one workgroup per (partition, block of 32 output channels, block of 64 input channels) walks its partition's
 * tiles in index order and writes its block of that partition's partial; the partials are added in index order, in groups of 32 and then the groups.
 * scratch (needed for dw / dbias only): DEVICE, at least rc_scratch_bytes(N, C_in, C_out, H, W) =
 *     4 * C_out * (9 * C_in + 1) * (parts + ceil(parts / 32))   bytes,
 *     parts = min(512 / (ceil(C_out / 32) * ceil(C_in / 64)) rounded down, N * ceil(H / 4) * ceil(W / 32))
 * -- at most 39.0 MB for the supported widths -- and 0 for arguments rc_forward would refuse (layout: the partials, then the group sums, as under
 * gsr_head_scratch_bytes).
 * GPSGS_E_INVALID, before any HIP call: channel counts rc_supported refuses, a non-positive N, H or W, 2^31 elements or more in x or in y, one of
 * dw / dbias without the other, a NULL required pointer (x, w, bias, y; x, w, dy, and scratch where dw is wanted) or a misaligned one. */
int rc_supported(int C_in, int C_out);
int rc_tile(int *tile_h, int *tile_w);
size_t rc_scratch_bytes(int N, int C_in, int C_out, int H, int W);
int rc_forward(const float *x, const float *w, const float *bias, int N, int C_in, int C_out, int H, int W, float *y, void *stream);
int rc_backward(const float *x, const float *w, const float *dy, int N, int C_in, int C_out, int H, int W, float *dx, float *dw, float *dbias,
                void *scratch, void *stream);

/* ---- Decoder glue: bilinear 2x upsample + channel concatenation in one pass, forward and backward ------------------------------------------
 * out[N, Ca + C_0 + .. + C_{K-1}, 2h, 2w]: channels [0, Ca) are nn.Upsample(scale_factor=2, mode="bilinear") of a[N,Ca,h,w] (align_corners =
 * False), the K skip tensors s_k[N,C_k,2h,2w] follow in order, copied bit for bit (torch.cat along dim 1).  0 <= K <= 3; everything contiguous NCHW
 * fp32.  The upsample is separable with fixed taps per axis (n the axis' input length):
 *     o[2i] = 0.25 a[max(i - 1, 0)] + 0.75 a[i]        o[2i + 1] = 0.75 a[i] + 0.25 a[min(i + 1, n - 1)]
 * evaluated along x first, then along y, each tap pair as fmaf(0.75, near, 0.25 * far): exact fp32 in that order, two roundings on every path.
 * skips, skip_channels: HOST arrays of K device pointers / K channel counts (read before the call returns; NULL allowed where K = 0).
 * uc_supported: 1 for 0 <= K <= 3 with every channel count >= 1; otherwise 0.
 * uc_tile: the output tile (rows, columns) one workgroup of the forward's upsampled part computes.
 * Pointers need 4-byte alignment; with w even and out and every skip 16-byte aligned the forward stores and copies 16 bytes per lane.
 * uc_backward takes dout, the gradient of out, [N, Ca + sum C_k, 2h, 2w], and WRITES ALL of da[N,Ca,h,w] (NULL = not wanted: nothing is launched,
 * GPSGS_OK): da[i,j] = the sum over the taps of dout[:, :Ca] the forward scattered from a[i,j] -- rows 2i-1 .. 2i+2 and columns 2j-1 .. 2j+2, clamped
 * to the plane (the clamp is the border element's folded tap), weights 0.25, 0.75, 0.75, 0.25 per axis -- along x first, then along y, each as
 * fmaf(0.75, d1 + d2, 0.25 * (d0 + d3)).  A gather, one thread per element: no atomics, nothing to clear, the same bits on every run.  The skips'
 * gradients are the slices dout[:, c0_k : c0_k + C_k]; no kernel computes them.
 * GPSGS_E_INVALID, before any HIP call: a non-positive N, Ca, h or w, K outside 0..3, a skip channel count below 1 (or skip_channels NULL with
 * K > 0), 2^31 elements or more in any tensor, a NULL pointer (a, out, skips or one of its entries; dout) or one aligned to less than 4 bytes. */
int uc_supported(int K, const int *skip_channels);
int uc_tile(int *tile_h, int *tile_w);
int uc_forward(const float *a, const float *const *skips, const int *skip_channels, int K, int N, int Ca, int h, int w, float *out, void *stream);
int uc_backward(const float *dout, const int *skip_channels, int K, int N, int Ca, int h, int w, float *da, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GPSGS_H */
