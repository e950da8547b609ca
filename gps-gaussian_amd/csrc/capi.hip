// capi.hip -- extern "C" entry points of libgpsgs_hip.so (declared in include/gpsgs.h).
// Pure enqueue: no allocation, no host synchronisation (except in the explicit *_read_header helper and under
// GSR_FLAG_DEBUG), so a forward+backward pair can be captured into a hipGraph.
#include <stdio.h>
#include <stdlib.h>

#include <mutex>

#include "gsr_common.h"

namespace {

// GPSGS_TRACE=1 (environment): every rasteriser stage announces itself on stderr before its launch and is synchronised after it --
// a device fault then names the stage that was running (a GPU memory fault aborts the process; there is nothing to return).
inline bool trace_on() {
    static int v = -1;
    if (v < 0) {
        const char *e = getenv("GPSGS_TRACE");
        v = (e && *e && *e != '0') ? 1 : 0;
    }
    return v == 1;
}
inline void trace(const char *what, int P, int W, int H, long long cap, unsigned flags) {
    if (trace_on()) { fprintf(stderr, "[gpsgs] %s P=%d %dx%d cap=%lld flags=0x%x ...", what, P, W, H, cap, flags); fflush(stderr); }
}

inline int check(hipStream_t s, unsigned flags) {
    if (hipGetLastError() != hipSuccess) return GPSGS_E_LAUNCH;
    if ((flags & GSR_FLAG_DEBUG) || trace_on()) {
        if (hipStreamSynchronize(s) != hipSuccess) return GPSGS_E_LAUNCH;
        if (hipGetLastError() != hipSuccess) return GPSGS_E_LAUNCH;
        if (trace_on()) { fprintf(stderr, " ok\n"); fflush(stderr); }
    }
    return GPSGS_OK;
}

// ---- optional per-stage hipEvent recorder (GSR_FLAG_TIMING) ---------------------------------------------------------
constexpr int TIMING_MAX = 8192;
struct Recorder {
    hipEvent_t ev[TIMING_MAX][2];
    int stage[TIMING_MAX];
    int created = 0, n = 0;
} g_rec;

struct StageTimer {  // RAII: records an event pair around one stage when timing is on
    bool on;
    int slot;
    hipStream_t s;
    StageTimer(unsigned flags, int stage, hipStream_t s_) : on((flags & GSR_FLAG_TIMING) != 0), slot(-1), s(s_) {
        const unsigned only = (flags >> 4) & 0xFu;  // GSR_FLAG_TIMING_STAGE(k): bracket stage k only (less perturbation)
        if (only && (int)only - 1 != stage) on = false;
        if (!on || g_rec.n >= TIMING_MAX) { on = false; return; }
        slot = g_rec.n++;
        if (slot >= g_rec.created) {
            (void)hipEventCreate(&g_rec.ev[slot][0]);
            (void)hipEventCreate(&g_rec.ev[slot][1]);
            g_rec.created = slot + 1;
        }
        g_rec.stage[slot] = stage;
        (void)hipEventRecord(g_rec.ev[slot][0], s);
    }
    ~StageTimer() {
        if (on) (void)hipEventRecord(g_rec.ev[slot][1], s);
    }
};

__global__ void k_export(int P, int T, const GsrSplat *__restrict__ splats, GsrBins bins, float *depth,
                         float *xy, float *conic_opacity, int *rect, int64_t *tile_ranges) {  // T = number of bins
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < P) {
        const GsrSplat s = splats[i];
        if (depth) depth[i] = s.depth;
        if (xy) { xy[2 * i] = s.x; xy[2 * i + 1] = s.y; }
        if (conic_opacity) { conic_opacity[4 * i] = s.A; conic_opacity[4 * i + 1] = s.B; conic_opacity[4 * i + 2] = s.C; conic_opacity[4 * i + 3] = s.op; }
        if (rect) { rect[4 * i] = s.bin_lo & 0xffff; rect[4 * i + 1] = s.bin_lo >> 16; rect[4 * i + 2] = s.bin_hi & 0xffff; rect[4 * i + 3] = s.bin_hi >> 16; }
    }
    if (i < T && tile_ranges) {
        uint32_t a, b;
        gsr_bin_range(bins, (uint32_t)i, a, b);
        tile_ranges[2 * i] = b > a ? (int64_t)a : 0;
        tile_ranges[2 * i + 1] = b > a ? (int64_t)b : 0;
    }
}

// GPSGS_TRACE only: after the sort, every entry of every bin list must be a Gaussian of the view and the lists must be in key order
__global__ void k_validate_lists(int P, int NB, GsrBins bins, const uint32_t *__restrict__ bin_cursor, const uint32_t *__restrict__ point_list,
                                 const GsrSplat *__restrict__ splats, unsigned long long *__restrict__ out) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= NB) return;
    uint32_t r0, r1;
    gsr_bin_range(bins, (uint32_t)b, r0, r1);
    // scanned lists: the scatter pass filled exactly the slots the count pass reserved (direct lists have no second pass: a slot nobody wrote shows
    // up below as an id that is not a Gaussian of the view, or out of order)
    if (!bins.cap && bin_cursor[(size_t)b * GSR_CPAD] != r1) atomicAdd(out + 4, 1ull);
    unsigned long long bad_id = 0, bad_order = 0, bad_rec = 0;
    uint64_t prev = 0;
    for (uint32_t k = r0; k < r1; k++) {
        const uint32_t id = point_list[k];
        if (id >= (uint32_t)P) { bad_id++; continue; }
        const GsrSplat s = splats[id];
        if (!(s.x == s.x) || !(s.A == s.A) || !(s.op == s.op)) bad_rec++;
        const uint64_t key = ((uint64_t)__float_as_uint(s.depth) << 32) | id;
        if (k > r0 && key <= prev) bad_order++;
        prev = key;
    }
    if (bad_id) atomicAdd(out + 0, bad_id);
    if (bad_order) atomicAdd(out + 1, bad_order);
    if (bad_rec) atomicAdd(out + 2, bad_rec);
    if (bad_id) atomicMax(out + 3, (unsigned long long)(r1 - r0));
}

// gsr_debug_count_records: how many gradient-record slots the last backward flagged (bench.py prices the record traffic with it)
__global__ __launch_bounds__(256) void k_count_flags(const uint8_t *__restrict__ flags, const GsrHeader *__restrict__ hdr, unsigned long long *__restrict__ out) {
    const uint32_t n = hdr->num_slots;
    unsigned long long c = 0;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) c += flags[i] != 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
    if (blockIdx.x == 0 && threadIdx.x == 0) out[1] = n;
}

// the forward's counter section (header + scan partials + bin_count + bin_count_fb: 0.13 MB at 1024^2) zeroed by a plain kernel instead of the
// runtime's fill path: 4.3 us against 4.7 (min 2.5 / 2.6) in the round-5 kernel trace -- most of it is being the first launch behind the
// previous step's 160 MB of gradient-record traffic, not the zeroing
__global__ __launch_bounds__(256) void k_zero16(uint4 *__restrict__ p, uint32_t n16) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n16) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace

extern "C" int gpsgs_abi_version(void) { return GPSGS_ABI_VERSION; }

extern "C" int gsr_supported_flags(void) {
    return (int)(GSR_FLAG_DEBUG | GSR_FLAG_TIMING | GSR_FLAG_NO_LARGE_SORT | GSR_FLAG_COMPOSITE_TILES | GSR_FLAG_NO_COLOR_GRAD | GSR_FLAG_WAVE_PRIORITY |
                 GSR_FLAG_ANTIALIAS);
}

extern "C" const char *gpsgs_build_info(void) { return "gfx950 hipcc " __VERSION__ " built " __DATE__; }

namespace {
// What every gsr_workspace_bytes_* function reports: 0 for invalid arguments (a bin capacity that direct lists cannot have included), else what a call
// with these needs demands (gsr_workspace_need)
size_t workspace_size(int P, int width, int height, int64_t instance_capacity, uint32_t bin_capacity, const GsrWorkspaceNeed &need) {
    if (P < 0 || width < 0 || height < 0 || instance_capacity < 0) return 0;
    if (bin_capacity && !gsr_direct_lists_ok(width, height, bin_capacity)) return 0;
    return gsr_workspace_need(gsr_layout(P, width, height, instance_capacity, bin_capacity), instance_capacity, need);
}
}  // namespace

extern "C" int gsr_direct_lists_ok(int width, int height, uint32_t bin_capacity) {
    if (width <= 0 || height <= 0 || bin_capacity == 0u || bin_capacity > GSR_DIRECT_MAX_CAP || (bin_capacity & 63u)) return 0;
    const GsrLayout L = gsr_layout(0, width, height, 0);
    const int nt = ((L.bx + 7) / 8) * ((L.by + 7) / 8) * 64;
    return (L.NB <= GSR_DIRECT_MAX_BINS && nt <= GSR_DIRECT_MAX_BINS) ? 1 : 0;
}

extern "C" size_t gsr_workspace_bytes(int P, int width, int height, int64_t instance_capacity) {
    return workspace_size(P, width, height, instance_capacity, 0u, {false, false, 0, false, false});
}

extern "C" size_t gsr_workspace_bytes_forward_only(int P, int width, int height, int64_t instance_capacity) {
    return workspace_size(P, width, height, instance_capacity, 0u, {true, false, 0, false, false});
}

extern "C" size_t gsr_workspace_bytes_ex(int P, int width, int height, int64_t instance_capacity, uint32_t bin_capacity, int forward_only) {
    return workspace_size(P, width, height, instance_capacity, bin_capacity, {forward_only != 0, false, 0, false, false});
}

extern "C" size_t gsr_workspace_bytes_depth_alpha(int P, int width, int height, int64_t instance_capacity, uint32_t bin_capacity, int forward_only) {
    return workspace_size(P, width, height, instance_capacity, bin_capacity, {forward_only != 0, true, 0, false, false});
}

extern "C" size_t gsr_workspace_bytes_features(int P, int width, int height, int64_t instance_capacity, uint32_t bin_capacity, int channels, int forward_only) {
    if (channels < 1 || channels > GSR_MAX_FEATURES) return 0;
    return workspace_size(P, width, height, instance_capacity, bin_capacity, {forward_only != 0, true, channels, false, false});
}

extern "C" size_t gsr_workspace_bytes_contrib(int P, int width, int height, int64_t instance_capacity, uint32_t bin_capacity, int forward_only) {
    (void)forward_only;  // (the same size: the statistics read the slot prefix of the backward tail)
    return workspace_size(P, width, height, instance_capacity, bin_capacity, {false, true, 0, true, false});
}

extern "C" size_t gsr_workspace_bytes_absgrad(int P, int width, int height, int64_t instance_capacity, uint32_t bin_capacity) {
    return workspace_size(P, width, height, instance_capacity, bin_capacity, {false, true, 0, false, true});
}

namespace {
// What the forward and backward entry points receive: the view (GSR_VIEW_CALL fills it from the argument names they all share), then each direction's own
struct ViewCall {
    int P, width, height;
    const float *means3D, *colors, *opacities, *scales, *rotations;
    float scale_modifier, tanfovx, tanfovy;
    const float *viewmatrix, *projmatrix, *bg;
    void *workspace;
    size_t workspace_bytes;
    int64_t instance_capacity;
    unsigned flags;
    void *stream;
    const GsrViewExt *ext;
};
#define GSR_VIEW_CALL(ext_)                                                                                                                          \
    {P, width, height, means3D, colors, opacities, scales, rotations, scale_modifier, tanfovx, tanfovy, viewmatrix, projmatrix, bg, workspace, workspace_bytes, \
     instance_capacity, flags, stream, ext_}
struct ForwardCall : ViewCall {
    float *out_color;
    int *radii;
    void *host_header_out;
    uint32_t notify_seq;
    const GsrFeatures *feat;     // gsr_forward_features
    const GsrContrib *contrib;   // gsr_forward_contrib
    const GsrDistort *distort;   // gsr_forward_distort
};
struct BackwardCall : ViewCall {
    const int *radii;
    const float *dL_dpix;
    float *dL_dmeans3D, *dL_dmeans2D, *dL_dcolors, *dL_dopacity, *dL_dscales, *dL_drotations;
    const GsrCamGrad *cam;    // gsr_backward_camera / _features / _absgrad with a camera gradient asked for
    const GsrFeatures *feat;  // gsr_backward_features
    const GsrAbsGrad *abs;    // gsr_backward_absgrad
    const GsrDistort *distort;  // gsr_backward_distort
};

// One stage of a call: announced (GPSGS_TRACE), bracketed by an event pair (GSR_FLAG_TIMING), launched, checked
struct Stages {
    const ViewCall &c;
    unsigned flags;  // (the call's, less the tile family where an option has only VALU kernels)
    hipStream_t s;
    template <typename Launch>
    int operator()(const char *name, int stage, Launch &&launch) const {
        trace(name, c.P, c.width, c.height, (long long)c.instance_capacity, flags);
        {
            StageTimer t(flags, stage, s);
            launch();
        }
        return check(s, flags);
    }
};

// F-channel feature maps: the channel count of a GsrFeatures (0 = none), or -1 for an invalid one (range, NULL features for P > 0, misaligned pointers)
int feature_channels(const GsrFeatures *feat, bool backward, int P) {
    if (!feat || feat->channels == 0) return 0;
    if (feat->channels < 0 || feat->channels > GSR_MAX_FEATURES || (P > 0 && !feat->features)) return -1;  // (a view without Gaussians has no rows)
    const uintptr_t a = reinterpret_cast<uintptr_t>(feat->features) | reinterpret_cast<uintptr_t>(feat->out_features) |
                        (backward ? reinterpret_cast<uintptr_t>(feat->dL_dfeatures) : 0u);
    if (a & 3u) return -1;
    if (!backward && !feat->out_features) return -1;
    return feat->channels;
}

// Self-check between the sort and the compositing (GPSGS_TRACE / GSR_FLAG_DEBUG; synchronises; never in normal operation)
int validate_lists(int P, int NB, const GsrWorkspace &w, hipStream_t s) {
    // everything on the caller's stream `s` and checked: PyTorch's side streams do not synchronise with the NULL stream, so a NULL-stream memset of
    // the counters could land AFTER k_validate_lists' atomics and hide a real inconsistency.  The five counters live in a small
    // device buffer allocated once per process (a debug forward is never captured, but it no longer allocates per call either).
    GsrHeader h;
    unsigned long long h_out[5] = {0, 0, 0, 0, 0};
    static unsigned long long *d_out_by_dev[64] = {nullptr};
    int devid = 0;
    if (hipGetDevice(&devid) != hipSuccess || devid < 0 || devid >= 64) return GPSGS_E_LAUNCH;
    unsigned long long *d_out;
    {
        static std::mutex mu;
        std::lock_guard<std::mutex> g(mu);
        if (!d_out_by_dev[devid] && hipMalloc(&d_out_by_dev[devid], sizeof(h_out)) != hipSuccess) return GPSGS_E_LAUNCH;
        d_out = d_out_by_dev[devid];
    }
    if (hipMemcpyAsync(&h, w.hdr, sizeof(h), hipMemcpyDeviceToHost, s) != hipSuccess || hipMemsetAsync(d_out, 0, sizeof(h_out), s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return GPSGS_E_LAUNCH;
    if (!h.overflow) hipLaunchKernelGGL(k_validate_lists, dim3((NB + 255) / 256), dim3(256), 0, s, P, NB, w.bins, w.bin_cursor, w.point_list, w.splats, d_out);
    if (hipMemcpyAsync(h_out, d_out, sizeof(h_out), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return GPSGS_E_LAUNCH;
    const bool bad = h_out[0] || h_out[1] || h_out[4];
    if (trace_on() || bad) {
        fprintf(stderr, "[gpsgs] header: R=%llu overflow=%u longest=%u busy=%u slots=%u points=%u | lists: ids out of range %llu, out of order %llu, non-finite records %llu, "
                        "bins whose scatter cursor missed its end %llu (longest list with a bad id %llu)\n",
                (unsigned long long)h.num_rendered, h.overflow, h.max_tile_count, h.num_busy_wgs, h.num_slots, h.num_points, h_out[0], h_out[1], h_out[2], h_out[4], h_out[3]);
        fflush(stderr);
    }
    return bad ? GPSGS_E_INTERNAL : GPSGS_OK;
}

inline bool misaligned(const void *a, const void *b = nullptr, const void *c = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 3u) != 0;
}

// depth-distortion map: is a GsrDistort (NULL = none) one the entry points accept?  (map = out_distort | dL_ddistort: the two share their slot)
inline bool distort_ok(const GsrDistort *d) {
    if (!d) return true;
    return !(misaligned(d->out_distort, d->totals) || d->reserved[0] || d->reserved[1] || (d->out_distort && !d->totals));
}

int forward_impl(const ForwardCall &c) {
    const int P = c.P, width = c.width, height = c.height;
    const int64_t instance_capacity = c.instance_capacity;
    const GsrViewExt *ext = c.ext;
    const int F = feature_channels(c.feat, false, P);
    if (F < 0) return GPSGS_E_INVALID;
    // contribution statistics (any pointer may be NULL): the VALU family's CONTRIB forward, 16 bytes per instance slot in the workspace's tail
    const GsrContrib con = c.contrib ? *c.contrib : GsrContrib{};
    if (con.reserved || misaligned(con.weight_sum, con.weight_max, con.pixel_count)) return GPSGS_E_INVALID;
    // opt-in depth / alpha maps
    float *out_depth = ext ? ext->out_depth : nullptr, *out_alpha = ext ? ext->out_alpha : nullptr;
    if (misaligned(out_depth, out_alpha)) return GPSGS_E_INVALID;
    const bool stats = con.weight_sum || con.weight_max || con.pixel_count;
    if (!gsr_one_tail(F, stats, false)) return GPSGS_E_INVALID;  // (no entry point passes both)
    // depth-distortion map: the VALU family's EXTRA + DISTORT forward, its totals in the caller's plane (no workspace tail)
    if (!distort_ok(c.distort)) return GPSGS_E_INVALID;
    float *out_distort = c.distort ? c.distort->out_distort : nullptr;
    // feature maps, statistics, depth / alpha maps, the distortion map: made by the VALU compositing kernels only (the tiles flag is ignored for such a view)
    const unsigned flags = (F > 0 || stats || out_depth || out_alpha || out_distort) ? c.flags & ~GSR_FLAG_COMPOSITE_TILES : c.flags;
    if (P < 0 || width <= 0 || height <= 0 || instance_capacity < 0 || instance_capacity > 0x7fffffffLL) return GPSGS_E_INVALID;
    if (width > 65535 * GSR_TILE || height > 65535 * GSR_TILE) return GPSGS_E_INVALID;
    if (!c.out_color || !c.workspace) return GPSGS_E_INVALID;
    const float *shs = ext ? ext->shs : nullptr, *cov3D_precomp = ext ? ext->cov3D_precomp : nullptr;
    if (P > 0 && (!c.means3D || !c.opacities || !c.viewmatrix || !c.projmatrix || !c.bg || !c.radii)) return GPSGS_E_INVALID;
    // exactly one of (colors, shs) and exactly one of (scales + rotations, cov3D_precomp): upstream's GaussianRasterizer.forward raises on both
    if (P > 0 && ((shs != nullptr) == (c.colors != nullptr) || (cov3D_precomp != nullptr) == (c.scales != nullptr && c.rotations != nullptr))) return GPSGS_E_INVALID;
    if (P > 0 && cov3D_precomp && (c.scales || c.rotations)) return GPSGS_E_INVALID;
    if (shs && (!ext->campos || ext->sh_degree > 3u || ext->sh_coeffs > 16u || (ext->sh_degree + 1u) * (ext->sh_degree + 1u) > ext->sh_coeffs)) return GPSGS_E_INVALID;
    const uint32_t bin_cap = ext ? ext->bin_capacity : 0u;  // direct lists: a fixed-capacity segment per bin (GsrBins)
    if (bin_cap && !gsr_direct_lists_ok(width, height, bin_cap)) return GPSGS_E_INVALID;
    const GsrLayout L = gsr_layout(P, width, height, instance_capacity, bin_cap);
    if (c.workspace_bytes < gsr_workspace_need(L, instance_capacity, {true, false, 0, stats, false})) return GPSGS_E_WORKSPACE;  // the backward tail is optional, but not for the statistics
    hipStream_t s = (hipStream_t)c.stream;
    uint32_t *host_hdr = nullptr;
    if (c.host_header_out) {  // must be pinned (hipHostMalloc / hipHostRegister) memory the device can write
        void *dptr = nullptr;
        if (c.notify_seq == 0 || hipHostGetDevicePointer(&dptr, c.host_header_out, 0) != hipSuccess || !dptr) {
            (void)hipGetLastError();
            return GPSGS_E_INVALID;
        }
        host_hdr = static_cast<uint32_t *>(dptr);
    }
    // a workspace that includes the backward tail gets the per-Gaussian slot prefix and cleared record flags from the forward
    const bool training = c.workspace_bytes >= L.total;
    const GsrWorkspace w = gsr_workspace_map(c.workspace, L, training);

    // header + scan partials (their ready flags) + bin_count + bin_count_fb (+ bin_cursor with direct lists, where no scan initialises it) are adjacent
    {
        const size_t zb = (bin_cap ? L.bin_offset : L.bin_cursor) - L.header;  // sections are 256-byte aligned: a whole number of 16-byte words
        if ((zb & 15u) == 0 && (reinterpret_cast<uintptr_t>(w.hdr) & 15u) == 0) {
            const uint32_t n16 = (uint32_t)(zb >> 4);
            hipLaunchKernelGGL(k_zero16, dim3((n16 + 255u) / 256u), dim3(256), 0, s, reinterpret_cast<uint4 *>(w.hdr), n16);
            if (hipGetLastError() != hipSuccess) return GPSGS_E_LAUNCH;  // stale scan flags / bin counts would corrupt the whole view
        } else if (hipMemsetAsync(w.hdr, 0, zb, s) != hipSuccess) {
            return GPSGS_E_LAUNCH;
        }
    }
    if (P == 0) {  // upstream returns its zero-initialised image (NOT the background) when there is nothing to draw
        const size_t map_bytes = sizeof(float) * (size_t)width * height;
        if (hipMemsetAsync(c.out_color, 0, 3 * map_bytes, s) != hipSuccess) return GPSGS_E_LAUNCH;
        if (out_depth && hipMemsetAsync(out_depth, 0, map_bytes, s) != hipSuccess) return GPSGS_E_LAUNCH;
        if (out_alpha && hipMemsetAsync(out_alpha, 0, map_bytes, s) != hipSuccess) return GPSGS_E_LAUNCH;
        if (out_distort && (hipMemsetAsync(out_distort, 0, map_bytes, s) != hipSuccess || hipMemsetAsync(c.distort->totals, 0, 2 * map_bytes, s) != hipSuccess))
            return GPSGS_E_LAUNCH;
        if (F > 0 && hipMemsetAsync(c.feat->out_features, 0, (size_t)F * map_bytes, s) != hipSuccess) return GPSGS_E_LAUNCH;
        if (hipMemsetAsync(w.bin_offset, 0, (size_t)(L.NB + 1) * 4, s) != hipSuccess) return GPSGS_E_LAUNCH;
        return check(s, flags);
    }
    const uint32_t *row_range = ext ? ext->row_range : nullptr;
    const uint32_t order_hint = ext ? ext->order_hint : 0u;
    GsrFwdParams q;
    q.P = P; q.W = width; q.H = height; q.gx = L.gx; q.gy = L.gy; q.bx = L.bx; q.by = L.by; q.bx_real = L.bx_real;
    q.means3D = c.means3D; q.colors = c.colors; q.opacities = c.opacities; q.scales = c.scales; q.rotations = c.rotations;
    q.scale_modifier = c.scale_modifier; q.tanfovx = c.tanfovx; q.tanfovy = c.tanfovy;
    q.view = c.viewmatrix; q.proj = c.projmatrix; q.bg = c.bg; q.out_color = c.out_color; q.radii = c.radii; q.cap = instance_capacity;
    q.row_range = row_range;
    q.shs = shs; q.campos = shs ? ext->campos : nullptr; q.cov3D_precomp = cov3D_precomp;
    q.sh_degree = shs ? ext->sh_degree : 0u; q.sh_coeffs = shs ? ext->sh_coeffs : 0u;
    q.antialias = (flags & GSR_FLAG_ANTIALIAS) ? 1 : 0;  // (k_preprocess<true>: the record's opacity is opacity * k)
    q.goff = w.goff; q.gpart = w.gscan_part;
    const int n_gblocks = (P + GSR_BIN_THREADS - 1) / GSR_BIN_THREADS;
    const bool no_large_sort = (flags & GSR_FLAG_NO_LARGE_SORT) != 0, self_check = trace_on() || (flags & GSR_FLAG_DEBUG);

    // direct lists + tile family: the forward compositing waves sort their own lists (no sort launch).  Not with the debug self-check, which inspects the
    // sorted lists between the two; GPSGS_FUSED_SORT=0 keeps the separate launch (development: A/B timing)
    static const bool fused_sort_env = [] { const char *e = getenv("GPSGS_FUSED_SORT"); return !(e && e[0] == '0'); }();
    const bool fused_sort = bin_cap && (flags & GSR_FLAG_COMPOSITE_TILES) && fused_sort_env && !self_check;
    const Stages stage = {c, flags, s};
    int rc;
    if ((rc = stage("preprocess", GSR_STAGE_PREPROCESS, [&] { gsr_launch_preprocess(q, w.splats, w.binrec, w.wg_tab, w.bin_count, w.bin_count_fb, w.hdr, s); })) != GPSGS_OK)
        return rc;
    if (bin_cap) {
        // direct lists: the scatter needs no offsets (slot = bin x capacity + recorded base + rank), its first workgroups publish the header (also towards the
        // host) and do what is left of the scan (work order, slot prefix) beside the scattering ones
        rc = stage("scatter (direct lists)", GSR_STAGE_SCATTER, [&] {
            gsr_launch_scatter_direct(P, row_range, L.bx, L.by, L.NB, w.splats, w.binrec, w.wg_tab, w.bin_count, w.bin_count_fb, w.bin_cursor, bin_cap, w.keys, w.hdr,
                                      instance_capacity, w.gscan_part, w.gprefix, n_gblocks, w.wg_order, w.scan_part, order_hint, host_hdr, c.notify_seq, s);
        });
        if (rc == GPSGS_OK && !fused_sort)
            rc = stage("sort (direct lists)", GSR_STAGE_SORT, [&] { gsr_launch_sort_direct(L.NB, w.bins, w.wg_order, w.keys, w.point_list, w.hdr, s); });
    } else {
        rc = stage("scan", GSR_STAGE_SCAN, [&] {
            gsr_launch_scan(w.bin_count, w.bin_count_fb, w.bin_offset, w.bin_cursor, w.wg_order, w.scan_part, L.NB, L.bx, L.by, instance_capacity, w.hdr, w.gscan_part, n_gblocks,
                            host_hdr, c.notify_seq, no_large_sort, order_hint, s);
        });
        if (rc == GPSGS_OK)
            rc = stage("scatter", GSR_STAGE_SCATTER, [&] { gsr_launch_scatter(P, row_range, L.bx, w.splats, w.binrec, w.wg_tab, w.bin_offset, w.bin_cursor, w.keys, w.hdr, s); });
        if (rc == GPSGS_OK)
            rc = stage("sort", GSR_STAGE_SORT, [&] { gsr_launch_sort(L.NB, w.bin_offset, w.wg_order, w.keys, w.point_list, w.hdr, no_large_sort, s); });
    }
    if (rc == GPSGS_OK && self_check) rc = validate_lists(P, L.NB, w, s);
    if (rc != GPSGS_OK) return rc;
    GsrCompositeFwd k = {width, height, L.bx, L.by, w.splats, w.bins, w.wg_order, w.point_list, c.bg, c.out_color, w.final_T, w.n_contrib, w.hdr, w.inst_valid, s, out_depth, out_alpha};
    if (F > 0) { k.features = c.feat->features; k.F = F; k.row_range = row_range; k.out_feat = c.feat->out_features; }
    if (stats) { k.goff = w.goff; k.gpart = w.gprefix; k.inst_contrib = static_cast<float4 *>(w.tail); }
    if (out_distort) { k.out_distort = out_distort; k.totals = c.distort->totals; }
    rc = stage("composite_fwd", GSR_STAGE_COMPOSITE_FWD, [&] {
        if (flags & GSR_FLAG_COMPOSITE_TILES) return gsr_launch_composite_fwd_tiles(k, training, (flags & GSR_FLAG_WAVE_PRIORITY) != 0, fused_sort ? w.keys : nullptr);
        if (k.inst_contrib) gsr_launch_contrib_clear(k.inst_contrib, instance_capacity, w.hdr, s);
        gsr_launch_composite_fwd(k);
    });
    if (rc == GPSGS_OK && k.inst_contrib)
        rc = stage("contrib_gather", GSR_STAGE_COMPOSITE_FWD, [&] {
            gsr_launch_contrib_gather(P, row_range, c.radii, k.goff, k.gpart, k.inst_contrib, w.hdr, con.weight_sum, con.weight_max, con.pixel_count, s);
        });
    return rc;
}
}  // namespace

extern "C" int gsr_forward_ex(int P, int width, int height, const float *means3D, const float *colors, const float *opacities,
                              const float *scales, const float *rotations, float scale_modifier, float tanfovx, float tanfovy,
                              const float *viewmatrix, const float *projmatrix, const float *bg, float *out_color, int *radii,
                              void *workspace, size_t workspace_bytes, int64_t instance_capacity, unsigned flags, void *stream,
                              void *host_header_out, uint32_t notify_seq, const GsrViewExt *ext) {
    return forward_impl({GSR_VIEW_CALL(ext), out_color, radii, host_header_out, notify_seq, nullptr, nullptr, nullptr});
}

extern "C" int gsr_forward_features(int P, int width, int height, const float *means3D, const float *colors, const float *opacities,
                                    const float *scales, const float *rotations, float scale_modifier, float tanfovx, float tanfovy,
                                    const float *viewmatrix, const float *projmatrix, const float *bg, float *out_color, int *radii,
                                    void *workspace, size_t workspace_bytes, int64_t instance_capacity, unsigned flags, void *stream,
                                    void *host_header_out, uint32_t notify_seq, const GsrViewExt *ext, const GsrFeatures *feat) {
    return forward_impl({GSR_VIEW_CALL(ext), out_color, radii, host_header_out, notify_seq, feat, nullptr, nullptr});
}

extern "C" int gsr_forward_contrib(int P, int width, int height, const float *means3D, const float *colors, const float *opacities,
                                   const float *scales, const float *rotations, float scale_modifier, float tanfovx, float tanfovy,
                                   const float *viewmatrix, const float *projmatrix, const float *bg, float *out_color, int *radii,
                                   void *workspace, size_t workspace_bytes, int64_t instance_capacity, unsigned flags, void *stream,
                                   void *host_header_out, uint32_t notify_seq, const GsrViewExt *ext, const GsrContrib *contrib) {
    return forward_impl({GSR_VIEW_CALL(ext), out_color, radii, host_header_out, notify_seq, nullptr, contrib, nullptr});
}

extern "C" int gsr_forward_distort(int P, int width, int height, const float *means3D, const float *colors, const float *opacities,
                                   const float *scales, const float *rotations, float scale_modifier, float tanfovx, float tanfovy,
                                   const float *viewmatrix, const float *projmatrix, const float *bg, float *out_color, int *radii,
                                   void *workspace, size_t workspace_bytes, int64_t instance_capacity, unsigned flags, void *stream,
                                   void *host_header_out, uint32_t notify_seq, const GsrViewExt *ext, const GsrDistort *distort) {
    return forward_impl({GSR_VIEW_CALL(ext), out_color, radii, host_header_out, notify_seq, nullptr, nullptr, distort});
}

extern "C" int gsr_forward_notify(int P, int width, int height, const float *means3D, const float *colors, const float *opacities,
                                  const float *scales, const float *rotations, float scale_modifier, float tanfovx, float tanfovy,
                                  const float *viewmatrix, const float *projmatrix, const float *bg, float *out_color, int *radii,
                                  void *workspace, size_t workspace_bytes, int64_t instance_capacity, unsigned flags, void *stream,
                                  void *host_header_out, uint32_t notify_seq) {
    return forward_impl({GSR_VIEW_CALL(nullptr), out_color, radii, host_header_out, notify_seq, nullptr, nullptr, nullptr});
}

extern "C" int gsr_forward(int P, int width, int height, const float *means3D, const float *colors, const float *opacities,
                           const float *scales, const float *rotations, float scale_modifier, float tanfovx, float tanfovy,
                           const float *viewmatrix, const float *projmatrix, const float *bg, float *out_color, int *radii,
                           void *workspace, size_t workspace_bytes, int64_t instance_capacity, unsigned flags, void *stream) {
    return forward_impl({GSR_VIEW_CALL(nullptr), out_color, radii, nullptr, 0u, nullptr, nullptr, nullptr});
}

extern "C" size_t gsr_camera_grad_scratch_bytes(int P) {
    if (P <= 0) return 0;
    return sizeof(float) * (size_t)GSR_CAMGRAD_TERMS * (size_t)((P + 255) / 256);  // one partial per term and preprocess_bwd workgroup
}

namespace {
// gsr_backward_ex, and with cam (gsr_backward_camera) the camera gradients too: the same validation, the same launches up to the preprocess
// backward, which then runs its CAMGRAD instantiation (bit-identical per-Gaussian results) and the fixed-order sum of the workgroup partials
int backward_impl(const BackwardCall &c) {
    // (c.colors: already folded into the splat records of the workspace; so are the opacities -- read again only with antialiasing)
    const int P = c.P, width = c.width, height = c.height;
    const int64_t instance_capacity = c.instance_capacity;
    const GsrViewExt *ext = c.ext;
    const bool antialias = (c.flags & GSR_FLAG_ANTIALIAS) != 0;
    // depth / alpha gradients (either may be NULL = zero): the VALU family's EXTRA kernels, one more float per instance slot in the workspace
    const float *dL_ddepth = ext ? ext->dL_ddepth : nullptr, *dL_dalpha = ext ? ext->dL_dalpha : nullptr;
    if (misaligned(dL_ddepth, dL_dalpha)) return GPSGS_E_INVALID;
    // feature maps (either gradient pointer may be NULL): the VALU family's feature kernels, cap x F more floats in the workspace's feature tail
    const int F = feature_channels(c.feat, true, P);
    if (F < 0) return GPSGS_E_INVALID;
    const float *dL_dfeat = F > 0 ? c.feat->dL_dfeaturemap : nullptr;
    float *dL_dfeatures = F > 0 ? c.feat->dL_dfeatures : nullptr;
    const bool feat_sums = dL_dfeat && dL_dfeatures;  // the per-slot feature sums (part b) are formed
    // absolute screen-space gradient: the VALU family's ABSGRAD kernels, 8 bytes per instance slot in the workspace's absgrad tail
    if (c.abs && c.abs->reserved) return GPSGS_E_INVALID;
    float2 *absgrad = c.abs ? reinterpret_cast<float2 *>(c.abs->absgrad) : nullptr;
    if (misaligned(absgrad) || !gsr_one_tail(F, false, absgrad != nullptr)) return GPSGS_E_INVALID;  // (no entry point passes both)
    // depth-distortion map: the VALU family's EXTRA + DISTORT backward; its dL/dz term rides in inst_ddepth (the depth / alpha workspace size)
    if (!distort_ok(c.distort)) return GPSGS_E_INVALID;
    const float *dL_ddistort = c.distort ? c.distort->dL_ddistort : nullptr;
    const bool extras = dL_ddepth || dL_dalpha || dL_ddistort;
    const unsigned flags = (extras || F > 0 || absgrad) ? c.flags & ~GSR_FLAG_COMPOSITE_TILES : c.flags;  // options only the VALU kernels have
    if (P < 0 || width <= 0 || height <= 0 || instance_capacity < 0) return GPSGS_E_INVALID;
    hipStream_t s = (hipStream_t)c.stream;
    if (P == 0) {
        if (c.cam) {  // nothing rendered: the camera gradients are zeros
            float *outs[3] = {c.cam->d_view, c.cam->d_proj, c.cam->d_campos};
            const size_t n[3] = {16, 16, 3};
            for (int k = 0; k < 3; k++)
                if (outs[k] && hipMemsetAsync(outs[k], 0, n[k] * sizeof(float), s) != hipSuccess) return GPSGS_E_LAUNCH;
            return check(s, flags);
        }
        return GPSGS_OK;
    }
    if (c.cam && c.cam->scratch && misaligned(c.cam->scratch)) return GPSGS_E_INVALID;
    const float *shs = ext ? ext->shs : nullptr, *cov3D_precomp = ext ? ext->cov3D_precomp : nullptr;
    if (!c.means3D || !c.viewmatrix || !c.projmatrix || !c.bg || !c.radii || !c.dL_dpix || !c.dL_dmeans3D || !c.dL_dmeans2D || !c.dL_dopacity || !c.workspace)
        return GPSGS_E_INVALID;
    if (!shs && !c.dL_dcolors) return GPSGS_E_INVALID;
    if (antialias && !c.opacities) return GPSGS_E_INVALID;  // dL/dk = g * opacity
    if (cov3D_precomp ? (!ext->dL_dcov3D || c.scales || c.rotations) : (!c.scales || !c.rotations || !c.dL_dscales || !c.dL_drotations)) return GPSGS_E_INVALID;
    if (shs && (!ext->campos || !ext->dL_dsh || ext->sh_degree > 3u || ext->sh_coeffs > 16u || (ext->sh_degree + 1u) * (ext->sh_degree + 1u) > ext->sh_coeffs))
        return GPSGS_E_INVALID;
    const uint32_t bin_cap = ext ? ext->bin_capacity : 0u;  // must be what the forward was given
    if (bin_cap && !gsr_direct_lists_ok(width, height, bin_cap)) return GPSGS_E_INVALID;
    const GsrLayout L = gsr_layout(P, width, height, instance_capacity, bin_cap);
    if (c.workspace_bytes < gsr_workspace_need(L, instance_capacity, {false, extras, feat_sums ? F : 0, false, absgrad != nullptr})) return GPSGS_E_WORKSPACE;
    // goff / gprefix / cleared inst_valid were produced by the matching gsr_forward (training workspace)
    const GsrWorkspace w = gsr_workspace_map(c.workspace, L, true);
    const uint32_t *row_range = ext ? ext->row_range : nullptr;
    GsrCompositeBwd k = {width, height, L.bx, L.by, w.splats, w.bins, w.wg_order, w.point_list, c.bg, c.dL_dpix, w.final_T, w.n_contrib, w.goff, w.gprefix, w.inst_valid, w.inst_dop,
                         w.inst_grad, w.hdr, s, dL_ddepth, dL_dalpha, extras ? w.inst_ddepth : nullptr};
    if (F > 0) { k.features = c.feat->features; k.F = F; k.row_range = row_range; k.dL_dfeat = dL_dfeat; k.inst_dfeat = feat_sums ? static_cast<float *>(w.tail) : nullptr; }
    if (absgrad) k.inst_absgrad = static_cast<float2 *>(w.tail);  // (the contribution tail's place: dead by now)
    if (dL_ddistort) { k.dL_ddistort = dL_ddistort; k.totals = c.distort->totals; }

    const Stages stage = {c, flags, s};
    // must be the same family as the forward that filled the workspace: the two designs round the exponent differently, and the
    // backward has to repeat the forward's per-pixel decisions
    int rc = stage("composite_bwd", GSR_STAGE_COMPOSITE_BWD, [&] {
        if (flags & GSR_FLAG_COMPOSITE_TILES) gsr_launch_composite_bwd_tiles(k, (flags & GSR_FLAG_NO_COLOR_GRAD) == 0, (flags & GSR_FLAG_WAVE_PRIORITY) != 0);
        else gsr_launch_composite_bwd(k);
    });
    if (rc != GPSGS_OK) return rc;
    GsrBwdParams b;
    b.P = P; b.W = width; b.H = height;
    b.means3D = c.means3D; b.scales = c.scales; b.rotations = c.rotations;
    b.scale_modifier = c.scale_modifier; b.tanfovx = c.tanfovx; b.tanfovy = c.tanfovy;
    b.view = c.viewmatrix; b.proj = c.projmatrix; b.radii = c.radii;
    b.dL_dmeans3D = c.dL_dmeans3D; b.dL_dmeans2D = c.dL_dmeans2D; b.dL_dcolors = c.dL_dcolors; b.dL_dopacity = c.dL_dopacity;
    b.dL_dscales = c.dL_dscales; b.dL_drotations = c.dL_drotations;
    b.row_range = row_range;
    b.shs = shs; b.campos = shs ? ext->campos : nullptr; b.cov3D_precomp = cov3D_precomp;
    b.sh_degree = shs ? ext->sh_degree : 0u; b.sh_coeffs = shs ? ext->sh_coeffs : 0u;
    b.dL_dsh = shs ? ext->dL_dsh : nullptr; b.dL_dcov3D = cov3D_precomp ? ext->dL_dcov3D : nullptr;
    b.inst_ddepth = k.inst_ddepth;
    b.antialias = antialias ? 1 : 0;
    b.opacities = c.opacities;
    b.dop_in_record = ((flags & GSR_FLAG_COMPOSITE_TILES) && (flags & GSR_FLAG_NO_COLOR_GRAD)) ? 1 : 0;  // what k_composite_bwd_tiles<false> just wrote
    rc = stage("preprocess_bwd", GSR_STAGE_PREPROCESS_BWD, [&] { gsr_launch_preprocess_bwd(b, w.splats, w.goff, w.gprefix, w.inst_valid, w.inst_dop, w.inst_grad, w.hdr, s, c.cam); });
    if (rc == GPSGS_OK && dL_dfeatures)
        rc = stage("feature_grad_gather", GSR_STAGE_PREPROCESS_BWD,
                   [&] { gsr_launch_feature_grad_gather(P, F, row_range, c.radii, w.goff, w.gprefix, w.inst_valid, k.inst_dfeat, w.hdr, dL_dfeatures, s); });
    if (rc == GPSGS_OK && absgrad)  // (the flags the compositing backward set are cleared only by the next forward's compositing launch)
        rc = stage("absgrad_gather", GSR_STAGE_PREPROCESS_BWD,
                   [&] { gsr_launch_absgrad_gather(P, row_range, c.radii, w.goff, w.gprefix, w.inst_valid, k.inst_absgrad, w.hdr, absgrad, s); });
    return rc;
}

// gsr_backward_camera / _absgrad / _features: the camera arguments first -- misaligned outputs or a scratch slab too small for P are refused; c.cam is set when
// any of the three gradients is asked for and stays NULL otherwise (the call is then gsr_backward_ex)
int backward_with_camera(BackwardCall c, float *dL_dviewmatrix, float *dL_dprojmatrix, float *dL_dcampos, void *scratch, size_t scratch_bytes) {
    if (misaligned(dL_dviewmatrix, dL_dprojmatrix, dL_dcampos)) return GPSGS_E_INVALID;
    const GsrCamGrad cam = {static_cast<float *>(scratch), dL_dviewmatrix, dL_dprojmatrix, dL_dcampos};
    if (dL_dviewmatrix || dL_dprojmatrix || dL_dcampos) {
        if (c.P > 0 && (!scratch || scratch_bytes < gsr_camera_grad_scratch_bytes(c.P))) return GPSGS_E_WORKSPACE;
        c.cam = &cam;
    }
    return backward_impl(c);
}
}  // namespace

extern "C" int gsr_backward_ex(int P, int width, int height, const float *means3D, const float *colors, const float *opacities,
                               const float *scales, const float *rotations, float scale_modifier, float tanfovx, float tanfovy,
                               const float *viewmatrix, const float *projmatrix, const float *bg, const int *radii,
                               const float *dL_dpix, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dcolors, float *dL_dopacity,
                               float *dL_dscales, float *dL_drotations, void *workspace, size_t workspace_bytes,
                               int64_t instance_capacity, unsigned flags, void *stream, const GsrViewExt *ext) {
    return backward_impl({GSR_VIEW_CALL(ext), radii, dL_dpix, dL_dmeans3D, dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dscales, dL_drotations, nullptr, nullptr, nullptr, nullptr});
}

extern "C" int gsr_backward_camera(int P, int width, int height, const float *means3D, const float *colors, const float *opacities,
                                   const float *scales, const float *rotations, float scale_modifier, float tanfovx, float tanfovy,
                                   const float *viewmatrix, const float *projmatrix, const float *bg, const int *radii,
                                   const float *dL_dpix, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dcolors, float *dL_dopacity,
                                   float *dL_dscales, float *dL_drotations, void *workspace, size_t workspace_bytes,
                                   int64_t instance_capacity, unsigned flags, void *stream, const GsrViewExt *ext,
                                   float *dL_dviewmatrix, float *dL_dprojmatrix, float *dL_dcampos, void *scratch, size_t scratch_bytes) {
    return backward_with_camera({GSR_VIEW_CALL(ext), radii, dL_dpix, dL_dmeans3D, dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dscales, dL_drotations, nullptr, nullptr, nullptr, nullptr},
                                dL_dviewmatrix, dL_dprojmatrix, dL_dcampos, scratch, scratch_bytes);
}

extern "C" int gsr_backward_absgrad(int P, int width, int height, const float *means3D, const float *colors, const float *opacities,
                                    const float *scales, const float *rotations, float scale_modifier, float tanfovx, float tanfovy,
                                    const float *viewmatrix, const float *projmatrix, const float *bg, const int *radii,
                                    const float *dL_dpix, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dcolors, float *dL_dopacity,
                                    float *dL_dscales, float *dL_drotations, void *workspace, size_t workspace_bytes,
                                    int64_t instance_capacity, unsigned flags, void *stream, const GsrViewExt *ext,
                                    float *dL_dviewmatrix, float *dL_dprojmatrix, float *dL_dcampos, void *scratch, size_t scratch_bytes,
                                    const GsrAbsGrad *abs) {
    return backward_with_camera({GSR_VIEW_CALL(ext), radii, dL_dpix, dL_dmeans3D, dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dscales, dL_drotations, nullptr, nullptr, abs, nullptr},
                                dL_dviewmatrix, dL_dprojmatrix, dL_dcampos, scratch, scratch_bytes);
}

extern "C" int gsr_backward_distort(int P, int width, int height, const float *means3D, const float *colors, const float *opacities,
                                    const float *scales, const float *rotations, float scale_modifier, float tanfovx, float tanfovy,
                                    const float *viewmatrix, const float *projmatrix, const float *bg, const int *radii,
                                    const float *dL_dpix, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dcolors, float *dL_dopacity,
                                    float *dL_dscales, float *dL_drotations, void *workspace, size_t workspace_bytes,
                                    int64_t instance_capacity, unsigned flags, void *stream, const GsrViewExt *ext,
                                    float *dL_dviewmatrix, float *dL_dprojmatrix, float *dL_dcampos, void *scratch, size_t scratch_bytes,
                                    const GsrDistort *distort) {
    return backward_with_camera({GSR_VIEW_CALL(ext), radii, dL_dpix, dL_dmeans3D, dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dscales, dL_drotations, nullptr, nullptr, nullptr, distort},
                                dL_dviewmatrix, dL_dprojmatrix, dL_dcampos, scratch, scratch_bytes);
}

extern "C" int gsr_backward_features(int P, int width, int height, const float *means3D, const float *colors, const float *opacities,
                                     const float *scales, const float *rotations, float scale_modifier, float tanfovx, float tanfovy,
                                     const float *viewmatrix, const float *projmatrix, const float *bg, const int *radii,
                                     const float *dL_dpix, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dcolors, float *dL_dopacity,
                                     float *dL_dscales, float *dL_drotations, void *workspace, size_t workspace_bytes,
                                     int64_t instance_capacity, unsigned flags, void *stream, const GsrViewExt *ext,
                                     float *dL_dviewmatrix, float *dL_dprojmatrix, float *dL_dcampos, void *scratch, size_t scratch_bytes,
                                     const GsrFeatures *feat) {
    return backward_with_camera({GSR_VIEW_CALL(ext), radii, dL_dpix, dL_dmeans3D, dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dscales, dL_drotations, nullptr, feat, nullptr, nullptr},
                                dL_dviewmatrix, dL_dprojmatrix, dL_dcampos, scratch, scratch_bytes);
}

extern "C" int gsr_backward(int P, int width, int height, const float *means3D, const float *colors, const float *opacities,
                            const float *scales, const float *rotations, float scale_modifier, float tanfovx, float tanfovy,
                            const float *viewmatrix, const float *projmatrix, const float *bg, const int *radii,
                            const float *dL_dpix, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dcolors, float *dL_dopacity,
                            float *dL_dscales, float *dL_drotations, void *workspace, size_t workspace_bytes,
                            int64_t instance_capacity, unsigned flags, void *stream) {
    return backward_impl({GSR_VIEW_CALL(nullptr), radii, dL_dpix, dL_dmeans3D, dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dscales, dL_drotations, nullptr, nullptr, nullptr, nullptr});
}
#undef GSR_VIEW_CALL

extern "C" int gsr_mark_visible(int P, const float *means3D, const float *viewmatrix, const float *projmatrix, uint8_t *present, void *stream) {
    (void)projmatrix;  // upstream's in_frustum() projects the point too, but tests only the view-space depth
    if (P < 0 || (P > 0 && (!means3D || !viewmatrix || !present))) return GPSGS_E_INVALID;
    gsr_launch_mark_visible(P, means3D, viewmatrix, present, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? GPSGS_OK : GPSGS_E_LAUNCH;
}

extern "C" int gsr_selftest(float *out4_device, void *stream) {
    if (!out4_device) return GPSGS_E_INVALID;
    gsr_launch_selftest(out4_device, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? GPSGS_OK : GPSGS_E_LAUNCH;
}

// ---- shader-clock measurement (diagnostic): s_memtime ticks once per shader cycle, wall_clock64() at the constant rate the runtime reports
// (hipDeviceAttributeWallClockRate); a chip-filling grid of dependent FMAs runs for a few milliseconds and wave 0 brackets itself with both.
namespace {
__global__ __launch_bounds__(256) void k_sclk(unsigned long long *out, int iters) {
    float a = (float)threadIdx.x * 1e-3f, b = 1.0001f;
    const unsigned long long w0 = wall_clock64(), c0 = clock64();
    for (int i = 0; i < iters; i++) {
#pragma unroll
        for (int u = 0; u < 8; u++) a = __builtin_fmaf(a, b, 1e-7f);
    }
    const unsigned long long c1 = clock64(), w1 = wall_clock64();
    if (blockIdx.x == 0 && threadIdx.x == 0) { out[0] = c1 - c0; out[1] = w1 - w0; }
    if (a == 123.456f) out[2] = 1ull;  // keeps the loop alive
}
}  // namespace

extern "C" int gpsgs_measure_sclk(unsigned long long *scratch3_device, double *mhz_host, void *stream) {
    if (!scratch3_device || !mhz_host) return GPSGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    int dev = 0, rate_khz = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || rate_khz <= 0)
        return GPSGS_E_NO_DEVICE;
    hipLaunchKernelGGL(k_sclk, dim3(2048), dim3(256), 0, s, scratch3_device, 60000);
    unsigned long long h[2] = {0ull, 0ull};
    if (hipMemcpyAsync(h, scratch3_device, sizeof(h), hipMemcpyDeviceToHost, s) != hipSuccess) return GPSGS_E_LAUNCH;
    if (hipStreamSynchronize(s) != hipSuccess) return GPSGS_E_LAUNCH;
    if (h[1] == 0ull) return GPSGS_E_LAUNCH;
    *mhz_host = (double)h[0] / (double)h[1] * (double)rate_khz * 1e-3;
    return GPSGS_OK;
}

extern "C" int gsr_debug_set_wg_trace(unsigned long long *rows_device) { return gsr_set_wg_trace(rows_device) == 0 ? GPSGS_OK : GPSGS_E_LAUNCH; }

extern "C" int gsr_debug_count_records(const void *workspace, size_t workspace_bytes, int P, int width, int height, int64_t instance_capacity, uint32_t bin_capacity,
                                       unsigned long long *out2_device, void *stream) {
    if (!workspace || !out2_device || P < 0 || width <= 0 || height <= 0 || instance_capacity < 0) return GPSGS_E_INVALID;
    if (bin_capacity && !gsr_direct_lists_ok(width, height, bin_capacity)) return GPSGS_E_INVALID;
    const GsrLayout L = gsr_layout(P, width, height, instance_capacity, bin_capacity);
    if (workspace_bytes < L.total) return GPSGS_E_WORKSPACE;  // a forward-only workspace has no record flags (they lie beyond its end)
    const GsrWorkspace w = gsr_workspace_map(const_cast<void *>(workspace), L, true);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(out2_device, 0, 16, s) != hipSuccess) return GPSGS_E_LAUNCH;
    hipLaunchKernelGGL(k_count_flags, dim3(1024), dim3(256), 0, s, w.inst_valid, w.hdr, out2_device);
    return hipGetLastError() == hipSuccess ? GPSGS_OK : GPSGS_E_LAUNCH;
}

extern "C" int gsr_timing_read(float *ms_sum_host, int *launches_host) {
    if (!ms_sum_host || !launches_host) return GPSGS_E_INVALID;
    for (int i = 0; i < GSR_STAGE_COUNT; i++) { ms_sum_host[i] = 0.f; launches_host[i] = 0; }
    if (hipDeviceSynchronize() != hipSuccess) return GPSGS_E_LAUNCH;
    for (int i = 0; i < g_rec.n; i++) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, g_rec.ev[i][0], g_rec.ev[i][1]) != hipSuccess) continue;
        ms_sum_host[g_rec.stage[i]] += ms;
        launches_host[g_rec.stage[i]] += 1;
    }
    g_rec.n = 0;
    return GPSGS_OK;
}

extern "C" int gsr_copy_header_async(const void *workspace, void *host_pinned_out, void *stream) {
    if (!workspace || !host_pinned_out) return GPSGS_E_INVALID;
    return hipMemcpyAsync(host_pinned_out, workspace, 32, hipMemcpyDeviceToHost, (hipStream_t)stream) == hipSuccess ? GPSGS_OK : GPSGS_E_LAUNCH;
}

extern "C" int gsr_read_header(const void *workspace, GsrHeader *host_out, void *stream) {
    if (!workspace || !host_out) return GPSGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(host_out, workspace, sizeof(GsrHeader), hipMemcpyDeviceToHost, s) != hipSuccess) return GPSGS_E_LAUNCH;
    if (hipStreamSynchronize(s) != hipSuccess) return GPSGS_E_LAUNCH;
    return GPSGS_OK;
}

extern "C" int gsr_export_state(const void *workspace, int P, int width, int height, int64_t instance_capacity, uint32_t bin_capacity, float *depth, float *xy,
                                float *conic_opacity, int *rect, int64_t *tile_ranges, uint32_t *point_list, float *final_T,
                                uint32_t *n_contrib, void *stream) {
    if (!workspace || P < 0 || width <= 0 || height <= 0) return GPSGS_E_INVALID;
    if (bin_capacity && !gsr_direct_lists_ok(width, height, bin_capacity)) return GPSGS_E_INVALID;
    const GsrLayout L = gsr_layout(P, width, height, instance_capacity, bin_capacity);
    const GsrWorkspace w = gsr_workspace_map(const_cast<void *>(workspace), L, false);
    hipStream_t s = (hipStream_t)stream;
    const int n = P > L.NB ? P : L.NB;
    if (n > 0) hipLaunchKernelGGL(k_export, dim3((n + 255) / 256), dim3(256), 0, s, P, L.NB, w.splats, w.bins, depth, xy, conic_opacity, rect, tile_ranges);
    const size_t npix = (size_t)width * height;
    if (point_list && L.key_cap > 0)  // point_list [key capacity]: the instance capacity, or bins x bin_capacity (direct lists: every bin's segment, gaps included)
        (void)hipMemcpyAsync(point_list, w.point_list, (size_t)L.key_cap * 4, hipMemcpyDeviceToDevice, s);
    if (final_T) (void)hipMemcpyAsync(final_T, w.final_T, npix * 4, hipMemcpyDeviceToDevice, s);
    if (n_contrib) (void)hipMemcpyAsync(n_contrib, w.n_contrib, npix * 4, hipMemcpyDeviceToDevice, s);
    return hipGetLastError() == hipSuccess ? GPSGS_OK : GPSGS_E_LAUNCH;
}
