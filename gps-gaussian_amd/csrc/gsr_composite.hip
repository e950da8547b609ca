// gsr_composite.hip -- forward and backward alpha compositing for gfx950: ONE wave64 per 8x8-pixel bin.
//
// Semantics: SURVEY.md section 9.2 (front-to-back blend with the power>0 / alpha<1/255 / T<1e-4 rules) and section 9.3 (back-to-
// front gradient recurrence); replaces upstream renderCUDA forward/backward (called through
// /root/reference/gaussian_renderer/__init__.py:54-62 and its autograd backward).
//
// CDNA4 mapping:
//   * lane = pixel of an 8x8 bin; every workgroup is ONE wave, so the dispatcher balances the CUs at wave granularity
//     (4-wave workgroups packed greedily left CUs with 7 busy workgroups next to CUs with 4).  There is no
//     __syncthreads anywhere: a wave that finishes early (all pixels saturated) stops fetching immediately;
//   * per round a wave stages 64 splat records {x,y,A,B | C,op,r,g | b} -- colour included -- with one 48-byte gather
//     per lane into its private LDS slice; the gather for round i+1 is issued BEFORE round i is consumed (registers),
//     so HBM/L2 latency hides under the blend loop; the blend loop reads wave-uniform LDS addresses (broadcast);
//   * lists are exact-extent culled per bin (gsr_common.h), so a wave never iterates a splat that cannot touch it; bins
//     are taken from the work-ordered list in an XCD-aware order (xcd_list_pos) so that neighbouring bins share an L2;
//   * backward: the 9 per-(pixel, splat) gradient terms are summed across the wave with a butterfly reduce-scatter
//     (v_permlane32/16_swap + DPP, 22 instructions instead of 54, no LDS traffic), parked per staged splat in LDS by
//     12 lanes and flushed once per round as one 32-byte record + dL/dopacity + flag per INSTANCE, at the instance's Gaussian-major
//     slot (gsr_common.h).  There is no global atomic in the backward at all (upstream issues 10 per (pixel, splat); float
//     atomics run at only 20-30 Mops/ms on MI355X): k_preprocess_bwd streams each Gaussian's slots in a fixed order, so
//     gradients are also bit-reproducible.
// This file is the VALU-only kernel family (GPSGS_COMPOSITE=valu); the default family takes the exponents from matrix-core tiles
// (gsr_composite_tiles.hip).
#include "gsr_composite_common.h"

namespace {

// ---- walk rules that the forward and backward kernels must take identically, each written once.  The pieces take and return VALUES, never references
// to a kernel's locals: a local whose address is taken is allocated differently, and instruction order and register use then change.
// Staging: lane `lane` puts its fetched record into the wave's LDS slice, the conic pre-scaled for gsr_power2
__device__ __forceinline__ void stage_record(float4 *wA, float4 *wB, int lane, float4 nA, float4 nB) {
    wA[lane] = make_float4(nA.x, nA.y, -0.5f * GSR_LOG2E * nA.z, -GSR_LOG2E * nA.w);
    wB[lane] = make_float4(-0.5f * GSR_LOG2E * nB.x, nB.y, nB.z, nB.w);
}
template <bool EXTRA>
__device__ __forceinline__ void stage_record(float4 *wA, float4 *wB, float *wC, float *wD, int lane, float4 nA, float4 nB, float nC, float nD) {
    stage_record(wA, wB, lane, nA, nB);
    wC[lane] = nC;
    if (EXTRA) wD[lane] = nD;
}

// CONTRIB prefetch of k_composite_fwd: list entry `pos` of bin (bin_x, bin_y), its record and its instance's slot.  By reference ON PURPOSE, the one exception
// to the rule above: only in this form do these two instantiations compile to the code they had before the rules were shared (by value: 4 more v_mov_b32).
template <bool EXTRA>
__device__ __forceinline__ void load_record_slot(const GsrSplat *splats, const uint32_t *point_list, const uint32_t *goff, const uint32_t *gpart, int bin_x,
                                                     int bin_y, uint32_t pos, float4 &nA, float4 &nB, float &nC, float &nD, uint32_t &nRec) {
    const uint32_t id = point_list[pos];
    const SplatRec r = load_record(splats, id);
    nA = r.A; nB = r.B; nC = r.C.x;
    if (EXTRA) nD = r.C.y;
    nRec = inst_slot(goff, gpart, id, r.C, bin_x, bin_y);
}

// Forward decision for one (pixel, staged splat {a, b}) pair: a pixel that is still active skips the splat if power > 0 or alpha < 1/255, saturates
// (leaves `active`, without blending it) if T (1 - alpha) < 1e-4, and blends it otherwise.
struct FwdPair {
    float w, test_T;              // the blend weight alpha T (0 where nothing is blended) and T behind the splat
    bool use;                     // this pixel blends the splat
    lanemask_t blended, active;   // the pixels that blend it, and those still active behind it
};
__device__ __forceinline__ FwdPair fwd_pair(float4 a, float4 b, float pxf, float pyf, float T, lanemask_t active) {
    FwdPair p;
    const float dx = a.x - pxf, dy = a.y - pyf;
    const float power = gsr_power2(a.z, a.w, b.x, dx, dy);
    const float alpha = fminf(0.99f, b.y * __builtin_amdgcn_exp2f(power));
    const lanemask_t valid = active & ~(__ballot(power > 0.f) | __ballot(alpha < 1.f / 255.f));
    p.test_T = __builtin_fmaf(-alpha, T, T);  // T (1 - alpha), one rounding
    const lanemask_t sat = __ballot(p.test_T < 0.0001f);
    p.active = active & ~(valid & sat);
    p.blended = valid & ~sat;
    p.use = __builtin_amdgcn_inverse_ballot_w64(p.blended);
    p.w = p.use ? alpha * T : 0.f;
    return p;
}

// Backward decision for the pair (pixel, staged splat {a, b} at 0-based list position pos): the pairs the forward blended are those in front of
// the pixel's last contributor that pass the forward's two skips (same arithmetic, same bits)
struct BwdPair { float dx, dy, G, alpha; lanemask_t valid_m; };  // valid_m: the pixels that blended this splat; 0: the wave skips it
__device__ __forceinline__ BwdPair bwd_pair(float4 a, float4 b, float pxf, float pyf, uint32_t pos, uint32_t last) {
    BwdPair p;
    p.dx = a.x - pxf; p.dy = a.y - pyf;
    const float power = gsr_power2(a.z, a.w, b.x, p.dx, p.dy);
    p.G = __builtin_amdgcn_exp2f(power);
    p.alpha = fminf(0.99f, b.y * p.G);
    p.valid_m = __ballot(pos < last) & ~(__ballot(power > 0.f) | __ballot(p.alpha < 1.f / 255.f));
    return p;
}

// The backward's recurrence for one pair the wave did not skip, in four straight-line pieces; what an option adds to cd (the features' fd, DISTORT's
// channel) and w = ae T sit between them at the call site.
// Branch-free: a lane this splat does not reach (behind its last contributor, power > 0, alpha < 1/255) runs the same arithmetic with alpha = 0 and
// G = 0: rcp(1) = 1 leaves T, bwd_alpha leaves A (0 * cd + 1 * A), and every sum receives an exact zero.
struct BwdStep { float Ge, ae, om, rcp, T; };  // T: in front of the splat
__device__ __forceinline__ BwdStep bwd_step(bool valid, float G, float alpha, float T) {
    const float Ge = valid ? G : 0.f, ae = valid ? alpha : 0.f, om = 1.f - ae, rcp = __builtin_amdgcn_rcpf(om);
    return {Ge, ae, om, rcp, T * rcp};
}
// cd = colour . dL/dpixel of staged splat j {b, wC[j] (, wD[j])}.  Takes the wave's LDS pointers and j, NOT the loaded values (those reorder k_composite_bwd_feat)
template <bool EXTRA>
__device__ __forceinline__ float bwd_colour_dot(float4 b, const float *wC, const float *wD, int j, float d0, float d1, float d2, float dd, float da) {
    float cd = b.z * d0 + b.w * d1 + wC[j] * d2;
    if (EXTRA) {
        // the two extra channels' share of cd, rounded like a colour channel's product-then-accumulate (no fma of z dd + da)
#pragma clang fp contract(off)
        const float zd = wD[j] * dd;
        cd = cd + (zd + da);
    }
    return cd;
}
// Upstream carries accum_rec (the colour seen behind the splat, 3 channels) with last_alpha / last_color; only its dot product with dL/dpixel is ever
// used, so the recurrence is carried on that scalar: A <- alpha cd + (1 - alpha) A.  Same order of operations back to front (no cancellation), 14
// instead of 23 instructions, and nothing but T and A is carried from splat to splat.  nTb = -T_final (bg . dL/dpixel)
struct BwdAlpha { float dL_dalpha, A; };
__device__ __forceinline__ BwdAlpha bwd_alpha(float cd, float A, float T, float nTb, float rcp, float ae, float om) {
    return {(cd - A) * T + nTb * rcp, ae * cd + om * A};
}
// Per pair only the colour terms and six MOMENTS of s = dL/dG * G are formed: S0 = sum s, Sx = sum s dx, Sy, Sxx, Sxy, Syy.  dL/dmean2D, dL/dconic and
// dL/dopacity are linear in them and are finished once per (bin, splat) at flush time (11 fewer instructions per pair than the nine upstream terms here).
struct BwdMom { float m_0, m_x, m_y, m_xx, m_xy, m_yy; };
__device__ __forceinline__ BwdMom bwd_moments(float op, float dL_dalpha, float Ge, float dx, float dy) {
    const float m_0 = (op * dL_dalpha) * Ge;  // s = dL/dG * G, with dL/dG = opacity * dL/dalpha straight through the 0.99 clamp
    const float m_x = m_0 * dx, m_y = m_0 * dy;
    return {m_0, m_x, m_y, m_x * dx, m_x * dy, m_y * dy};
}

// Flush: lane j turns staged splat j's parked sums into ONE 32-byte instance record + its dL/dopacity (+ EXTRA: dL/dz), at the
// instance's SLOT `rec` (Gaussian-major; gsr_common.h); no atomics.  REC = float4s per staged splat in wAcc.  The caller sets the slot's flag last.
// dG/d(delta) = -G (A dx + B dy), -G (C dy + B dx);  dL/dconic = -0.5 s {dx^2, dx dy, dy^2};  dL/dop = G dL/dalpha = s / op
// the staged conic is pre-scaled: A = sa.z / (-0.5 log2 e), B = sa.w / (-log2 e), C = sb.x / (-0.5 log2 e)
constexpr float GSR_KA = 2.f / GSR_LOG2E, GSR_KB = 1.f / GSR_LOG2E;
template <bool EXTRA>
__device__ __forceinline__ void flush_record(const float4 *wAcc, int REC, const float4 *wA, const float4 *wB, int lane, float ddelx_dx, float ddely_dy,
                                             uint32_t rec, GsrGradAcc *inst_grad, float *inst_dop, float *inst_ddepth) {
    const float4 v0 = wAcc[REC * lane], v1 = wAcc[REC * lane + 1], rs = wAcc[REC * lane + 2];
    const float4 sa = wA[lane], sb = wB[lane];  // this lane staged splat `lane` itself: conic (sa.z, sa.w, sb.x), opacity sb.y
    const float Sx = v0.w, Sy = v1.x, Sxx = v1.y, Sxy = v1.z, Syy = v1.w;
    const float S0 = (rs.x + rs.y) + (rs.z + rs.w);  // arrives as 4 row sums
    const float g_mx = ddelx_dx * (GSR_KA * sa.z * Sx + GSR_KB * sa.w * Sy);
    const float g_my = ddely_dy * (GSR_KA * sb.x * Sy + GSR_KB * sa.w * Sx);
    float4 *dst = reinterpret_cast<float4 *>(inst_grad + rec);  // one whole 32-byte sector
    dst[0] = make_float4(v0.x, v0.y, v0.z, g_mx);
    dst[1] = make_float4(g_my, -0.5f * Sxx, -0.5f * Sxy, -0.5f * Syy);
    inst_dop[rec] = S0 * __builtin_amdgcn_rcpf(sb.y);
    if (EXTRA) {
        const float4 rz = wAcc[REC * lane + 3];
        inst_ddepth[rec] = (rz.x + rz.y) + (rz.z + rz.w);
    }
}

// ---- per-Gaussian contribution statistics (GsrContrib): a max / sum reduce-scatter of eight values ------------------------------------------
// The forward's CONTRIB instantiation reduces the 64 per-lane weights of each staged splat to a wave sum and a wave max.  Eight splats (one
// blend group) go through one butterfly reduce-scatter per operation, wave_reduce_scatter9's first 18 instructions: value k ends in every lane
// of one 8-lane group (acc_slot(lane) for lanes 0, 8, .., 56).  Max is exact; the sum's order is fixed, so both have the same bits on every run.
// The weights are never negative or NaN (+0 where nothing is blended), so their max is the max of their bit patterns: one v_max_u32 per step
// (fmaxf costs two canonicalising v_max_f32 on top).
template <bool MAX>
__device__ __forceinline__ float rs_op(float a, float b) {
    return MAX ? __uint_as_float(max(__float_as_uint(a), __float_as_uint(b))) : a + b;
}
template <bool MAX, int CTRL>
__device__ __forceinline__ float dpp_op_row(float v) {
    const int t = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true);
    return rs_op<MAX>(v, __int_as_float(t));
}
template <bool MAX>
__device__ __forceinline__ float wave_reduce_scatter8(const float (&v)[8], bool upper8) {
    auto swap32 = [](float a, float b) {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
        return rs_op<MAX>(__uint_as_float(r[0]), __uint_as_float(r[1]));
    };
    auto swap16 = [](float a, float b) {
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
        return rs_op<MAX>(__uint_as_float(r[0]), __uint_as_float(r[1]));
    };
    const float u0 = swap32(v[0], v[1]), u1 = swap32(v[2], v[3]);
    const float u2 = swap32(v[4], v[5]), u3 = swap32(v[6], v[7]);
    const float t0 = swap16(u0, u1), t1 = swap16(u2, u3);
    const float keep = upper8 ? t1 : t0, send = upper8 ? t0 : t1;
    const int sw = __builtin_amdgcn_update_dpp(0, __float_as_int(send), 0x128, 0xF, 0xF, true);  // row_ror:8
    float r = rs_op<MAX>(keep, __int_as_float(sw));
    r = dpp_op_row<MAX, 0x141>(r);  // row_half_mirror
    r = dpp_op_row<MAX, 0x1B>(r);   // quad_perm [3,2,1,0]
    r = dpp_op_row<MAX, 0xB1>(r);   // quad_perm [1,0,3,2]
    return r;
}

// EXTRA: the opt-in depth and alpha maps (GsrViewExt.out_depth / out_alpha) -- two more channels of the same blend, background 0:
// depth = sum z_i alpha_i T_i (z_i = the view-space depth in the splat record's `depth` slot), alpha = sum alpha_i T_i.  The record already carries
// z next to b, so the gather is the same 48-byte record; only one LDS word per staged splat and two accumulators are added.
// CONTRIB: the per-instance contribution statistics (GsrContrib) -- for every staged splat the sum and the max of its 64 weights w = alpha T and the
// number of pixels it is blended into.  The count is the popcount of the blended-lane ballot (scalar), selected into lane j of a register; the sum and
// max go through wave_reduce_scatter8 once per blend group of eight splats and are parked in LDS.  Once per round lane j writes staged splat j's
// {sum, max, count, 0} to inst_contrib[slot] -- the instance's Gaussian-major slot, as the backward's records -- if the splat was blended anywhere.
// Slots nobody writes (not walked, nothing blended, bin-rect cells outside the list) were zeroed by k_contrib_clear in front of this launch.
// DISTORT (on top of EXTRA): the opt-in depth-distortion map (GsrDistort), sum_i sum_j w_i w_j |z_i - z_j| = 2 sum_i w_i (z_i A_<i - D_<i) with the prefix
// sums A_<i = sum_{j<i} w_j, D_<i = sum_{j<i} w_j z_j of the list order (the list is sorted by the same fp32 depth).  The depths are taken relative to
// the depth of the bin list's first entry (wave-uniform): the sum does not change under a shift of z, and z A - D then has the size of the depth spread
// instead of cancelling two numbers of the size of z.  One accumulator and one FMA pair per blended pair; the per-pixel totals {sum w, sum w (z - z0)}
// go to the caller's [2, H, W] plane for the backward, which reads these very numbers (not the public depth / alpha maps).
template <bool EXTRA, bool CONTRIB = false, bool DISTORT = false>
__global__ __launch_bounds__(64 * WAVES) void k_composite_fwd(int W, int H, int bx, const GsrSplat *__restrict__ splats,
                                                       GsrBins bins, const uint32_t *__restrict__ wg_order,
                                                       const uint32_t *__restrict__ point_list, const float *__restrict__ bg,
                                                       float *__restrict__ out_color, float *__restrict__ final_T,
                                                       uint32_t *__restrict__ n_contrib, const GsrHeader *__restrict__ hdr, uint8_t *__restrict__ inst_valid,
                                                       float *__restrict__ out_depth, float *__restrict__ out_alpha,
                                                       const uint32_t *__restrict__ goff = nullptr, const uint32_t *__restrict__ gpart = nullptr,
                                                       float4 *__restrict__ inst_contrib = nullptr, float *__restrict__ out_distort = nullptr,
                                                       float *__restrict__ totals = nullptr) {
    static_assert(!DISTORT || EXTRA, "DISTORT reads the staged depths of EXTRA");
    __shared__ float4 sA[WAVES][WAVE];
    __shared__ float4 sB[WAVES][WAVE];
    __shared__ float sC[WAVES][WAVE];
    __shared__ float sD[WAVES][EXTRA ? WAVE : 1];
    __shared__ float sS[WAVES][CONTRIB ? WAVE : 1], sM[WAVES][CONTRIB ? WAVE : 1];  // CONTRIB: per staged splat, the wave sum and max of w
    const uint32_t list_pos = xcd_list_pos(blockIdx.x, hdr->num_busy_wgs);
    const WaveGeom g = wave_geom(W, H, bx, bins, wg_order, list_pos);
    if (hdr->overflow) {  // nothing can be rendered from truncated lists: a deterministic zero image instead of uninitialised memory
        fwd_write_blank<EXTRA>(g, W, H, out_color, final_T, n_contrib, out_depth, out_alpha);
        if (DISTORT && g.inside) {  // a zero map (the backward of an overflowed view does nothing: the totals are zeroed only for tidiness)
            const size_t npix = (size_t)W * H, q = (size_t)g.py * W + g.px;
            out_distort[q] = 0.f;
            totals[q] = 0.f;
            totals[npix + q] = 0.f;
        }
        return;
    }
    clear_record_flags(inst_valid, hdr, (int)threadIdx.x, 64 * WAVES);
    const float pxf = (float)g.px, pyf = (float)g.py;
    float4 *wA = sA[g.wid], *wB = sB[g.wid];
    float *wC = sC[g.wid], *wD = sD[g.wid];

    float T = 1.f, C0 = 0.f, C1 = 0.f, C2 = 0.f, CD = 0.f, CA = 0.f;
    float DI = 0.f, DS = 0.f;  // DISTORT: sum_i w_i (zs_i A_<i - DS_<i) and DS = sum w zs, zs = z - z0
    uint32_t last = 0;      // 1-based list position of the last splat that contributed (n_contrib), up to the previous round
    uint32_t last_rnd = 0;  // ... 1-based slot of the last contributor inside the current round (0: none): an inline constant per select
    lanemask_t active = __ballot(g.inside);  // pixels inside the image that are not yet saturated
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)g.r0), r1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)g.r1);
    float z0 = 0.f;  // DISTORT: the reference depth, the bin list's first entry's (wave-uniform; the backward takes the same)
    if constexpr (DISTORT) {
        if (r0 < r1) z0 = load_record(splats, point_list[r0]).C.y;
    }

    float4 nA = make_float4(0.f, 0.f, 0.f, 0.f), nB = nA;
    float nC = 0.f, nD = 0.f;
    uint32_t nRec = 0;  // CONTRIB: the slot of this lane's prefetched instance, as the backward forms it
    if constexpr (CONTRIB) {
        if (r0 + g.lane < r1) load_record_slot<EXTRA>(splats, point_list, goff, gpart, g.bin % bx, g.bin / bx, r0 + g.lane, nA, nB, nC, nD, nRec);  // prefetch round 0
    } else if (r0 + g.lane < r1) {  // prefetch round 0
        const SplatRec r = load_record(splats, point_list[r0 + g.lane]);
        nA = r.A; nB = r.B; nC = r.C.x;
        if (EXTRA) nD = r.C.y;
    }
    for (uint32_t base = r0; base < r1; base += WAVE) {
        if (active == 0ull) break;  // every pixel of this bin is saturated (or outside the image)
        wave_sync_lds();            // previous round fully consumed
        stage_record<EXTRA>(wA, wB, wC, wD, g.lane, nA, nB, nC, nD);
        const uint32_t curRec = nRec;
        wave_sync_lds();
        const uint32_t nk = base + WAVE + g.lane;
        nB.y = 0.f;  // a slot without a splat blends nothing (opacity 0 -> alpha 0 < 1/255; stale x, y, conic stay finite)
        if constexpr (CONTRIB) {
            if (nk < r1) load_record_slot<EXTRA>(splats, point_list, goff, gpart, g.bin % bx, g.bin / bx, nk, nA, nB, nC, nD, nRec);  // prefetch the next round
        } else if (nk < r1) {  // prefetch the next round while this one is blended
            const SplatRec r = load_record(splats, point_list[nk]);
            nA = r.A; nB = r.B; nC = r.C.x;
            if (EXTRA) nD = r.C.y;
        }
        const int cnt = (int)min((uint32_t)WAVE, r1 - base);
        uint32_t n_blend = 0;  // CONTRIB: lane j = the number of pixels staged splat j was blended into (0 for a group that was not walked)
        // Branch-free blend in groups of 8 (the tail group is padded by opacity-0 slots; 4 and 16 measured slower); between groups one
        // scalar test stops the round as soon as all 64 pixels are saturated -- on average half a round (~8 % of a body bin's list) is
        // not walked at all
#pragma unroll
        for (int j0 = 0; j0 < WAVE; j0 += 8) {
            if (j0 < cnt && active != 0ull) {
                float wv[8];  // CONTRIB: the group's weights
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int j = j0 + u;
                    const float4 a = wA[j];
                    const float4 b = wB[j];
                    const float c2 = wC[j];
                    const FwdPair p = fwd_pair(a, b, pxf, pyf, T, active);
                    active = p.active;
                    const float w = p.w;
                    C0 += b.z * w;
                    C1 += b.w * w;
                    C2 += c2 * w;
                    if constexpr (DISTORT) {  // in front of CA's update: the prefix sums exclude the pair itself (w = 0 adds exact zeros: every operand is finite)
                        const float zs = wD[j] - z0;
                        DI = __builtin_fmaf(w, __builtin_fmaf(zs, CA, -DS), DI);
                        DS = __builtin_fmaf(zs, w, DS);
                    }
                    if (EXTRA) {
                        CD += wD[j] * w;  // the same contraction as a colour channel: fma(z, w, CD)
                        CA += w;          // alpha as the sum of the weights (its gradient then follows the colour recurrence), not 1 - T
                    }
                    if constexpr (CONTRIB) {
                        wv[u] = w;
                        const uint32_t nb = (uint32_t)__builtin_popcountll(p.blended);  // (scalar)
                        n_blend = __builtin_amdgcn_inverse_ballot_w64(1ull << j) ? nb : n_blend;  // lane j takes it
                    }
                    T = p.use ? p.test_T : T;
                    last_rnd = p.use ? (uint32_t)(j + 1) : last_rnd;
                }
                if constexpr (CONTRIB) {
                    const bool upper8 = (g.lane & 8) != 0;
                    const float ws = wave_reduce_scatter8<false>(wv, upper8), wm = wave_reduce_scatter8<true>(wv, upper8);
                    if ((g.lane & 7) == 0) {
                        const int k = j0 + acc_slot(g.lane);
                        sS[g.wid][k] = ws;
                        sM[g.wid][k] = wm;
                    }
                }
            }
        }
        last = last_rnd ? (base - r0) + last_rnd : last;
        last_rnd = 0;
        if constexpr (CONTRIB) {
            wave_sync_lds();
            if (n_blend != 0u) inst_contrib[curRec] = make_float4(sS[g.wid][g.lane], sM[g.wid][g.lane], __uint_as_float(n_blend), 0.f);
        }
    }
    if (g.inside) {
        const size_t npix = (size_t)W * H, q = (size_t)g.py * W + g.px;
        final_T[q] = T;
        n_contrib[q] = last;
        // a view WITHOUT Gaussians is upstream's zero-initialised image, not the background (it skips every kernel when P == 0); with a
        // row range the host does not know the count, so the rule is applied here (wave-uniform scalar load)
        const float bgs = hdr->num_points != 0u ? 1.f : 0.f;
        out_color[q] = C0 + T * (bgs * bg[0]);
        out_color[npix + q] = C1 + T * (bgs * bg[1]);
        out_color[2 * npix + q] = C2 + T * (bgs * bg[2]);
        if (EXTRA) {  // background 0 (a view without Gaussians gives 0 too: CD = CA = 0)
            if (out_depth) out_depth[q] = CD;
            if (out_alpha) out_alpha[q] = CA;
        }
        if constexpr (DISTORT) {  // (a view without Gaussians gives 0: DI = CA = DS = 0)
            out_distort[q] = 2.f * DI;
            totals[q] = CA;
            totals[npix + q] = DS;
        }
    }
}

// EXTRA: the depth / alpha channels' upstream gradients (either may be NULL = zero).  They enter the scalar recurrence as a colour channel with
// c = z resp. c = 1 and background 0 would: cd gains z dL/ddepth + dL/dalpha, so dL/dalpha_i -- and with it dL/dopacity, dL/dconic, dL/dmean2D
// -- folds into the existing record's sums.  The tenth per-(pixel, splat) term, dL/dz_i = sum_p w dL/ddepth, is row-reduced (4 DPP adds) beside
// the nine-term reduce-scatter; its 4 row sums are parked in a fourth float4 per staged splat and flushed as inst_ddepth[slot] (no atomics).
// ABSGRAD: the opt-in absolute screen-space gradient (GsrAbsGrad) -- per (pixel, splat) pair the magnitudes of the two terms whose signed sums are
// dL/dmean2D, |s (A dx + B dy)| and |s (C dy + B dx)| with s = m_0.  Both go through ONE register: v_permlane32_swap folds the wave's halves (lanes
// 0-31 then hold the x term, lanes 32-63 the y term; |.| is an input modifier of that add), four DPP adds make the row sums, and the two row sums per
// component are parked in one more float4 per staged splat.  The flush lane adds them, scales by 0.5 W (2 / log2 e) resp. 0.5 H (2 / log2 e) once and
// writes one float2 to inst_absgrad[slot], next to the record -- which, with inst_dop, inst_ddepth and the flag, is written exactly as without it.
// DISTORT (on top of EXTRA): the distortion map's upstream gradient g.  Walking back to front with the suffix sums behind the pair, d dist / d w_i =
// 2 [zs_i (A_tot - 2 A_>i) - (D_tot - 2 D_>i)] (the pair's own w cancels) enters cd like one more colour channel whose value differs per pixel, so
// dL/dopacity, dL/dmean2D and dL/dconic follow through the scalar recurrence; g d dist / d z_i = 2 g w_i (A_tot - 2 A_>i - w_i) joins w dL/ddepth in
// the row-summed dL/dz.  A_tot, D_tot are the forward's own totals (depths relative to the bin list's first entry, as there); the two carried values
// are U_A = A_tot - 2 A_>i and U_D = D_tot - 2 D_>i.  With g = 0 every term is an exact zero.
template <bool EXTRA, bool ABSGRAD = false, bool DISTORT = false>
__global__ __launch_bounds__(64 * WAVES) void k_composite_bwd(int W, int H, int bx, const GsrSplat *__restrict__ splats,
                                                       GsrBins bins, const uint32_t *__restrict__ wg_order,
                                                       const uint32_t *__restrict__ point_list, const float *__restrict__ bg,
                                                       const float *__restrict__ dL_dpix, const float *__restrict__ final_T,
                                                       const uint32_t *__restrict__ n_contrib, const uint32_t *__restrict__ goff,
                                                       const uint32_t *__restrict__ gpart, uint8_t *__restrict__ inst_valid, float *__restrict__ inst_dop,
                                                       GsrGradAcc *__restrict__ inst_grad, const GsrHeader *__restrict__ hdr,
                                                       const float *__restrict__ dL_ddepth, const float *__restrict__ dL_dalpha, float *__restrict__ inst_ddepth,
                                                       float2 *__restrict__ inst_absgrad = nullptr, const float *__restrict__ dL_ddistort = nullptr,
                                                       const float *__restrict__ totals = nullptr) {
    static_assert(!DISTORT || EXTRA, "DISTORT reads the staged depths of EXTRA and writes inst_ddepth");
    constexpr int AB = EXTRA ? 4 : 3;              // ABSGRAD: the float4 of the absolute sums
    constexpr int REC = AB + (ABSGRAD ? 1 : 0);    // float4s per staged splat in sAcc
    __shared__ float4 sA[WAVES][WAVE];
    __shared__ float4 sB[WAVES][WAVE];
    __shared__ float sC[WAVES][WAVE];
    __shared__ float sD[WAVES][EXTRA ? WAVE : 1];
    // per staged splat: {dr,dg,db,dmx | dmy,cxx,cxy,cyy | 4 row sums of dop (| 4 row sums of dz) (| 2 row sums of |t_x|, 2 of |t_y|)}
    __shared__ float4 sAcc[WAVES][WAVE * REC];
    if (hdr->overflow) return;
    const uint32_t list_pos = xcd_list_pos(blockIdx.x, hdr->num_busy_wgs);
    if (list_pos >= hdr->num_busy_wgs) return;  // idle workgroups sit at the end of wg_order
    const WaveGeom g = wave_geom(W, H, bx, bins, wg_order, list_pos);
    if (g.r1 <= g.r0) return;
    const int lane = g.lane;
    const float pxf = (float)g.px, pyf = (float)g.py;
    const size_t npix = (size_t)W * H, q = (size_t)g.py * W + g.px;
    float4 *wA = sA[g.wid], *wB = sB[g.wid], *wAcc = sAcc[g.wid];
    float *wC = sC[g.wid], *wD = sD[g.wid], *wAccF = reinterpret_cast<float *>(sAcc[g.wid]);
    const int slot = acc_slot(lane);

    const float T_final = g.inside ? final_T[q] : 0.f;
    const uint32_t last = g.inside ? n_contrib[q] : 0u;
    float d0 = 0.f, d1 = 0.f, d2 = 0.f;
    if (g.inside) {
        d0 = dL_dpix[q];
        d1 = dL_dpix[npix + q];
        d2 = dL_dpix[2 * npix + q];
    }
    float dd = 0.f, da = 0.f;  // dL/ddepth, dL/dalpha of this pixel
    if (EXTRA && g.inside) {
        if (dL_ddepth) dd = dL_ddepth[q];
        if (dL_dalpha) da = dL_dalpha[q];
    }
    float g2 = 0.f, UA = 0.f, UD = 0.f, z0 = 0.f;  // DISTORT: 2 dL/ddistortion of this pixel, U_A, U_D, the reference depth
    if constexpr (DISTORT) {
        if (g.inside) {
            g2 = 2.f * dL_ddistort[q];
            UA = totals[q];
            UD = totals[npix + q];
        }
        z0 = load_record(splats, point_list[g.r0]).C.y;  // (g.r0 < g.r1 here)
    }
    const float bg_dot = bg[0] * d0 + bg[1] * d1 + bg[2] * d2;
    const float ddelx_dx = 0.5f * (float)W, ddely_dy = 0.5f * (float)H;

    // deepest contributor over the bin: nothing behind it receives gradient
    uint32_t m = last;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d, 64));
    const int64_t max_last = (int64_t)__builtin_amdgcn_readfirstlane((int)m);
    if (max_last == 0) return;

    float T = T_final, A = 0.f;  // A = (colour accumulated behind the current splat) . dL/dpixel
    const float nTb = -T_final * bg_dot;

    // positions are 0-based from the front of the bin list; walk from max_last-1 down to 0 in rounds of 64
    float4 nA = make_float4(0.f, 0.f, 0.f, 0.f), nB = nA;
    float nC = 0.f, nD = 0.f;
    uint32_t nRec = 0;  // this lane's staged instance's slot (Gaussian, cell of its bin rect) = index of its gradient record
    const int bin_x = g.bin % bx, bin_y = g.bin / bx;
    auto stage = [&](uint32_t list_pos) {
        const uint32_t id = point_list[list_pos];
        const SplatRec r = load_record(splats, id);
        nA = r.A; nB = r.B; nC = r.C.x;
        if (EXTRA) nD = r.C.y;
        nRec = inst_slot(goff, gpart, id, r.C, bin_x, bin_y);
    };
    if ((int64_t)lane <= max_last - 1) stage(g.r0 + (uint32_t)(max_last - 1 - lane));
    for (int64_t top = max_last - 1; top >= 0; top -= WAVE) {
        const int cnt = (int)min((int64_t)WAVE, top + 1);
        wave_sync_lds();
        stage_record<EXTRA>(wA, wB, wC, wD, lane, nA, nB, nC, nD);
        const uint32_t curRec = nRec;
        wave_sync_lds();
        const int64_t ntop = top - WAVE;
        if (ntop - lane >= 0) stage(g.r0 + (uint32_t)(ntop - lane));  // prefetch the next round
        lanemask_t touched = 0ull;  // which staged splats received any gradient (wave-uniform)
        for (int j = 0; j < cnt; j++) {
            const uint32_t pos = (uint32_t)(top - j);
            const float4 a = wA[j];
            const float4 b = wB[j];
            const BwdPair p = bwd_pair(a, b, pxf, pyf, pos, last);
            if (p.valid_m == 0ull) continue;  // wave-uniform
            const bool valid = __builtin_amdgcn_inverse_ballot_w64(p.valid_m);
            touched |= 1ull << j;
            const BwdStep s = bwd_step(valid, p.G, p.alpha, T);
            T = s.T;
            float cd = bwd_colour_dot<EXTRA>(b, wC, wD, j, d0, d1, d2, dd, da);
            const float w = s.ae * T;  // dchannel/dcolour
            float dzv = 0.f;         // DISTORT: this pixel's g d dist / d z_i
            if constexpr (DISTORT) {
                const float zs = wD[j] - z0;
                cd = cd + __builtin_fmaf(zs, UA, -UD) * g2;
                dzv = (g2 * w) * (UA - w);
                UA = __builtin_fmaf(-2.f, w, UA);
                UD = __builtin_fmaf(-2.f * w, zs, UD);
            }
            const BwdAlpha r = bwd_alpha(cd, A, T, nTb, s.rcp, s.ae, s.om);
            A = r.A;
            const float g_r = w * d0, g_g = w * d1, g_b = w * d2;  // in front of the moments: the statement order decides the schedule
            const BwdMom mom = bwd_moments(b.y, r.dL_dalpha, s.Ge, p.dx, p.dy);
            const float red[9] = {g_r, g_g, g_b, mom.m_x, mom.m_y, mom.m_xx, mom.m_xy, mom.m_yy, mom.m_0};
            float ra = 0.f;
            if constexpr (ABSGRAD) {
                // s (A dx + B dy) and s (C dy + B dx) up to the factor -2 / log2 e of the pre-scaled conic (applied at flush time); a lane the splat
                // does not reach has m_0 = 0 and adds exact zeros.  (Formed in front of the reduce-scatter so that the two DPP chains interleave.)
                const float hb = 0.5f * a.w;
                const float tx = a.z * mom.m_x + hb * mom.m_y;
                const float ty = b.x * mom.m_y + hb * mom.m_x;
                ra = wave_row_sum(swap_absadd32(tx, ty));  // rows 0, 1: |t_x| of the row pairs (0, 2), (1, 3); rows 2, 3: |t_y|
            }
            const float out = wave_reduce_scatter9(red, (lane & 8) != 0);
            if (slot >= 0) wAccF[4 * REC * j + slot] = out;  // 12 lanes, 12 distinct words of this splat's record
            if (EXTRA) {
                float rz = wave_row_sum(w * dd);  // dL/dz share of this pixel: w dL/ddepth
                // DISTORT: the map's share in a row sum of its own, so that w dL/ddepth's keeps the operations -- and with g = 0 the bits -- it has without it
                if constexpr (DISTORT) rz += wave_row_sum(dzv);
                if ((lane & 15) == 7) wAccF[4 * REC * j + 12 + (lane >> 4)] = rz;
            }
            if constexpr (ABSGRAD) {
                if ((lane & 15) == 7) wAccF[4 * REC * j + 4 * AB + (lane >> 4)] = ra;
            }
        }
        wave_sync_lds();
        if ((touched >> lane) & 1ull) {  // lane j flushes staged splat j
            flush_record<EXTRA>(wAcc, REC, wA, wB, lane, ddelx_dx, ddely_dy, curRec, inst_grad, inst_dop, inst_ddepth);
            if constexpr (ABSGRAD) {  // in the units of g_mx / g_my (NDC-scaled); a fixed order, never negative
                const float4 ab = wAcc[REC * lane + AB];
                inst_absgrad[curRec] = make_float2(ddelx_dx * (GSR_KA * (ab.x + ab.y)), ddely_dy * (GSR_KA * (ab.z + ab.w)));
            }
            inst_valid[curRec] = 1;
        }
    }
}

// ---- F-channel feature maps (GsrFeatures): feat[c, p] = sum_i f[i, c] alpha_i T_i, background 0 -------------------------------------------------
// The same blend as k_composite_fwd, with F more channels whose values come from the caller's [rows, F] array instead of the splat record.  The
// channels are split into chunks of NF over gridDim.y (NF accumulators per lane keep the kernel near the plain one's register budget); every
// chunk's wave walks the same bin with the same arithmetic, so w = alpha T has the same bits in every chunk and in a plain run, and chunk 0 alone
// writes the image, final_T, n_contrib (and the depth / alpha maps) and clears the record flags.  Each lane stages its splat's NF features
// (dword loads: a row is 4-byte aligned only) into LDS beside sA / sB / sC; the blend loop reads them as broadcasts, acc += f w being the
// same v_fma_f32 as a colour channel's.
constexpr int GSR_FEAT_PAD = 4;  // LDS row stride NF + 4 floats: a lane's 16-byte stores of its row spread over the banks
template <bool EXTRA, int NF>
__global__ __launch_bounds__(64 * WAVES) void k_composite_fwd_feat(int W, int H, int bx, const GsrSplat *__restrict__ splats,
                                                            GsrBins bins, const uint32_t *__restrict__ wg_order,
                                                            const uint32_t *__restrict__ point_list, const float *__restrict__ bg,
                                                            float *__restrict__ out_color, float *__restrict__ final_T,
                                                            uint32_t *__restrict__ n_contrib, const GsrHeader *__restrict__ hdr, uint8_t *__restrict__ inst_valid,
                                                            float *__restrict__ out_depth, float *__restrict__ out_alpha,
                                                            const float *__restrict__ features, int F, const uint32_t *__restrict__ row_range,
                                                            float *__restrict__ out_feat) {
    constexpr int FS = NF + GSR_FEAT_PAD;
    __shared__ float4 sA[WAVES][WAVE];
    __shared__ float4 sB[WAVES][WAVE];
    __shared__ float sC[WAVES][WAVE];
    __shared__ float sD[WAVES][EXTRA ? WAVE : 1];
    __shared__ __attribute__((aligned(16))) float sF[WAVES][WAVE * FS];
    const uint32_t list_pos = xcd_list_pos(blockIdx.x, hdr->num_busy_wgs);
    const WaveGeom g = wave_geom(W, H, bx, bins, wg_order, list_pos);
    const bool chunk0 = blockIdx.y == 0;
    const int c0 = (int)blockIdx.y * NF, nc = min(NF, F - c0);  // this chunk's channels [c0, c0 + nc)
    const size_t npix = (size_t)W * H;
    if (hdr->overflow) {
        if (chunk0) {
            fwd_write_blank<EXTRA>(g, W, H, out_color, final_T, n_contrib, out_depth, out_alpha);
        }
        if (g.inside) {
            const size_t q = (size_t)g.py * W + g.px;
            for (int k = 0; k < nc; k++) out_feat[(size_t)(c0 + k) * npix + q] = 0.f;
        }
        return;
    }
    if (chunk0) clear_record_flags(inst_valid, hdr, (int)threadIdx.x, 64 * WAVES);
    const uint32_t row0 = row_range ? row_range[0] : 0u;  // splat id i is row row0 + i of the caller's arrays (gsr_view_rows)
    const float *__restrict__ fbase = features + c0;
    const float pxf = (float)g.px, pyf = (float)g.py;
    float4 *wA = sA[g.wid], *wB = sB[g.wid];
    float *wC = sC[g.wid], *wD = sD[g.wid], *wF = sF[g.wid];

    float T = 1.f, C0 = 0.f, C1 = 0.f, C2 = 0.f, CD = 0.f, CA = 0.f;
    float acc[NF];
#pragma unroll
    for (int k = 0; k < NF; k++) acc[k] = 0.f;
    uint32_t last = 0, last_rnd = 0;
    lanemask_t active = __ballot(g.inside);
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)g.r0), r1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)g.r1);

    float4 nA = make_float4(0.f, 0.f, 0.f, 0.f), nB = nA;
    float nC = 0.f, nD = 0.f;
    float nF[NF];
    auto fetch = [&](uint32_t k) {  // list entry k: its 48-byte record and its NF features (0 past the last channel)
        const uint32_t id = point_list[k];
        const SplatRec r = load_record(splats, id);
        nA = r.A; nB = r.B; nC = r.C.x;
        if (EXTRA) nD = r.C.y;
        const float *f = fbase + (size_t)(row0 + id) * (size_t)F;
#pragma unroll
        for (int c = 0; c < NF; c++) nF[c] = c < nc ? f[c] : 0.f;
    };
#pragma unroll
    for (int c = 0; c < NF; c++) nF[c] = 0.f;
    if (r0 + g.lane < r1) fetch(r0 + g.lane);
    for (uint32_t base = r0; base < r1; base += WAVE) {
        if (active == 0ull) break;
        wave_sync_lds();
        stage_record<EXTRA>(wA, wB, wC, wD, g.lane, nA, nB, nC, nD);
#pragma unroll
        for (int c = 0; c < NF; c += 4) *reinterpret_cast<float4 *>(wF + g.lane * FS + c) = make_float4(nF[c], nF[c + 1], nF[c + 2], nF[c + 3]);
        wave_sync_lds();
        const uint32_t nk = base + WAVE + g.lane;
        nB.y = 0.f;
        if (nk < r1) fetch(nk);
        const int cnt = (int)min((uint32_t)WAVE, r1 - base);
#pragma unroll
        for (int j0 = 0; j0 < WAVE; j0 += 8) {
            if (j0 < cnt && active != 0ull) {
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int j = j0 + u;
                    const float4 a = wA[j];
                    const float4 b = wB[j];
                    const float c2 = wC[j];
                    const FwdPair p = fwd_pair(a, b, pxf, pyf, T, active);
                    active = p.active;
                    const float w = p.w;
                    C0 += b.z * w;
                    C1 += b.w * w;
                    C2 += c2 * w;
                    if (EXTRA) {
                        CD += wD[j] * w;
                        CA += w;
                    }
#pragma unroll
                    for (int c = 0; c < NF; c += 4) {
                        const float4 f = *reinterpret_cast<const float4 *>(wF + j * FS + c);
                        acc[c] += f.x * w;  // fma(f, w, acc): a colour channel's contraction
                        acc[c + 1] += f.y * w;
                        acc[c + 2] += f.z * w;
                        acc[c + 3] += f.w * w;
                    }
                    T = p.use ? p.test_T : T;
                    last_rnd = p.use ? (uint32_t)(j + 1) : last_rnd;
                }
            }
        }
        last = last_rnd ? (base - r0) + last_rnd : last;
        last_rnd = 0;
    }
    if (g.inside) {
        const size_t q = (size_t)g.py * W + g.px;
        if (chunk0) {
            final_T[q] = T;
            n_contrib[q] = last;
            const float bgs = hdr->num_points != 0u ? 1.f : 0.f;
            out_color[q] = C0 + T * (bgs * bg[0]);
            out_color[npix + q] = C1 + T * (bgs * bg[1]);
            out_color[2 * npix + q] = C2 + T * (bgs * bg[2]);
            if (EXTRA) {
                if (out_depth) out_depth[q] = CD;
                if (out_alpha) out_alpha[q] = CA;
            }
        }
#pragma unroll
        for (int c = 0; c < NF; c++)
            if (c < nc) out_feat[(size_t)(c0 + c) * npix + q] = acc[c];
    }
}

// Feature maps, backward (a): the geometry.  k_composite_bwd with the features' share of cd: cd += sum_c f[i, c] dL/dfeat[c, p] over ALL F
// channels (NG >= F of them held per lane in registers, the staged splats' rows in LDS), folded in before dL/dalpha -- exactly as F more colour
// channels with background 0 would enter the scalar recurrence.  The record, its nine-term reduce-scatter and inst_ddepth stay as they are.
// The staged splats' feature rows are loaded at the top of each round (the register prefetch would cost NG more VGPRs).
template <bool EXTRA, int NG>
__global__ __launch_bounds__(64 * WAVES) void k_composite_bwd_feat(int W, int H, int bx, const GsrSplat *__restrict__ splats,
                                                            GsrBins bins, const uint32_t *__restrict__ wg_order,
                                                            const uint32_t *__restrict__ point_list, const float *__restrict__ bg,
                                                            const float *__restrict__ dL_dpix, const float *__restrict__ final_T,
                                                            const uint32_t *__restrict__ n_contrib, const uint32_t *__restrict__ goff,
                                                            const uint32_t *__restrict__ gpart, uint8_t *__restrict__ inst_valid, float *__restrict__ inst_dop,
                                                            GsrGradAcc *__restrict__ inst_grad, const GsrHeader *__restrict__ hdr,
                                                            const float *__restrict__ dL_ddepth, const float *__restrict__ dL_dalpha, float *__restrict__ inst_ddepth,
                                                            const float *__restrict__ features, int F, const uint32_t *__restrict__ row_range,
                                                            const float *__restrict__ dL_dfeat) {
    constexpr int REC = EXTRA ? 4 : 3;
    constexpr int FS = NG + GSR_FEAT_PAD;
    __shared__ float4 sA[WAVES][WAVE];
    __shared__ float4 sB[WAVES][WAVE];
    __shared__ float sC[WAVES][WAVE];
    __shared__ float sD[WAVES][EXTRA ? WAVE : 1];
    __shared__ float4 sAcc[WAVES][WAVE * REC];
    __shared__ __attribute__((aligned(16))) float sF[WAVES][WAVE * FS];
    if (hdr->overflow) return;
    const uint32_t list_pos = xcd_list_pos(blockIdx.x, hdr->num_busy_wgs);
    if (list_pos >= hdr->num_busy_wgs) return;
    const WaveGeom g = wave_geom(W, H, bx, bins, wg_order, list_pos);
    if (g.r1 <= g.r0) return;
    const int lane = g.lane;
    const float pxf = (float)g.px, pyf = (float)g.py;
    const size_t npix = (size_t)W * H, q = (size_t)g.py * W + g.px;
    float4 *wA = sA[g.wid], *wB = sB[g.wid], *wAcc = sAcc[g.wid];
    float *wC = sC[g.wid], *wD = sD[g.wid], *wAccF = reinterpret_cast<float *>(sAcc[g.wid]), *wF = sF[g.wid];
    const int slot = acc_slot(lane);
    const uint32_t row0 = row_range ? row_range[0] : 0u;

    const float T_final = g.inside ? final_T[q] : 0.f;
    const uint32_t last = g.inside ? n_contrib[q] : 0u;
    float d0 = 0.f, d1 = 0.f, d2 = 0.f;
    if (g.inside) {
        d0 = dL_dpix[q];
        d1 = dL_dpix[npix + q];
        d2 = dL_dpix[2 * npix + q];
    }
    float dd = 0.f, da = 0.f;
    if (EXTRA && g.inside) {
        if (dL_ddepth) dd = dL_ddepth[q];
        if (dL_dalpha) da = dL_dalpha[q];
    }
    float gf[NG];  // dL/dfeat[c] of this pixel (0 past the last channel and outside the image)
#pragma unroll
    for (int c = 0; c < NG; c++) gf[c] = (c < F && g.inside) ? dL_dfeat[(size_t)c * npix + q] : 0.f;
    const float bg_dot = bg[0] * d0 + bg[1] * d1 + bg[2] * d2;
    const float ddelx_dx = 0.5f * (float)W, ddely_dy = 0.5f * (float)H;

    uint32_t m = last;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d, 64));
    const int64_t max_last = (int64_t)__builtin_amdgcn_readfirstlane((int)m);
    if (max_last == 0) return;

    float T = T_final, A = 0.f;
    const float nTb = -T_final * bg_dot;

    float4 nA = make_float4(0.f, 0.f, 0.f, 0.f), nB = nA;
    float nC = 0.f, nD = 0.f;
    uint32_t nRec = 0, nId = 0;
    bool nHas = false;
    const int bin_x = g.bin % bx, bin_y = g.bin / bx;
    auto stage = [&](uint32_t list_pos) {
        const uint32_t id = point_list[list_pos];
        const SplatRec r = load_record(splats, id);
        nA = r.A; nB = r.B; nC = r.C.x;
        if (EXTRA) nD = r.C.y;
        nRec = inst_slot(goff, gpart, id, r.C, bin_x, bin_y);
        nId = id;
        nHas = true;
    };
    if ((int64_t)lane <= max_last - 1) stage(g.r0 + (uint32_t)(max_last - 1 - lane));
    for (int64_t top = max_last - 1; top >= 0; top -= WAVE) {
        const int cnt = (int)min((int64_t)WAVE, top + 1);
        wave_sync_lds();
        stage_record<EXTRA>(wA, wB, wC, wD, lane, nA, nB, nC, nD);
        {  // this round's feature rows (a slot without a splat: zeros)
            const float *f = features + (size_t)(row0 + nId) * (size_t)F;
#pragma unroll
            for (int c = 0; c < NG; c += 4) {
                float4 v;
                v.x = (nHas && c < F) ? f[c] : 0.f;
                v.y = (nHas && c + 1 < F) ? f[c + 1] : 0.f;
                v.z = (nHas && c + 2 < F) ? f[c + 2] : 0.f;
                v.w = (nHas && c + 3 < F) ? f[c + 3] : 0.f;
                *reinterpret_cast<float4 *>(wF + lane * FS + c) = v;
            }
        }
        const uint32_t curRec = nRec;
        nHas = false;
        wave_sync_lds();
        const int64_t ntop = top - WAVE;
        if (ntop - lane >= 0) stage(g.r0 + (uint32_t)(ntop - lane));
        lanemask_t touched = 0ull;
        for (int j = 0; j < cnt; j++) {
            const uint32_t pos = (uint32_t)(top - j);
            const float4 a = wA[j];
            const float4 b = wB[j];
            const BwdPair p = bwd_pair(a, b, pxf, pyf, pos, last);
            if (p.valid_m == 0ull) continue;
            const bool valid = __builtin_amdgcn_inverse_ballot_w64(p.valid_m);
            touched |= 1ull << j;
            const BwdStep s = bwd_step(valid, p.G, p.alpha, T);
            T = s.T;
            float cd = bwd_colour_dot<EXTRA>(b, wC, wD, j, d0, d1, d2, dd, da);
            float fd = 0.f;  // the features' share: sum_c f[c] dL/dfeat[c]
#pragma unroll
            for (int c = 0; c < NG; c += 4) {
                const float4 f = *reinterpret_cast<const float4 *>(wF + j * FS + c);
                fd += f.x * gf[c];
                fd += f.y * gf[c + 1];
                fd += f.z * gf[c + 2];
                fd += f.w * gf[c + 3];
            }
            cd = cd + fd;
            const float w = s.ae * T;
            const BwdAlpha r = bwd_alpha(cd, A, T, nTb, s.rcp, s.ae, s.om);
            A = r.A;
            const float g_r = w * d0, g_g = w * d1, g_b = w * d2;
            const BwdMom mom = bwd_moments(b.y, r.dL_dalpha, s.Ge, p.dx, p.dy);
            const float red[9] = {g_r, g_g, g_b, mom.m_x, mom.m_y, mom.m_xx, mom.m_xy, mom.m_yy, mom.m_0};
            const float out = wave_reduce_scatter9(red, (lane & 8) != 0);
            if (slot >= 0) wAccF[4 * REC * j + slot] = out;
            if (EXTRA) {
                const float rz = wave_row_sum(w * dd);
                if ((lane & 15) == 7) wAccF[4 * REC * j + 12 + (lane >> 4)] = rz;
            }
        }
        wave_sync_lds();
        if ((touched >> lane) & 1ull) {
            flush_record<EXTRA>(wAcc, REC, wA, wB, lane, ddelx_dx, ddely_dy, curRec, inst_grad, inst_dop, inst_ddepth);
            inst_valid[curRec] = 1;
        }
    }
}

// Feature maps, backward (b): dL/df[i, c] = sum_p w dL/dfeat[c, p] per (bin, splat) instance.  w = alpha T needs only the T recurrence, which
// does not depend on colour, so this walk is chunked over gridDim.y like the forward and repeats the geometry walk's decisions (same arithmetic:
// its `touched` set is the set of instances whose inst_valid flag k_composite_bwd(_feat) sets).  Per round every lane parks its 64 weights in LDS
// (w[p][j], row stride 65: conflict-free both ways); then lane j forms its staged splat's NF sums over the 64 pixels in pixel order from the
// broadcast gradients of the chunk -- a fixed order, no atomics -- and writes them to inst_dfeat[slot * F + c].
template <int NF>
__global__ __launch_bounds__(64 * WAVES) void k_composite_bwd_featgrad(int W, int H, int bx, const GsrSplat *__restrict__ splats,
                                                                GsrBins bins, const uint32_t *__restrict__ wg_order,
                                                                const uint32_t *__restrict__ point_list, const float *__restrict__ final_T,
                                                                const uint32_t *__restrict__ n_contrib, const uint32_t *__restrict__ goff,
                                                                const uint32_t *__restrict__ gpart, const GsrHeader *__restrict__ hdr,
                                                                int F, const float *__restrict__ dL_dfeat, float *__restrict__ inst_dfeat) {
    constexpr int WS = WAVE + 1;
    __shared__ float4 sA[WAVES][WAVE];
    __shared__ float4 sB[WAVES][WAVE];
    __shared__ __attribute__((aligned(16))) float sG[WAVES][WAVE * NF];
    __shared__ float sW[WAVES][WAVE * WS];
    if (hdr->overflow) return;
    const uint32_t list_pos = xcd_list_pos(blockIdx.x, hdr->num_busy_wgs);
    if (list_pos >= hdr->num_busy_wgs) return;
    const WaveGeom g = wave_geom(W, H, bx, bins, wg_order, list_pos);
    if (g.r1 <= g.r0) return;
    const int lane = g.lane;
    const int c0 = (int)blockIdx.y * NF, nc = min(NF, F - c0);
    const float pxf = (float)g.px, pyf = (float)g.py;
    const size_t npix = (size_t)W * H, q = (size_t)g.py * W + g.px;
    float4 *wA = sA[g.wid], *wB = sB[g.wid];
    float *wG = sG[g.wid], *wW = sW[g.wid];

    const float T_final = g.inside ? final_T[q] : 0.f;
    const uint32_t last = g.inside ? n_contrib[q] : 0u;
#pragma unroll
    for (int c = 0; c < NF; c++) wG[lane * NF + c] = (c < nc && g.inside) ? dL_dfeat[(size_t)(c0 + c) * npix + q] : 0.f;

    uint32_t m = last;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d, 64));
    const int64_t max_last = (int64_t)__builtin_amdgcn_readfirstlane((int)m);
    if (max_last == 0) return;

    float T = T_final;
    float4 nA = make_float4(0.f, 0.f, 0.f, 0.f), nB = nA;
    uint32_t nRec = 0;
    const int bin_x = g.bin % bx, bin_y = g.bin / bx;
    auto stage = [&](uint32_t list_pos) {
        const uint32_t id = point_list[list_pos];
        const SplatRec r = load_record(splats, id);
        nA = r.A; nB = r.B;
        nRec = inst_slot(goff, gpart, id, r.C, bin_x, bin_y);
    };
    if ((int64_t)lane <= max_last - 1) stage(g.r0 + (uint32_t)(max_last - 1 - lane));
    for (int64_t top = max_last - 1; top >= 0; top -= WAVE) {
        const int cnt = (int)min((int64_t)WAVE, top + 1);
        wave_sync_lds();
        stage_record(wA, wB, lane, nA, nB);
        const uint32_t curRec = nRec;
        wave_sync_lds();
        const int64_t ntop = top - WAVE;
        if (ntop - lane >= 0) stage(g.r0 + (uint32_t)(ntop - lane));
        lanemask_t touched = 0ull;
        for (int j = 0; j < cnt; j++) {
            const uint32_t pos = (uint32_t)(top - j);
            const float4 a = wA[j];
            const float4 b = wB[j];
            const BwdPair p = bwd_pair(a, b, pxf, pyf, pos, last);
            if (p.valid_m == 0ull) continue;  // (its weights are never read: lane j only sums when touched)
            const bool valid = __builtin_amdgcn_inverse_ballot_w64(p.valid_m);
            touched |= 1ull << j;
            const BwdStep s = bwd_step(valid, p.G, p.alpha, T);
            T = s.T;
            wW[lane * WS + j] = s.ae * T;
        }
        wave_sync_lds();
        if ((touched >> lane) & 1ull) {
            float acc[NF];
#pragma unroll
            for (int c = 0; c < NF; c++) acc[c] = 0.f;
#pragma unroll 2
            for (int p = 0; p < WAVE; p++) {
                const float w = wW[p * WS + lane];
#pragma unroll
                for (int c = 0; c < NF; c += 4) {
                    const float4 gv = *reinterpret_cast<const float4 *>(wG + p * NF + c);
                    acc[c] += w * gv.x;
                    acc[c + 1] += w * gv.y;
                    acc[c + 2] += w * gv.z;
                    acc[c + 3] += w * gv.w;
                }
            }
            float *dst = inst_dfeat + (size_t)curRec * (size_t)F + c0;
#pragma unroll
            for (int c = 0; c < NF; c++)
                if (c < nc) dst[c] = acc[c];
        }
    }
}

// Feature maps, backward (b), second half: each Gaussian's flagged slots streamed in slot order (k_preprocess_bwd's order and slot range) into
// dL_dfeatures[row, c]; one thread per (Gaussian, channel), so neighbouring threads read neighbouring floats of a slot.  Gaussians without records
// -- culled, overflowed view, or inst_dfeat NULL (the feature map received no gradient) -- get exact zeros.  Rows outside the view are not written.
__global__ __launch_bounds__(256) void k_feature_grad_gather(int P, int F, const uint32_t *__restrict__ row_range, const int *__restrict__ radii,
                                                             const uint32_t *__restrict__ goff, const uint32_t *__restrict__ gpart,
                                                             const uint8_t *__restrict__ inst_valid, const float *__restrict__ inst_dfeat,
                                                             const GsrHeader *__restrict__ hdr, float *__restrict__ dL_dfeatures) {
    uint32_t row0;
    int nP;
    gsr_view_rows(row_range, P, row0, nP);
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)nP * F) return;
    const int i = (int)(idx / F), c = (int)(idx - (int64_t)i * F);
    const size_t r = (size_t)row0 + (size_t)i;
    float sum = 0.f;
    if (inst_dfeat && hdr->overflow == 0u && radii[r] > 0) {
        const int gb = i >> GSR_BIN_SHIFT;
        const uint32_t gbase = gpart[gb];
        const uint32_t s0 = gbase + goff[i];
        const uint32_t s1 = ((i & (GSR_BIN_THREADS - 1)) != GSR_BIN_THREADS - 1 && i + 1 < P) ? gbase + goff[i + 1] : ((gb + 1) * GSR_BIN_THREADS < P ? gpart[gb + 1] : hdr->num_slots);
        for (uint32_t k = s0; k < s1; k++)
            if (inst_valid[k]) sum += inst_dfeat[(size_t)k * F + c];
    }
    dL_dfeatures[r * F + c] = sum;
}

// Contribution statistics: the tail's slots [0, num_slots) are zeroed in front of the CONTRIB forward -- a slot no staged splat writes (not walked
// before its bin saturated, blended into no pixel, or a bin-rect cell outside the Gaussian's lists) must read as empty.  It cannot be the forward's
// own job like clear_record_flags: there another workgroup's record could land before the clearing one.  An overflowed view is left alone (its slot
// count may exceed the capacity the tail was sized for; the gather writes zeros for it).
__global__ __launch_bounds__(256) void k_contrib_clear(float4 *__restrict__ inst_contrib, const GsrHeader *__restrict__ hdr) {
    if (hdr->overflow) return;
    const uint32_t n = hdr->num_slots;
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < n; k += gridDim.x * 256u) inst_contrib[k] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// Contribution statistics, second half: each Gaussian's slots streamed in slot order (k_preprocess_bwd's slot range) into weight_sum / weight_max /
// pixel_count[row]; one thread per Gaussian.  A fixed summation order and no atomics: the same bits on every run.  Culled Gaussians and every
// Gaussian of an overflowed view get exact zeros; rows outside the view are not written; a NULL output is skipped.
__global__ __launch_bounds__(256) void k_contrib_gather(int P, const uint32_t *__restrict__ row_range, const int *__restrict__ radii,
                                                        const uint32_t *__restrict__ goff, const uint32_t *__restrict__ gpart,
                                                        const float4 *__restrict__ inst_contrib, const GsrHeader *__restrict__ hdr,
                                                        float *__restrict__ weight_sum, float *__restrict__ weight_max, int32_t *__restrict__ pixel_count) {
    uint32_t row0;
    int nP;
    gsr_view_rows(row_range, P, row0, nP);
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= nP) return;
    const size_t r = (size_t)row0 + (size_t)i;
    float sum = 0.f, mx = 0.f;
    uint32_t n = 0u;
    if (hdr->overflow == 0u && radii[r] > 0) {
        const int gb = i >> GSR_BIN_SHIFT;
        const uint32_t gbase = gpart[gb];
        const uint32_t s0 = gbase + goff[i];
        const uint32_t s1 = ((i & (GSR_BIN_THREADS - 1)) != GSR_BIN_THREADS - 1 && i + 1 < P) ? gbase + goff[i + 1] : ((gb + 1) * GSR_BIN_THREADS < P ? gpart[gb + 1] : hdr->num_slots);
        for (uint32_t k = s0; k < s1; k++) {
            const float4 v = inst_contrib[k];
            sum += v.x;
            mx = fmaxf(mx, v.y);
            n += __float_as_uint(v.z);
        }
    }
    if (weight_sum) weight_sum[r] = sum;
    if (weight_max) weight_max[r] = mx;
    if (pixel_count) pixel_count[r] = (int32_t)n;
}

// Absolute screen-space gradient, second half: each Gaussian's FLAGGED slots (the records the backward compositing launch just wrote) streamed in slot
// order (k_preprocess_bwd's slot range) into absgrad[row]; one thread per Gaussian, a fixed summation order, no atomics.  Culled Gaussians, Gaussians
// without a record and every Gaussian of an overflowed view (whose backward wrote nothing: the flags are not looked at) get exact zeros; rows outside
// the view are not written.
__global__ __launch_bounds__(256) void k_absgrad_gather(int P, const uint32_t *__restrict__ row_range, const int *__restrict__ radii,
                                                        const uint32_t *__restrict__ goff, const uint32_t *__restrict__ gpart,
                                                        const uint8_t *__restrict__ inst_valid, const float2 *__restrict__ inst_absgrad,
                                                        const GsrHeader *__restrict__ hdr, float2 *__restrict__ absgrad) {
    uint32_t row0;
    int nP;
    gsr_view_rows(row_range, P, row0, nP);
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= nP) return;
    const size_t r = (size_t)row0 + (size_t)i;
    float ax = 0.f, ay = 0.f;
    if (hdr->overflow == 0u && radii[r] > 0) {
        const int gb = i >> GSR_BIN_SHIFT;
        const uint32_t gbase = gpart[gb];
        const uint32_t s0 = gbase + goff[i];
        const uint32_t s1 = ((i & (GSR_BIN_THREADS - 1)) != GSR_BIN_THREADS - 1 && i + 1 < P) ? gbase + goff[i + 1] : ((gb + 1) * GSR_BIN_THREADS < P ? gpart[gb + 1] : hdr->num_slots);
        for (uint32_t k = s0; k < s1; k++)
            if (inst_valid[k]) {
                const float2 v = inst_absgrad[k];
                ax += v.x;
                ay += v.y;
            }
    }
    absgrad[r] = make_float2(ax, ay);
}

}  // namespace

// feature chunk width of the forward and the per-slot sums: the smallest of 4 / 8 / 16 that holds F, 16-channel chunks beyond
static int feat_chunk(int F) { return F <= 4 ? 4 : F <= 8 ? 8 : 16; }

// The launch records unpacked into the kernels' parameter lists; LAUNCH(true / false, ...) by the run-time `extra`.  One helper per option, in the order the
// options were added: the kernels stand in the code object in the order of their first use, and that order is kept.
#define GSR_FWD_ARGS c.W, c.H, c.bx, c.splats, c.bins, c.wg_order, c.point_list, c.bg, c.out_color, c.final_T, c.n_contrib, c.hdr, c.inst_valid, c.out_depth, c.out_alpha
#define GSR_BWD_ARGS c.W, c.H, c.bx, c.splats, c.bins, c.wg_order, c.point_list, c.bg, c.dL_dpix, c.final_T, c.n_contrib, c.goff, c.gpart, c.inst_valid, c.inst_dop, \
                     c.inst_grad, c.hdr, extra ? c.dL_ddepth : nullptr, extra ? c.dL_dalpha : nullptr, c.inst_ddepth
#define GSR_FWD(E, C) hipLaunchKernelGGL((k_composite_fwd<E, C>), grid, block, gsr_debug_lds_pad(), c.s, GSR_FWD_ARGS, c.goff, c.gpart, c.inst_contrib, nullptr, nullptr)
#define GSR_BWD(E, A) hipLaunchKernelGGL((k_composite_bwd<E, A>), grid, block, gsr_debug_lds_pad(), c.s, GSR_BWD_ARGS, c.inst_absgrad, nullptr, nullptr)
#define GSR_FWD_FEAT(E, N) hipLaunchKernelGGL((k_composite_fwd_feat<E, N>), grid, block, gsr_debug_lds_pad(), c.s, GSR_FWD_ARGS, c.features, c.F, c.row_range, c.out_feat)
#define GSR_BWD_FEAT(E, N) hipLaunchKernelGGL((k_composite_bwd_feat<E, N>), grid, block, gsr_debug_lds_pad(), c.s, GSR_BWD_ARGS, c.features, c.F, c.row_range, c.dL_dfeat)
#define GSR_FEATGRAD(N) hipLaunchKernelGGL((k_composite_bwd_featgrad<N>), dim3(grid.x, (c.F + N - 1) / N), block, gsr_debug_lds_pad(), c.s, c.W, c.H, c.bx, c.splats, c.bins, \
                                           c.wg_order, c.point_list, c.final_T, c.n_contrib, c.goff, c.gpart, c.hdr, c.F, c.dL_dfeat, c.inst_dfeat)
#define GSR_PICK_EXTRA(LAUNCH, OPT) do { if (extra) LAUNCH(true, OPT); else LAUNCH(false, OPT); } while (0)
static const dim3 block(64 * WAVES);

static void fwd_plain(const GsrCompositeFwd &c, dim3 grid, bool extra) { GSR_PICK_EXTRA(GSR_FWD, false); }
static void bwd_plain(const GsrCompositeBwd &c, dim3 grid, bool extra) { GSR_PICK_EXTRA(GSR_BWD, false); }
static void fwd_feat(const GsrCompositeFwd &c, dim3 grid, bool extra) {
    const int nf = feat_chunk(c.F);
    grid.y = (c.F + nf - 1) / nf;
    if (extra) {
        if (nf == 4) GSR_FWD_FEAT(true, 4); else if (nf == 8) GSR_FWD_FEAT(true, 8); else GSR_FWD_FEAT(true, 16);
    } else {
        if (nf == 4) GSR_FWD_FEAT(false, 4); else if (nf == 8) GSR_FWD_FEAT(false, 8); else GSR_FWD_FEAT(false, 16);
    }
}
static void bwd_feat(const GsrCompositeBwd &c, dim3 grid, bool extra) {
    if (extra) {
        if (c.F <= 4) GSR_BWD_FEAT(true, 4); else if (c.F <= 8) GSR_BWD_FEAT(true, 8); else if (c.F <= 16) GSR_BWD_FEAT(true, 16);
        else if (c.F <= 32) GSR_BWD_FEAT(true, 32); else GSR_BWD_FEAT(true, 64);
    } else {
        if (c.F <= 4) GSR_BWD_FEAT(false, 4); else if (c.F <= 8) GSR_BWD_FEAT(false, 8); else if (c.F <= 16) GSR_BWD_FEAT(false, 16);
        else if (c.F <= 32) GSR_BWD_FEAT(false, 32); else GSR_BWD_FEAT(false, 64);
    }
    if (!c.inst_dfeat) return;
    const int nf = feat_chunk(c.F);
    if (nf == 4) GSR_FEATGRAD(4); else if (nf == 8) GSR_FEATGRAD(8); else GSR_FEATGRAD(16);
}
static void fwd_contrib(const GsrCompositeFwd &c, dim3 grid, bool extra) { GSR_PICK_EXTRA(GSR_FWD, true); }
static void bwd_absgrad(const GsrCompositeBwd &c, dim3 grid, bool extra) { GSR_PICK_EXTRA(GSR_BWD, true); }
// the distortion map: EXTRA whatever the depth / alpha pointers are (the maps a call did not ask for stay NULL and are not written)
static void fwd_distort(const GsrCompositeFwd &c, dim3 grid, bool) {
    hipLaunchKernelGGL((k_composite_fwd<true, false, true>), grid, block, gsr_debug_lds_pad(), c.s, GSR_FWD_ARGS, c.goff, c.gpart, c.inst_contrib, c.out_distort, c.totals);
}
static void bwd_distort(const GsrCompositeBwd &c, dim3 grid, bool) {
    const bool extra = true;
    hipLaunchKernelGGL((k_composite_bwd<true, false, true>), grid, block, gsr_debug_lds_pad(), c.s, GSR_BWD_ARGS, c.inst_absgrad, c.dL_ddistort, c.totals);
}

void gsr_launch_composite_fwd(const GsrCompositeFwd &c) {
    const int wgs = (c.bx / WAVES) * c.by;
    if (wgs > 0) (c.F > 0 ? fwd_feat : c.inst_contrib ? fwd_contrib : c.out_distort ? fwd_distort : fwd_plain)(c, dim3(wgs), c.out_depth || c.out_alpha);
}

void gsr_launch_composite_bwd(const GsrCompositeBwd &c) {
    const int wgs = (c.bx / WAVES) * c.by;
    if (wgs > 0) (c.dL_dfeat && c.F > 0 ? bwd_feat : c.inst_absgrad ? bwd_absgrad : c.dL_ddistort ? bwd_distort : bwd_plain)(c, dim3(wgs), c.inst_ddepth != nullptr);
}

void gsr_launch_feature_grad_gather(int P, int F, const uint32_t *row_range, const int *radii, const uint32_t *goff, const uint32_t *gpart,
                                    const uint8_t *inst_valid, const float *inst_dfeat, const GsrHeader *hdr, float *dL_dfeatures, hipStream_t s) {
    const int64_t n = (int64_t)P * F;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_feature_grad_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P, F, row_range, radii, goff, gpart, inst_valid, inst_dfeat, hdr,
                       dL_dfeatures);
}

void gsr_launch_contrib_clear(float4 *inst_contrib, int64_t cap, const GsrHeader *hdr, hipStream_t s) {
    const int64_t blocks = (cap + 255) / 256;
    hipLaunchKernelGGL(k_contrib_clear, dim3((unsigned)(blocks < 1 ? 1 : blocks > 2048 ? 2048 : blocks)), dim3(256), 0, s, inst_contrib, hdr);
}

void gsr_launch_contrib_gather(int P, const uint32_t *row_range, const int *radii, const uint32_t *goff, const uint32_t *gpart, const float4 *inst_contrib,
                               const GsrHeader *hdr, float *weight_sum, float *weight_max, int32_t *pixel_count, hipStream_t s) {
    if (P <= 0) return;
    hipLaunchKernelGGL(k_contrib_gather, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, P, row_range, radii, goff, gpart, inst_contrib, hdr, weight_sum,
                       weight_max, pixel_count);
}

void gsr_launch_absgrad_gather(int P, const uint32_t *row_range, const int *radii, const uint32_t *goff, const uint32_t *gpart, const uint8_t *inst_valid,
                               const float2 *inst_absgrad, const GsrHeader *hdr, float2 *absgrad, hipStream_t s) {
    if (P <= 0) return;
    hipLaunchKernelGGL(k_absgrad_gather, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, P, row_range, radii, goff, gpart, inst_valid, inst_absgrad, hdr,
                       absgrad);
}
