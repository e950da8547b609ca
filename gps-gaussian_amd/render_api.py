"""render(data, idx, ...) and pts2render(data, bg_color) with the reference's signatures and semantics.

Host-side mirror of /root/reference/gaussian_renderer/__init__.py:17-67 (`render`) and
/root/reference/lib/GaussianRender.py:6-40 (`pts2render`).  The reference's own two files also run unmodified against
the drop-in `diff_gaussian_rasterization` shim; these mirrors exist so that callers (bench, tests, the DDP launcher)
do not need /root/reference on the path, and they read the camera scalars without per-sample device syncs when the
tensors already live on the host.
"""
import math
import os

import torch

from . import rasterizer as _RZ
from .rasterizer import GaussianRasterizationSettings, GaussianRasterizer

import threading

_tls = threading.local()  # per host thread: device index -> side streams (the samples of a batch are independent views and render concurrently)


def _streams(dev, n):
    pools = getattr(_tls, "pools", None)
    if pools is None:
        pools = _tls.pools = {}
    pool = pools.setdefault(dev.index, [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device=dev))
    return pool[:n]


_bg_cache = {}


def _bg_tensor(bg_color, dev):
    """The background colour on the device.  torch.tensor(list, device=cuda) -- what the reference does per render() call,
    gaussian_renderer/__init__.py:23 -- is a SYNCHRONOUS copy from pageable memory: it blocks the host until the stream has drained
    (measured 0.35 ms per stage-2 iteration, and it stops the host from running ahead of the GPU).  The handful of distinct colours a
    run uses are kept on the device instead."""
    if isinstance(bg_color, torch.Tensor):
        return bg_color.to(device=dev, dtype=torch.float32)
    key = (tuple(float(c) for c in bg_color), dev.index)
    t = _bg_cache.get(key)
    if t is None:
        if len(_bg_cache) > 64:
            _bg_cache.clear()
        t = _bg_cache[key] = torch.tensor(key[0], dtype=torch.float32, device=dev)
    return t


def _scalar(x):
    return float(x.item()) if isinstance(x, torch.Tensor) else float(x)


class _SplitRows(torch.autograd.Function):
    """packed[rows, C] -> row chunks, like torch.split -- but if the chunk gradients come back as the matching consecutive row
    slices of ONE buffer (the rasteriser backward was handed such slices: grad_arena), that buffer IS the gradient of `packed`
    and nothing is copied.  Otherwise falls back to what SplitBackward does: one concatenation."""

    @staticmethod
    def forward(ctx, packed, sizes, arena):
        ctx.sizes = sizes
        ctx.arena = arena
        ctx.shape = tuple(packed.shape)
        ctx.set_materialize_grads(False)
        return tuple(c.view_as(c) for c in packed.detach().split(sizes))

    @staticmethod
    def backward(ctx, *grads):
        arena = ctx.arena
        if arena is not None:
            off, ok = 0, True
            for g, n in zip(grads[:-1], ctx.sizes[:-1]):  # the last chunk is the unused tail of the packed capacity
                if n and (g is None or g.data_ptr() != arena.data_ptr() + off * arena.stride(0) * 4 or g.shape[0] != n):
                    ok = False
                    break
                off += n
            if ok:
                return arena, None, None
        parts = [g if g is not None else torch.zeros((n,) + ctx.shape[1:], dtype=torch.float32, device=arena.device if arena is not None else None)
                 for g, n in zip(grads, ctx.sizes)]
        return torch.cat(parts, dim=0), None, None


class _Holder:
    """Attribute holder handed to rasterizer._forward_impl / _backward_impl in place of an autograd ctx (one per view of a batch)."""
    pass


def _row(t, i):
    return t[i] if t is not None else None


class _RenderBatch(torch.autograd.Function):
    """All samples of a pts2render batch as ONE autograd node: B raster forwards enqueued back to back on B HIP streams (the views
    are independent and one view leaves the chip under-occupied: DESIGN.md section 4), their exact capacity checks collected and run
    once all are in flight, the images written straight into one [B,3,H,W] tensor; the backward does the same with the B raster
    backwards, each writing its rows of six batch-wide gradient buffers.  Replaces, per iteration, 5 split nodes + B rasteriser
    nodes + one concatenation (and their Python), which is what kept the per-sample form host-bound (tools/stage2_ab.py).

    The HOST NEVER LEARNS how many valid pixels a sample has: every view is handed the packed batch-wide arrays plus a DEVICE pointer
    to its {begin, end} row range (GsrViewExt.row_range; the pack kernels' offsets tensor) and a row capacity; the kernels read the range
    themselves.  The reference learns those counts through ten boolean-mask gathers per sample, each a device sync
    (lib/GaussianRender.py:15-34); the round-2 form of this class still read the B + 1 offsets back (one sync per batch).
    Numerically it IS the per-sample path: the same kernels on the same rows (tests/test_gpu_pack.py compares the bits)."""

    @staticmethod
    def forward(ctx, xyz, rgb, rot, scale, opacity, offsets, settings, cap_rows, opts=_RZ._DEFAULT_OPTIONS, view_all=None, proj_all=None,
                campos_all=None, features=None):
        # xyz .. opacity: packed [N, C] fp32 (pack.pack_views); offsets: B + 1 row offsets, int32 ON THE DEVICE; settings: B
        # GaussianRasterizationSettings; cap_rows: upper bound of a sample's rows (views x pixels); opts (rasterizer._ViewOptions) -- depth_alpha:
        # also return the depth and alpha maps [B,1,H,W] (rasterizer.rasterize_gaussians(return_depth_alpha=True)); antialiasing: every view with
        # GSR_FLAG_ANTIALIAS; camera_grad: view_all / proj_all / campos_all ([B,4,4], [B,4,4], [B,3]: the batch's novel cameras as the caller holds
        # them) get the per-sample camera gradients (rasterizer.rasterize_gaussians(camera_grad=True)); features: packed [N, F]
        # (pack.pack_features), the feature maps [B,F,H,W] are returned last (rasterizer.rasterize_gaussians(features=...)); contrib: then the
        # per-Gaussian statistics weight_sum, weight_max (fp32) and pixel_count (int32), batch-wide [N] like the packed inputs (each view writes its
        # rows); absgrad: last of all the absolute screen-space gradient [N, 2], zeros here, each view's rows overwritten by every backward
        # (rasterizer.rasterize_gaussians(return_absgrad=True)); opts.absgrad_sink is then called with it at the end of the backward, on its stream;
        # distortion: last, the depth-distortion maps [B,1,H,W] (rasterizer.rasterize_gaussians(return_distortion=True)), differentiable
        # -> rasterizer._pack_outputs of the batch-wide rasterizer._Outputs (no radii)
        bs = len(settings)
        dev = xyz.device
        H, W = int(settings[0].image_height), int(settings[0].image_width)
        N, f32 = xyz.shape[0], torch.float32
        out = torch.empty((bs, 3, H, W), dtype=f32, device=dev)
        depth = torch.empty((bs, 1, H, W), dtype=f32, device=dev) if opts.depth_alpha else None
        alpha = torch.empty((bs, 1, H, W), dtype=f32, device=dev) if opts.depth_alpha else None
        fmaps = torch.empty((bs, features.shape[1], H, W), dtype=f32, device=dev) if opts.features else None
        feat_grad = opts.features and ctx.needs_input_grad[12]
        radii = torch.empty((N,), dtype=torch.int32, device=dev)  # batch-wide, like the inputs
        cstats = (torch.empty((N,), dtype=f32, device=dev), torch.empty((N,), dtype=f32, device=dev),
                  torch.empty((N,), dtype=torch.int32, device=dev)) if opts.contrib else (None, None, None)
        agrad = torch.zeros((N, 2), dtype=f32, device=dev) if opts.absgrad else None
        dist = torch.empty((bs, 1, H, W), dtype=f32, device=dev) if opts.distortion else None  # (each view keeps its own totals plane in its holder)
        outs = _RZ._Outputs(out, None, depth, alpha, fmaps, *cstats, agrad, dist)
        cur = torch.cuda.current_stream(dev)
        # one HIP stream per sample -- except under graph capture (GPSGS_CHECK=none), where everything stays on the capturing stream
        side = _streams(dev, bs) if (bs > 1 and not torch.cuda.is_current_stream_capturing()) else [cur] * bs
        needs = any(ctx.needs_input_grad[:5]) or feat_grad
        views = []
        with _RZ.defer_capacity_checks():
            for i in range(bs):
                h = _Holder()
                if side[i] is not cur:
                    side[i].wait_stream(cur)
                with torch.cuda.stream(side[i]):
                    _RZ._forward_impl(h, xyz, rgb, opacity, scale, rot, settings[i], needs, opts,
                                      out=dict(color=out[i], radii=radii, depth=_row(depth, i), alpha=_row(alpha, i), feat=_row(fmaps, i),
                                               contrib=cstats, absgrad=agrad, distortion=_row(dist, i)),
                                      rows=_RZ._Rows(offsets, i, cap_rows), features=features, feat_grad=feat_grad)
                views.append(h)
        for i in range(bs):
            if side[i] is not cur:
                cur.wait_stream(side[i])
        # the packed inputs go through save_for_backward (autograd then notices an in-place change between forward and backward); the
        # per-view holders keep only what is not an input: camera matrices, background, radii, workspace.  (pack_views hands out
        # contiguous fp32, which _forward_impl uses as is; should an input ever have been converted on the way in, the holder keeps the
        # converted tensors instead.)
        for h in views:
            s = h.saved
            pairs = ((s.m3, xyz), (s.col, rgb), (s.opa, opacity), (s.sca, scale), (s.rot, rot))
            if all(sv.data_ptr() == t.data_ptr() and sv.numel() == t.numel() for sv, t in pairs):
                h.saved = s._replace(m3=None, col=None, opa=None, sca=None, rot=None)
        ctx.save_for_backward(xyz, rgb, rot, scale, opacity)
        ctx.views, ctx.side, ctx.opts = views, side, opts
        ctx.cams = (view_all, proj_all, campos_all) if opts.camera_grad else None
        ctx.color_grad = bool(ctx.needs_input_grad[1])  # False in stage 2: pack_views marks rgb non-differentiable when no image needs a gradient
        ctx.shapes = tuple(tuple(t.shape) for t in (xyz, rgb, rot, scale, opacity))
        ctx.feat_shape = tuple(features.shape) if feat_grad else None
        ctx.absgrad_out = agrad
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*_RZ._non_differentiable(outs))
        return _RZ._pack_outputs(outs)

    @staticmethod
    def backward(ctx, *grads):
        opts = ctx.opts
        g = _RZ._unpack_outputs(opts, grads, radii=False)  # (None for the statistics and absgrad: not differentiable)
        if g.color is None and g.depth is None and g.alpha is None and g.feat is None and g.distortion is None:
            return (None,) * len(ctx.needs_input_grad)
        views, side = ctx.views, ctx.side
        xyz, rgb, rot, scale, opacity = ctx.saved_tensors
        dev = xyz.device
        f32c = _RZ._map_grad  # fp32, contiguous
        g = _RZ._Outputs(color=f32c(g.color), depth=f32c(g.depth), alpha=f32c(g.alpha), feat=f32c(g.feat), distortion=f32c(g.distortion))
        d_feat = torch.empty(ctx.feat_shape, dtype=torch.float32, device=dev) if ctx.feat_shape is not None else None  # batch-wide, each view writes its rows
        # one gradient buffer per packed tensor (+ one for the unused screen-space gradient); every view's backward writes its own
        # rows, rows behind offsets[-1] (the unused tail of the packed capacity) are never read by the pack backward
        d_xyz, d_rgb, d_rot, d_scale, d_op = (torch.empty(sh, dtype=torch.float32, device=dev) for sh in ctx.shapes)
        d_m2 = torch.empty(ctx.shapes[0], dtype=torch.float32, device=dev)
        # camera gradients: [B, 16], [B, 16], [B, 3] on the device, sample i's rows written by its own backward
        cam_all = None
        if opts.camera_grad:
            cam_all = tuple(torch.empty((len(views), n), dtype=torch.float32, device=dev) if w and t is not None else None
                            for w, t, n in zip(ctx.needs_input_grad[9:12], ctx.cams, (16, 16, 3)))
        cur = torch.cuda.current_stream(dev)
        for i, h in enumerate(views):
            if side[i] is not cur:
                side[i].wait_stream(cur)
            s = h.saved if h.saved.m3 is not None else h.saved._replace(m3=xyz, col=rgb, opa=opacity.reshape(-1), sca=scale, rot=rot)
            with torch.cuda.stream(side[i]):  # (a workspace replaced by the overflow repair is picked up from h.view.ws_box in there)
                _RZ._backward_impl(h, s, _RZ._Outputs(color=_row(g.color, i), depth=_row(g.depth, i), alpha=_row(g.alpha, i), feat=_row(g.feat, i),
                                                      distortion=_row(g.distortion, i)),
                                   (d_xyz, d_rgb, d_op, d_scale, d_rot, d_m2), ctx.color_grad,
                                   None if cam_all is None else tuple(_row(c, i) for c in cam_all), d_feat)
        for i in range(len(views)):
            if side[i] is not cur:
                cur.wait_stream(side[i])
        if opts.absgrad_sink is not None:  # (every view's rows of ctx.absgrad_out are written: the holders carry the tensor)
            opts.absgrad_sink(ctx.absgrad_out)
        d_cam = (None, None, None)
        if cam_all is not None:
            d_cam = tuple(_RZ._cam_grad_as(c, t) for c, t in zip(cam_all, ctx.cams))
        return (d_xyz, (d_rgb if ctx.color_grad else None), d_rot, d_scale, d_op, None, None, None, None, *d_cam, d_feat)[:len(ctx.needs_input_grad)]


def render(data, idx, pts_xyz, pts_rgb, rotations, scales, opacity, bg_color, grad_arena=None, antialiasing=False, camera_grad=False):
    """Render one novel view.  Same arguments and return value as the reference's render(): returns image [3,H,W].
    (grad_arena: internal, see pts2render.)  antialiasing=True: the opacity-compensated 2D filter (rasterizer.rasterize_gaussians).
    camera_grad=True: data['novel_view']['world_view_transform'], ['full_proj_transform'] and ['camera_center'] receive the gradient of
    sample idx's camera (through their [idx] slices) when they require one."""
    opts = _RZ._view_options(None, False, antialiasing, camera_grad)
    return _render_view(data, idx, pts_xyz, pts_rgb, rotations, scales, opacity, bg_color, grad_arena, opts, retain_grad=True).color


def _render_view(data, idx, pts_xyz, pts_rgb, rotations, scales, opacity, bg_color, grad_arena, opts, features=None, retain_grad=False):
    """One novel view with the opt-ins of `opts` (a rasterizer._ViewOptions) -> rasterizer._Outputs.  Through the GaussianRasterizer module, as the
    reference's render() goes: constructing it is what arms the opt-in accelerate hooks on first use.  retain_grad: the screen-space points keep
    their gradient, as the reference's render() asks (render_ex never did)."""
    bg = _bg_tensor(bg_color, pts_xyz.device)
    screenspace_points = torch.zeros_like(pts_xyz, dtype=torch.float32, requires_grad=True, device=pts_xyz.device) + 0
    if retain_grad:
        try:
            screenspace_points.retain_grad()
        except Exception:
            pass
    rasterizer = GaussianRasterizer(raster_settings=_settings(data['novel_view'], idx, bg))
    out = rasterizer(means3D=pts_xyz, means2D=screenspace_points, shs=None, colors_precomp=pts_rgb, opacities=opacity, scales=scales,
                     rotations=rotations, cov3D_precomp=None, grad_arena=grad_arena, return_depth_alpha=opts.depth_alpha,
                     antialiasing=opts.antialiasing, camera_grad=opts.camera_grad, features=features, return_contrib=opts.contrib,
                     return_absgrad=opts.absgrad_sink or opts.absgrad, return_distortion=opts.distortion)
    return _RZ._unpack_outputs(opts, out)


def render_ex(data, idx, pts_xyz, pts_rgb, rotations, scales, opacity, bg_color, grad_arena=None, antialiasing=False, camera_grad=False,
              features=None, contrib=False, absgrad=False, distortion=False):
    """render() plus the depth and alpha maps of the novel view: {'img': [3,H,W], 'depth': [1,H,W], 'alpha': [1,H,W]}, all differentiable.
    depth = sum_i z_i alpha_i T_i with z_i the view-space depth -- NOT normalised: depth / alpha is the expected depth where alpha > 0 --
    and alpha = sum_i alpha_i T_i (the accumulated opacity, 1 - final transmittance); both have background 0, whatever bg_color is.
    The image is what render() returns up to the compositing family: the maps come from the VALU kernels, render() uses GPSGS_COMPOSITE.
    antialiasing=True: as render()'s; the maps then see the filtered opacities too.  camera_grad=True: as render()'s, the maps' gradients
    included.  features [P, F] (1 <= F <= 64): also 'feat' [F,H,W] = sum_i f_i alpha_i T_i, background 0 (for a feature background add
    (1 - alpha) bg_f), differentiable in the features and the geometry (rasterizer.rasterize_gaussians).  contrib=True: also the per-Gaussian
    contribution statistics of the view, 'contrib_weight' (fp32 [P], sum over pixels of alpha T), 'contrib_max' (fp32 [P], its maximum) and
    'contrib_pixels' (int32 [P], pixels blended into), not differentiable (rasterizer.rasterize_gaussians(return_contrib=True)); not with
    features.  absgrad=True: also 'absgrad' (fp32 [P, 2]), the absolute screen-space gradient sum_p |dL_p/dmean2D_i| in the units of the screen-space
    gradient: zeros until a backward through the view has run, then overwritten in place by each one; not differentiable
    (rasterizer.rasterize_gaussians(return_absgrad=True)); not with features.  distortion=True: also 'distortion' [1,H,W], the depth-distortion map
    sum_i sum_j w_i w_j |z_i - z_j| of the view's blend in raw view-space depth units (not normalised, background 0), differentiable
    (rasterizer.rasterize_gaussians(return_distortion=True)); not with features, contrib or absgrad."""
    opts = _RZ._view_options(None, True, antialiasing, camera_grad, features, contrib, absgrad, distortion)
    o = _render_view(data, idx, pts_xyz, pts_rgb, rotations, scales, opacity, bg_color, grad_arena, opts, features)
    r = {'img': o.color, 'depth': o.depth, 'alpha': o.alpha}
    if opts.features:
        r['feat'] = o.feat
    if opts.absgrad:
        r['absgrad'] = o.absgrad
    if opts.distortion:
        r['distortion'] = o.distortion
    if opts.contrib:
        r['contrib_weight'], r['contrib_max'], r['contrib_pixels'] = o.contrib_weight, o.contrib_max, o.contrib_pixels
    return r


def _settings(nv, idx, bg, view=None, proj=None):
    return GaussianRasterizationSettings(
        image_height=int(nv['height'][idx]), image_width=int(nv['width'][idx]),
        tanfovx=math.tan(_scalar(nv['FovX'][idx]) * 0.5), tanfovy=math.tan(_scalar(nv['FovY'][idx]) * 0.5),
        bg=bg, scale_modifier=1.0, viewmatrix=(nv['world_view_transform'] if view is None else view)[idx],
        projmatrix=(nv['full_proj_transform'] if proj is None else proj)[idx],
        sh_degree=3, campos=nv['camera_center'][idx], prefiltered=False, debug=False)


def _to_device_once(t, dev):
    """[B,4,4] camera matrices of the whole batch in ONE copy (H1: in training they arrive as pinned CPU tensors; per-sample slices
    would each cost their own small H2D copy)."""
    if t.device != dev or t.dtype != torch.float32 or t.requires_grad or not t.is_contiguous():
        t = t.detach().to(device=dev, dtype=torch.float32, non_blocking=True).contiguous()
    return t


_CONTRIB_KEYS = ('contrib_weight', 'contrib_max', 'contrib_pixels')


def _write_contrib_maps(data, stats, row_of_pixel):
    """The packed rows' statistics -> data[view][key] [B,1,H,W] for lmain and rmain (pack.unpack_rows: device index ops, no host sync)."""
    from .pack import VIEWS, unpack_rows

    for key, vals in zip(_CONTRIB_KEYS, stats):
        maps = unpack_rows(vals, row_of_pixel)
        for v, view in enumerate(VIEWS):
            H, W = int(data[view]['img'].shape[2]), int(data[view]['img'].shape[3])
            data[view][key] = maps[:, v].reshape(-1, 1, H, W)


def _absgrad_maps(data):
    """data['lmain' | 'rmain']['absgrad'] = zeros [B,2,H,W] (pts2render(with_absgrad=True)) -> the two maps"""
    from .pack import VIEWS

    maps = []
    for view in VIEWS:
        img = data[view]['img']
        data[view]['absgrad'] = torch.zeros((img.shape[0], 2, int(img.shape[2]), int(img.shape[3])), dtype=torch.float32, device=img.device)
        maps.append(data[view]['absgrad'])
    return maps


def _fill_absgrad_maps(maps, absgrad, rows, first_row=0):
    """absgrad [n, 2] of the packed rows first_row .. first_row + n -> the source pixels of maps[v] ([b,2,H,W] each); rows: pack_views' row_of_pixel
    [b, views, S2] of the same samples (a pixel whose pts_valid is false: -1 -> 0).  Device index ops only, no host synchronisation; runs inside the
    render node's backward."""
    idx = rows.to(torch.int64) - first_row
    vals = torch.where((idx >= 0).unsqueeze(-1), absgrad[idx.clamp(min=0)], absgrad.new_zeros(()))  # [b, views, S2, 2]
    for v, m in enumerate(maps):
        m.copy_(vals[:, v].permute(0, 2, 1).reshape(m.shape))


def _write_outputs(data, o, row_of_pixel):
    """The batch-wide rasterizer._Outputs of a pts2render call -> data['novel_view']['img_pred'], 'depth_pred' / 'alpha_pred', 'feat_pred' and the
    contribution maps of the source views.  (The absgrad maps exist already -- _absgrad_maps -- and are filled by the backward.)"""
    nv = data['novel_view']
    nv['img_pred'] = o.color
    if o.depth is not None:
        nv['depth_pred'], nv['alpha_pred'] = o.depth, o.alpha
    if o.feat is not None:
        nv['feat_pred'] = o.feat
    if o.distortion is not None:
        nv['distortion_pred'] = o.distortion
    if o.contrib_weight is not None:
        _write_contrib_maps(data, (o.contrib_weight, o.contrib_max, o.contrib_pixels), row_of_pixel)


def pts2render(data, bg_color, with_depth_alpha=False, antialiasing=False, camera_grad=False, feature_key=None, with_contrib=False,
               with_absgrad=False, with_distortion=False):
    """Same contract as the reference's pts2render(): writes data['novel_view']['img_pred'] = [B,3,H,W].  with_depth_alpha=True (opt-in)
    also writes 'depth_pred' and 'alpha_pred' [B,1,H,W] (render_ex: unnormalised depth sum_i z_i alpha_i T_i, accumulated opacity, background 0).
    antialiasing=True (opt-in): every sample is rendered with the opacity-compensated 2D filter (render(antialiasing=True)).
    camera_grad=True (opt-in): each sample's camera gradient reaches data['novel_view']['world_view_transform'], ['full_proj_transform'] and
    ['camera_center'] ([B,4,4], [B,4,4], [B,3]) where they require one -- with the bits of B render_ex / render calls.
    feature_key (opt-in): data['lmain'][feature_key] and data['rmain'][feature_key], each [B,F,H,W] (1 <= F <= 64), are packed with the
    same validity mask and row order as 'img' (pack.pack_features: torch index ops, no host sync) and splatted with the image's blend weights:
    'feat_pred' [B,F,H,W] (render_ex(features=...)), differentiable back to the per-view maps.
    with_contrib=True (opt-in): every Gaussian's contribution statistics in the novel view (render_ex(contrib=True)) go back to the source pixel it
    came from -- data['lmain'] and data['rmain'] get 'contrib_weight', 'contrib_max' (fp32) and 'contrib_pixels' (int32), each [B,1,H,W], 0 where
    pts_valid is false.  Not differentiable; not with feature_key (RuntimeError before anything is launched).
    with_absgrad=True (opt-in): data['lmain'] and data['rmain'] get 'absgrad' [B,2,H,W], zeros now; the BACKWARD of the render node writes every
    Gaussian's absolute screen-space gradient (render_ex(absgrad=True)) to the source pixel it came from, 0 where pts_valid is false -- overwritten by
    each backward, with device index ops only.  Not differentiable; not with feature_key (RuntimeError mentioning features, before any launch).
    with_distortion=True (opt-in): also writes 'distortion_pred' [B,1,H,W], every sample's depth-distortion map (render_ex(distortion=True)),
    differentiable back to the source views' maps.  Not with feature_key, with_contrib or with_absgrad (RuntimeError before any launch).

    The flatten / mask-gather / concat / rgb-affine of lib/GaussianRender.py:15-34 runs as one fused op for the whole batch
    (pack.py: 3 launches, no sync) instead of 10 boolean-index gathers + syncs per sample, and the B + 1 row offsets STAY ON THE
    DEVICE: the B renders run as ONE autograd node with the samples on B HIP streams, every view reading its row range of the packed
    arrays from device memory (_RenderBatch) -- with GPSGS_CHECK=none the whole pack -> render -> loss -> backward chain is launches only
    and can be captured into ONE HIP graph (tests/test_gpu_pack.py).  GPSGS_PTS2RENDER=loop restores the literal per-sample loop of
    render() calls, which reads the offsets back (also taken when the samples differ in image size)."""
    from .pack import pack_views

    bs = data['lmain']['img'].shape[0]
    feats = row_of_pixel = None
    if with_contrib and feature_key is not None:
        raise RuntimeError("gps_gaussian_amd: with_contrib cannot be combined with feature_key")
    if with_absgrad and feature_key is not None:
        raise RuntimeError("gps_gaussian_amd: with_absgrad cannot be combined with feature_key (features)")
    if with_distortion and (feature_key is not None or with_contrib or with_absgrad):
        raise RuntimeError(_RZ._DISTORTION_ALONE.replace("return_distortion", "with_distortion")
                           % ("feature_key (features)" if feature_key is not None else "with_contrib" if with_contrib else "with_absgrad"))
    if with_contrib or with_absgrad or feature_key is not None:
        xyz, rgb, rot, scale, opacity, offsets, row_of_pixel = pack_views(data, return_rows=True)
        if feature_key is not None:
            from .pack import pack_features
            feats = pack_features(data, feature_key, row_of_pixel)
    else:
        xyz, rgb, rot, scale, opacity, offsets = pack_views(data)
    opts = _RZ._view_options(None, with_depth_alpha, antialiasing, camera_grad, feats, with_contrib, with_absgrad, with_distortion)
    nv = data['novel_view']
    dev = xyz.device
    sizes_hw = {(int(nv['height'][i]), int(nv['width'][i])) for i in range(bs)}
    if os.environ.get("GPSGS_PTS2RENDER", "batch") != "loop" and len(sizes_hw) == 1:
        bg = _bg_tensor(bg_color, dev)
        view, proj = _to_device_once(nv['world_view_transform'], dev), _to_device_once(nv['full_proj_transform'], dev)
        settings = [_settings(nv, i, bg, view, proj) for i in range(bs)]
        if opts.absgrad:
            amaps = _absgrad_maps(data)
            opts = opts._replace(absgrad_sink=lambda a: _fill_absgrad_maps(amaps, a, row_of_pixel))
        cams = (nv['world_view_transform'], nv['full_proj_transform'], nv['camera_center']) if opts.camera_grad else (None, None, None)
        if opts == _RZ._DEFAULT_OPTIONS:  # the default call keeps the eight arguments it always had (rasterizer._rasterize says why)
            out = _RenderBatch.apply(xyz, rgb, rot, scale, opacity, offsets, settings, xyz.shape[0] // bs)  # no read-back of the offsets
        else:
            out = _RenderBatch.apply(xyz, rgb, rot, scale, opacity, offsets, settings, xyz.shape[0] // bs, opts, *cams, feats)
        _write_outputs(data, _RZ._unpack_outputs(opts, out, radii=False), row_of_pixel)
        return data
    return _pts2render_loop(data, bg_color, (xyz, rgb, rot, scale, opacity), offsets.tolist(), opts, feats, row_of_pixel)


def _pts2render_loop(data, bg_color, packed, offs, opts=_RZ._DEFAULT_OPTIONS, feats=None, row_of_pixel=None):
    """The per-sample form: one render() (one rasteriser autograd node) per sample, on the current stream.  opts: the call's
    rasterizer._ViewOptions; row_of_pixel (pack_views'): needed with opts.contrib (the statistics go back to their source pixels) and with
    opts.absgrad (every sample's node fills its slice of the absgrad maps in its backward)."""
    bs = data['lmain']['img'].shape[0]
    xyz, rgb, rot, scale, opacity = packed
    # ONE split per packed tensor (its backward is one concatenation of the per-sample gradients); B Python slices would make
    # autograd zero-fill and add a full-size gradient per sample and tensor (measured: 0.6 ms of a 4.1 ms stage-2 iteration)
    sizes = [offs[i + 1] - offs[i] for i in range(bs)] + [xyz.shape[0] - offs[bs]]
    if any(t.requires_grad for t in packed):
        # gradient arenas: one buffer per packed tensor; every sample's rasteriser backward writes its rows in place and the
        # split's backward hands the whole buffer on (no per-sample allocation, no concatenation).  Rows behind offs[bs] are
        # never read by the pack backward.
        arenas = [torch.empty(t.shape, dtype=torch.float32, device=t.device) for t in packed]
        a_parts = [a.split(sizes) for a in arenas]
    else:
        arenas, a_parts = [None] * 5, None
    parts = [_SplitRows.apply(t, sizes, a) for t, a in zip(packed, arenas)]
    # the features' split has no arena (the rasteriser backward allocates dL/dfeatures per sample): its backward concatenates the samples'
    # gradients, and the empty device tensor only gives the zero-filled tail its device
    f_parts = _SplitRows.apply(feats, sizes, feats.new_empty((0, feats.shape[1]))) if feats is not None else None
    out = []
    dev = xyz.device
    cur = torch.cuda.current_stream(dev)
    # GPSGS_PTS2RENDER_STREAMS=1: each sample on its own HIP stream also in this form (measured no gain: through B autograd nodes the
    # batch loop is host-bound, tools/stage2_ab.py -- the reason _RenderBatch exists)
    concurrent = bs > 1 and not torch.cuda.is_current_stream_capturing() and os.environ.get("GPSGS_PTS2RENDER_STREAMS", "0") == "1"
    side = _streams(dev, bs) if concurrent else [cur] * bs
    amaps = _absgrad_maps(data) if opts.absgrad else None
    # any map or statistic is wanted: every sample is rendered as render_ex renders it, with the depth / alpha maps too; else as render() does
    full = opts.depth_alpha or opts.features or opts.contrib or opts.absgrad or opts.distortion
    view_opts = opts._replace(depth_alpha=True) if full else opts
    with _RZ.defer_capacity_checks():
        for i in range(bs):
            # arena order expected by the rasteriser: means3D, colours, opacities, scales, rotations
            ga = (a_parts[0][i], a_parts[1][i], a_parts[4][i], a_parts[3][i], a_parts[2][i]) if a_parts is not None else None
            if side[i] is not cur:
                side[i].wait_stream(cur)
            sink = None
            if amaps is not None:  # sample i's rows start at offs[i] of the packed order row_of_pixel speaks of
                def sink(a, i=i):
                    _fill_absgrad_maps([m[i:i + 1] for m in amaps], a, row_of_pixel[i:i + 1], offs[i])
            with torch.cuda.stream(side[i]):
                out.append(_render_view(data, i, parts[0][i], parts[1][i], parts[2][i], parts[3][i], parts[4][i], bg_color, ga,
                                        view_opts._replace(absgrad_sink=sink), f_parts[i] if feats is not None else None, retain_grad=not full))
    for i in range(bs):
        if side[i] is not cur:
            cur.wait_stream(side[i])
            for t in _RZ._pack_outputs(out[i]):
                t.record_stream(cur)

    def batch(name):
        return torch.cat([getattr(o, name).unsqueeze(0) for o in out], dim=0)

    def packed_rows(name):  # the samples' statistics in packed row order (rows behind offs[bs] are never looked up: zeros)
        return torch.cat([getattr(o, name) for o in out] + [getattr(out[0], name).new_zeros((xyz.shape[0] - offs[bs],))])

    stats = {k: packed_rows(k) for k in _CONTRIB_KEYS} if opts.contrib else {}
    whole = _RZ._Outputs(color=batch('color'), depth=batch('depth') if opts.depth_alpha else None, alpha=batch('alpha') if opts.depth_alpha else None,
                         feat=batch('feat') if opts.features else None, distortion=batch('distortion') if opts.distortion else None, **stats)
    _write_outputs(data, whole, row_of_pixel)
    return data


def pts2render_unfused(data, bg_color):
    """Literal mirror of the reference's pts2render (per-sample torch mask-gathers); kept as the comparison baseline."""
    bs = data['lmain']['img'].shape[0]
    out = []
    for i in range(bs):
        parts = [[], [], [], [], []]
        for view in ('lmain', 'rmain'):
            d = data[view]
            valid = d['pts_valid'][i, :]
            maps = (d['xyz'][i], d['img'][i].permute(1, 2, 0).reshape(-1, 3), d['rot_maps'][i].permute(1, 2, 0).reshape(-1, 4),
                    d['scale_maps'][i].permute(1, 2, 0).reshape(-1, 3), d['opacity_maps'][i].permute(1, 2, 0).reshape(-1, 1))
            for lst, m in zip(parts, maps):
                lst.append(m[valid])
        xyz, rgb, rot, scale, opacity = (torch.cat(p, dim=0) for p in parts)
        rgb = rgb * 0.5 + 0.5
        out.append(render(data, i, xyz, rgb, rot, scale, opacity, bg_color=bg_color).unsqueeze(0))
    data['novel_view']['img_pred'] = torch.cat(out, dim=0)
    return data
