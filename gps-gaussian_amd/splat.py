"""Z-buffer point splat of the stage-1 validation render (lib/TaichiRender.py of the reference), on the GPU.

`zsplat(pts, mask, depth, color)` is `render_respective_color` (lib/TaichiRender.py:13-24) for any number of source views at once;
`flow2render(data)` and `TaichiRenderBatch(bs, res).flow2render(data)` are `TaichiRenderBatch.flow2render` (:26-60) fused into one scatter
launch (up_flow2render_dev): flow2depth, depth2pc (the bits of unproject.py's kernel), perspective into the novel view, inverse depth and the
splat of both source views, cameras read from device memory (no host synchronisation in the middle of validation).

Per target pixel the result is the SEQUENTIAL one -- lmain's points in index order, then rmain's, each doing
`if z >= depth[px]: depth[px] = z; colour[px] = rgb` -- deterministically; the reference's Taichi kernel writes the colour after a separate
atomic_max and can keep the colour of the farther of two points landing together.  No gradients (the reference's path has none) and no CPU fallback.
"""
import torch

from . import _capi
from ._ops import call, ptr
from .unproject import _cams


def _gpu(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("gps_gaussian_amd.splat: %s must be a tensor on a GPU (no CPU fallback)" % what)
    return t


def zsplat(pts, mask, depth, color):
    """In place, like render_respective_color: pts [V,B,N,6] (or [B,N,6]) = (x, y, inverse depth, r, g, b), mask [V,B,N] (or [V,B,N,1],
    [B,N,1], [B,N]); depth [B,res,res] or [B,1,res,res] and color [B,3,res,res] are fp32, contiguous and updated in place.  Returns (depth, color)."""
    for t, what in ((pts, "pts"), (mask, "mask"), (depth, "depth"), (color, "color")):
        _gpu(t, what)
    if depth.requires_grad or color.requires_grad:
        raise RuntimeError("gps_gaussian_amd.splat.zsplat: the splat has no gradient; pass buffers that do not require grad")
    if pts.dim() == 3:
        pts = pts.unsqueeze(0)
    V, B, N, six = pts.shape
    if six != 6:
        raise RuntimeError("zsplat: pts must end in 6 values (x, y, z, r, g, b), got %s" % (tuple(pts.shape),))
    res = depth.shape[-1]
    if depth.numel() != B * res * res or depth.shape[-2] != res or tuple(color.shape) != (B, 3, res, res):
        raise RuntimeError("zsplat: depth must be [B,(1,)res,res] and color [B,3,res,res] for B=%d, got %s and %s"
                           % (B, tuple(depth.shape), tuple(color.shape)))
    for t, what in ((depth, "depth"), (color, "color")):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError("zsplat: %s is updated in place and must be contiguous fp32" % what)
    dev = depth.device
    with torch.no_grad():
        q = pts.detach().to(device=dev, dtype=torch.float32).contiguous()
        m = mask.detach().to(device=dev, dtype=torch.float32).reshape(V, B, N).contiguous()
        lib = _capi.lib()
        scratch = torch.empty((max(1, lib.up_splat_scratch_bytes(B, res)),), dtype=torch.uint8, device=dev)
        call("up_zsplat", dev, V, B, N, res, ptr(q), ptr(m), ptr(depth), ptr(color), ptr(scratch), scratch.numel())
    return depth, color


def render_views(lmain, rmain, intr, extr, res=None, batch=None, with_points=False):
    """The fused flow2render of the two source-view dicts ('flow_pred', 'mask', 'img', 'ref_intr', 'intr', 'extr', 'Tf_x') into the novel view
    with intrinsics `intr` [B,3,3] and extrinsics `extr` [B,3,4].  Renders the first `batch` samples (default all); the others stay -1.
    Returns (img_pred [B,3,res,res], pts [2,B,S*S,3] of projected (x, y, 1/z) with NaN for invalid points, or None)."""
    flow = _gpu(lmain['flow_pred'], "lmain['flow_pred']")
    dev = flow.device
    B, _, S, S_ = flow.shape
    if S != S_:
        raise RuntimeError("flow2render: depth2pc assumes square maps")
    res = S if res is None else int(res)
    nb = B if batch is None else max(0, min(int(batch), B))
    views = []
    for name, view in (("lmain", lmain), ("rmain", rmain)):
        for k in ("flow_pred", "mask", "img"):
            _gpu(view[k], "%s[%r]" % (name, k))
        if tuple(view['flow_pred'].shape) != (B, 1, S, S) or view['img'].shape[-3:] != (3, S, S):
            raise RuntimeError("flow2render: %s flow_pred must be [B,1,S,S] and img [B,3,S,S]" % name)
        views.append(view)
    _gpu(intr, "novel_view['intr']")
    _gpu(extr, "novel_view['extr']")
    img_pred = torch.full((B, 3, res, res), -1.0, dtype=torch.float32, device=dev)
    pts = torch.empty((2, nb, S * S, 3), dtype=torch.float32, device=dev) if with_points else None
    if nb == 0:
        return img_pred, pts
    with torch.no_grad():
        f = [v['flow_pred'].detach()[:nb].to(dtype=torch.float32).contiguous() for v in views]
        m = [v['mask'].detach()[:nb, 0].to(device=dev, dtype=torch.float32).contiguous() for v in views]
        im = [v['img'].detach()[:nb].to(device=dev, dtype=torch.float32).contiguous() for v in views]
        cams = torch.cat([_cams(v['ref_intr'][:nb], v['intr'][:nb], v['extr'][:nb], v['Tf_x'][:nb], nb, dev) for v in views], dim=0)
        novel = torch.cat([intr.detach()[:nb].reshape(nb, 9), extr.detach()[:nb, :3, :4].reshape(nb, 12)], dim=1).to(dtype=torch.float32).contiguous()
        lib = _capi.lib()
        scratch = torch.empty((max(1, lib.up_splat_scratch_bytes(nb, res)),), dtype=torch.uint8, device=dev)
        call("up_flow2render_dev", dev, nb, S, res, ptr(f[0]), ptr(f[1]), ptr(m[0]), ptr(m[1]), S * S, ptr(im[0]), ptr(im[1]), ptr(cams), ptr(novel),
             ptr(scratch), scratch.numel(), ptr(img_pred), ptr(pts))
    return img_pred, pts


def flow2render(data, res=None, batch=None):
    """TaichiRenderBatch.flow2render's contract: reads data['lmain'|'rmain'] and data['novel_view']['intr'|'extr'], writes
    data['novel_view']['img_pred'] [B,3,res,res] (-1 where no point lands) and returns data."""
    nv = data['novel_view']
    nv['img_pred'], _ = render_views(data['lmain'], data['rmain'], nv['intr'], nv['extr'], res=res, batch=batch)
    return data


class TaichiRenderBatch:
    """Drop-in for lib/TaichiRender.py's class.  Like the reference (whose kernel loops over a (bs, res*res) field), it renders the first `bs`
    samples of the batch; the rest of img_pred keeps the -1 background."""

    def __init__(self, bs, res):
        self.bs = bs
        self.res = res

    def flow2render(self, data):
        from . import accelerate
        accelerate.calls["splat"] += 1
        return flow2render(data, res=self.res, batch=self.bs)
