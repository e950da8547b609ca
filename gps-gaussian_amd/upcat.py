"""The regresser's decoder glue -- nn.Upsample(scale_factor=2, mode="bilinear") followed by torch.cat with the skip tensors -- forward and backward,
as one pass over the streaming kernels of csrc/upcat.hip (uc_forward / uc_backward of include/gpsgs.h).

GSRegresser.forward (lib/gs_parm_network.py:56-67) upsamples a decoder's output and concatenates it with the image and depth features of the
next finer level, three times, the last time at full resolution.  ATen writes the upsampled tensor, copies it into the concatenation (the
reference concatenates the two feature tensors first: a third copy of those channels), and accumulates the upsample's backward with atomics -- the
one node of the regresser's backward that `torch.use_deterministic_algorithms` lists.  Here one kernel reads the half-resolution tensor and the
skips and writes the concatenation once; the backward is a gather with a fixed order, the same bits on every run (DESIGN.md "Decoder glue").

  upsample2x_cat(a, *skips)                  the op (autograd); GPU tensors only, like every other op of this package
  regresser_forward(reg, img, depth, feat)   GSRegresser.forward stated from its data flow, the three glue sites on the op
  convert(model)                             binds regresser_forward to every module of a tree that has the regresser's members
  tile()                                     the forward's output tile (rows, columns)
  calls                                      {"upcat": sites that ran fused, "upcat_passthrough": sites that went to `up` + torch.cat}

There is no GPSGS_ACCELERATE name for this op: it is reached through convert(model) in the caller's own script."""
import ctypes
import types

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd.function import once_differentiable

from . import _ops
from ._ops import aligned16, call, ptr

MAX_SKIPS = 3
calls = {"upcat": 0, "upcat_passthrough": 0}


def tile():
    """(rows, columns) of the output tile one workgroup of the forward's upsampled part computes (uc_tile)."""
    return _ops.tile("uc_tile")


def _channels(counts):
    return (ctypes.c_int * len(counts))(*counts) if counts else None


class _UpCat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, *skips):
        every = (a,) + skips
        if not all(t.is_cuda for t in every):
            raise RuntimeError("gps_gaussian_amd: upsample2x_cat inputs must live on a GPU (no CPU fallback)")
        if len(skips) > MAX_SKIPS or any(t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous() or t.device != a.device for t in every):
            raise RuntimeError("gps_gaussian_amd: upsample2x_cat takes contiguous fp32 tensors on one GPU: a [N, Ca, h, w] and at most %d skips "
                               "[N, C_k, 2h, 2w]" % MAX_SKIPS)
        N, Ca, h, w = a.shape
        if a.numel() == 0 or any(s.shape[0] != N or s.shape[1] < 1 or tuple(s.shape[2:]) != (2 * h, 2 * w) for s in skips):
            raise RuntimeError("gps_gaussian_amd: upsample2x_cat: unsupported shapes: a %s, skips %s" % (tuple(a.shape), [tuple(s.shape) for s in skips]))
        counts = tuple(int(s.shape[1]) for s in skips)
        ac, sc = aligned16(a.detach()), [aligned16(s.detach()) for s in skips]
        out = torch.empty((N, Ca + sum(counts), 2 * h, 2 * w), dtype=torch.float32, device=a.device)
        ptrs = (ctypes.c_void_p * len(sc))(*[ptr(s) for s in sc]) if sc else None
        call("uc_forward", a.device, ptr(ac), ptrs, _channels(counts), len(sc), N, Ca, h, w, ptr(out))
        ctx.dims = (counts, N, Ca, h, w)     # nothing but shapes is saved
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        counts, N, Ca, h, w = ctx.dims
        needs = ctx.needs_input_grad
        da = None
        if needs[0]:
            dc = aligned16(dout.to(torch.float32))
            da = torch.empty((N, Ca, h, w), dtype=torch.float32, device=dout.device)    # every element is written
            call("uc_backward", dout.device, ptr(dc), _channels(counts), len(counts), N, Ca, h, w, ptr(da))
        grads, c0 = [], Ca
        for k, c in enumerate(counts):
            grads.append(dout[:, c0:c0 + c] if needs[1 + k] else None)                  # a view, as ATen's cat backward returns
            c0 += c
        return (da,) + tuple(grads)


def upsample2x_cat(a, *skips):
    """torch.cat([nn.Upsample(scale_factor=2, mode="bilinear")(a), *skips], dim=1) for contiguous fp32 GPU tensors a [N, Ca, h, w] and at most
    three skips [N, C_k, 2h, 2w]; anything else is a RuntimeError.  Exact fp32 arithmetic in a fixed order (csrc/upcat.hip); the skip channels
    are copied bit for bit.  a.grad is computed only if a requires grad (a gather, no atomics: the same bits on every run); a skip's gradient is
    the matching channel slice of the output's gradient, returned as a view."""
    return _UpCat.apply(a, *skips)


def _plain_up(up):
    """nn.Upsample as the regresser builds it: a scale of 2 on both axes, bilinear, align_corners None or False (no explicit size)."""
    if not isinstance(up, nn.Upsample) or up.mode != "bilinear" or up.size is not None or up.align_corners not in (None, False):
        return False
    sf = up.scale_factor
    sf = tuple(sf) if isinstance(sf, (tuple, list)) else (sf, sf)
    return len(sf) == 2 and all(float(f) == 2.0 for f in sf)


def _dense(t, dev):
    return torch.is_tensor(t) and t.is_cuda and t.device == dev and t.dim() == 4 and t.dtype == torch.float32 and t.is_contiguous() and t.numel() > 0


def _fusable(up, a, skips):
    if not torch.is_tensor(a) or not a.is_cuda or torch.is_autocast_enabled() or len(skips) > MAX_SKIPS:
        return False                                 # ... inside autocast ATen decides the dtypes
    if not all(_dense(t, a.device) for t in (a,) + tuple(skips)) or not _plain_up(up):
        return False
    N, _, h, w = a.shape
    return all(s.shape[0] == N and tuple(s.shape[2:]) == (2 * h, 2 * w) for s in skips)


def _glue(reg, a, *skips):
    """One glue site: the fused op where it applies, else the module's own `up` and torch.cat (which is what the reference computes, bit for bit:
    its intermediate concatenation of the two feature tensors only copies).  Counted in `calls`."""
    if _fusable(reg.up, a, skips):
        calls["upcat"] += 1
        return _UpCat.apply(a, *skips)
    calls["upcat_passthrough"] += 1
    return torch.cat([reg.up(a)] + list(skips), dim=1)


def regresser_forward(reg, img, depth, img_feat):
    """GSRegresser.forward from its data flow: the depth encoder's three levels join the image encoder's; the coarsest pair is concatenated and
    decoded, and each decoder's output is upsampled and joined with the next finer pair (at full resolution: with the image and the depth
    themselves) before the next decoder (the output convolution); the three heads read the last hidden tensor.  Returns (rotation, scale,
    opacity) as the reference does: the rotation normalised over its channels, the scale clamped at 0.01."""
    img1, img2, img3 = img_feat
    dep1, dep2, dep3 = reg.depth_encoder(depth)
    x = reg.decoder3(torch.cat([img3, dep3], dim=1))
    x = reg.decoder2(_glue(reg, x, img2, dep2))
    x = reg.decoder1(_glue(reg, x, img1, dep1))
    x = reg.out_relu(reg.out_conv(_glue(reg, x, img, depth)))
    rot = F.normalize(reg.rot_head(x), dim=1)
    scale = torch.clamp_max(reg.scale_head(x), 0.01)
    return rot, scale, reg.opacity_head(x)


MEMBERS = ("depth_encoder", "decoder1", "decoder2", "decoder3", "up", "out_conv", "out_relu", "rot_head", "scale_head", "opacity_head")


def convert(model):
    """Every module of `model`'s tree (the model itself included) that has the regresser's members (MEMBERS) gets regresser_forward bound as
    that instance's `forward`.  Parameters, buffers, submodules and the state_dict are untouched, so this composes with the conversions that change
    submodule classes (gshead, conv3x3, conv1x1, groupnorm) in any order.  Idempotent; returns the number of modules newly bound."""
    n = 0
    for m in model.modules():
        if all(isinstance(getattr(m, name, None), nn.Module) for name in MEMBERS) \
                and getattr(m.__dict__.get("forward"), "__func__", None) is not regresser_forward:
            m.forward = types.MethodType(regresser_forward, m)
            n += 1
    return n
