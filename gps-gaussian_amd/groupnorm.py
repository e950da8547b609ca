"""GroupNorm, forward and backward, on the HIP kernels of csrc/group_norm.hip (gn_forward / gn_backward of include/gpsgs.h).

ATen normalises one (sample, group) row per workgroup; the reference's feature extractor builds `GroupNorm(planes // 8, planes)`, 8..24 rows of up
to two million elements, so most of the chip idles while a handful of CUs stream.  The kernels here cut every row into chunks of
`_capi.lib().gn_chunk_elems()` elements, one workgroup each (DESIGN.md "GroupNorm").

  group_norm(x, num_groups, weight, bias, eps)   the op (autograd); GPU tensors only, like every other op of this package
  FusedGroupNorm                                 nn.GroupNorm with `forward` on that op; whatever the op does not take goes to nn.GroupNorm.forward
  convert(module)                                turn every nn.GroupNorm of a module tree into a FusedGroupNorm, in place

`GPSGS_ACCELERATE=groupnorm` makes the reference's extractor classes call convert() on themselves (accelerate.py)."""
import ctypes as C

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _capi, accelerate

_DTYPES = {torch.float32: 0, torch.float16: 1}


def _aligned(t):
    """Contiguous and 16-byte aligned (a fresh allocation always is; a view into a larger tensor may start anywhere)."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class _GroupNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, num_groups, weight, bias, eps):
        lib = _capi.lib()
        if not x.is_cuda:
            raise RuntimeError("gps_gaussian_amd: group_norm input must live on a GPU (no CPU fallback)")
        if x.dtype not in _DTYPES:
            raise RuntimeError("gps_gaussian_amd: group_norm takes fp32 or fp16 input, not %s" % x.dtype)
        if x.dim() < 2 or weight is None or bias is None:
            raise RuntimeError("gps_gaussian_amd: group_norm needs an [N, C, ...] input, a weight and a bias")
        N, Cn, G = x.shape[0], x.shape[1], int(num_groups)
        if G <= 0 or Cn % G != 0 or weight.numel() != Cn or bias.numel() != Cn:
            raise RuntimeError("gps_gaussian_amd: group_norm: %d channels, %d groups, %d weights, %d biases" % (Cn, G, weight.numel(), bias.numel()))
        dev = x.device
        xc = _aligned(x.detach())
        w = weight.detach().to(device=dev, dtype=torch.float32).contiguous()
        b = bias.detach().to(device=dev, dtype=torch.float32).contiguous()
        HW = xc.numel() // (N * Cn) if N * Cn else 0
        y = torch.empty(x.shape, dtype=torch.float32, device=dev)
        mean = torch.empty((N, G), dtype=torch.float32, device=dev)
        rstd = torch.empty((N, G), dtype=torch.float32, device=dev)
        scratch = torch.empty((lib.gn_scratch_bytes(N, Cn, G, HW) // 4 + 4,), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = lib.gn_forward(_ptr(xc), _DTYPES[x.dtype], _ptr(w), _ptr(b), N, Cn, G, HW, float(eps), _ptr(y), _ptr(mean), _ptr(rstd), _ptr(scratch),
                                C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        _capi.check(rc, "gn_forward")
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(xc, mean, rstd, w)   # never y: the reference applies an in-place ReLU to it
            ctx.dims = (N, Cn, G, HW, x.shape, weight.dtype, bias.dtype)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        lib = _capi.lib()
        xc, mean, rstd, w = ctx.saved_tensors
        N, Cn, G, HW, shape, wdt, bdt = ctx.dims
        dev = xc.device
        need_x, _, need_w, need_b, _ = ctx.needs_input_grad
        dyc = _aligned(dy.to(torch.float32))
        dx = torch.empty_like(xc) if need_x else None
        dgamma = torch.empty((Cn,), dtype=torch.float32, device=dev) if need_w or need_b else None
        dbeta = torch.empty((Cn,), dtype=torch.float32, device=dev) if need_w or need_b else None
        scratch = torch.empty((lib.gn_scratch_bytes(N, Cn, G, HW) // 4 + 4,), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = lib.gn_backward(_ptr(xc), _DTYPES[xc.dtype], _ptr(dyc), _ptr(w), _ptr(mean), _ptr(rstd), N, Cn, G, HW, _ptr(dx), _ptr(dgamma), _ptr(dbeta),
                                 _ptr(scratch), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        _capi.check(rc, "gn_backward")
        if dgamma is not None and N * Cn * HW == 0:
            dgamma.zero_(), dbeta.zero_()
        return (dx.view(shape) if need_x else None, None, dgamma.to(wdt) if need_w else None, dbeta.to(bdt) if need_b else None, None)


def group_norm(x, num_groups, weight, bias, eps=1e-5):
    """torch.nn.functional.group_norm(x, num_groups, weight, bias, eps) for a GPU tensor x [N, C, *] in fp32 or fp16; the result is fp32 (what
    autocast's fp32 policy for group_norm gives for an fp16 input), x.grad comes back in x's dtype.  The backward reads x, not the output, so the
    output may be modified in place."""
    return _GroupNorm.apply(x, num_groups, weight, bias, eps)


def _autocast_dtype():
    get = getattr(torch, "get_autocast_dtype", None)      # newer torch; the older accessor warns there
    return get("cuda") if get is not None else torch.get_autocast_gpu_dtype()


def _fusable(m, x):
    if not (x.is_cuda and m.affine and x.dim() >= 3 and x.numel() > 0):
        return False
    if m.weight.dtype != torch.float32 or m.bias.dtype != torch.float32 or not m.weight.is_cuda:
        return False
    if x.dtype == torch.float16:
        if not (torch.is_autocast_enabled() and _autocast_dtype() == torch.float16):
            return False   # ATen would return fp16 here
    elif x.dtype != torch.float32:
        return False
    if not x.is_contiguous():
        cl = torch.channels_last if x.dim() == 4 else torch.channels_last_3d if x.dim() == 5 else None
        if cl is not None and x.is_contiguous(memory_format=cl):
            return False   # ATen keeps the channels-last layout of its input; the fused op would silently change it
    return True


class FusedGroupNorm(nn.GroupNorm):
    """nn.GroupNorm whose forward runs the fused op for: a GPU tensor of at least 3 dims, affine=True, fp32 -- or fp16 while fp16 autocast is
    active (fp32 out, as autocast gives; the cast kernel in front disappears).  Everything else (CPU, affine=False, channels-last, fp16 outside
    autocast, bf16, empty) is nn.GroupNorm.forward, counted in accelerate.calls["groupnorm_passthrough"].  Same parameters, same state_dict."""

    def forward(self, input):
        if not _fusable(self, input):
            accelerate.calls["groupnorm_passthrough"] += 1
            return nn.GroupNorm.forward(self, input)
        accelerate.calls["groupnorm"] += 1
        return _GroupNorm.apply(input, self.num_groups, self.weight, self.bias, self.eps)


def convert(module):
    """Make every nn.GroupNorm in `module`'s tree (the module itself included) a FusedGroupNorm, in place: the instance keeps its parameters, buffers,
    hooks and state_dict keys, only its class changes.  A module reachable through two parents is converted once; already converted modules and
    subclasses of nn.GroupNorm are left alone.  Returns the number converted."""
    n = 0
    for m in module.modules():
        if type(m) is nn.GroupNorm:
            m.__class__ = FusedGroupNorm
            n += 1
    return n
