"""GroupNorm, forward and backward, on the HIP kernels of csrc/group_norm.hip (gn_forward / gn_backward of include/gpsgs.h).

ATen normalises one (sample, group) row per workgroup; the reference's feature extractor builds `GroupNorm(planes // 8, planes)`, 8..24 rows of up
to two million elements, so most of the chip idles while a handful of CUs stream.  The kernels here cut every row into chunks of
`_capi.lib().gn_chunk_elems()` elements, one workgroup each (DESIGN.md "GroupNorm").

  group_norm(x, num_groups, weight, bias, eps)   the op (autograd); GPU tensors only, like every other op of this package
      relu=True                                  ... with the ReLU that follows it in the same kernels (gne_forward / gne_backward)
      relu=True, residual=r                      ... and relu(r + .) on top: the tail of a residual block, one autograd node
  FusedGroupNorm                                 nn.GroupNorm with `forward` on that op; whatever the op does not take goes to nn.GroupNorm.forward
      .forward_relu(input, residual=None)        the two fused forms; otherwise relu_(nn.GroupNorm.forward(input)) and relu(residual + .)
  convert(module)                                turn every nn.GroupNorm of a module tree into a FusedGroupNorm, in place
  residual_block_forward(block, x)               the forward of a conv1 / norm1 / conv2 / norm2 / downsample block on forward_relu
  fuse_sequential_relu(module)                   GroupNorm directly followed by nn.ReLU in an nn.Sequential -> one FusedGroupNormReLU + nn.Identity

`GPSGS_ACCELERATE=groupnorm` makes the reference's extractor classes call convert() on themselves, `GPSGS_ACCELERATE=resblock` also rebinds the
residual block's forward and fuses the stem's ReLU (accelerate.py)."""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _capi, accelerate
from ._ops import DTYPE_CODE, aligned16, autocast_dtype, call, fp32_on, ptr, sequential_slots, swap_class


class _GroupNorm(torch.autograd.Function):
    """group_norm(x); with relu, relu(group_norm(x)) or, with a residual too, relu(residual + relu(group_norm(x))): one node each.  Saved for the
    backward: x, mean, rstd, weight -- never y: the reference applies an in-place ReLU to it; with relu also the bias (the sign of the normalised
    value is recomputed from them, not read from the output) and, in the residual form only, the output (its sign masks the incoming gradient; the
    layer that consumes the output keeps it alive anyway)."""

    @staticmethod
    def forward(ctx, x, num_groups, weight, bias, eps, relu, residual):
        lib = _capi.lib()
        if not x.is_cuda:
            raise RuntimeError("gps_gaussian_amd: group_norm input must live on a GPU (no CPU fallback)")
        if x.dtype not in DTYPE_CODE:
            raise RuntimeError("gps_gaussian_amd: group_norm takes fp32 or fp16 input, not %s" % x.dtype)
        if x.dim() < 2 or weight is None or bias is None:
            raise RuntimeError("gps_gaussian_amd: group_norm needs an [N, C, ...] input, a weight and a bias")
        N, Cn, G = x.shape[0], x.shape[1], int(num_groups)
        if G <= 0 or Cn % G != 0 or weight.numel() != Cn or bias.numel() != Cn:
            raise RuntimeError("gps_gaussian_amd: group_norm: %d channels, %d groups, %d weights, %d biases" % (Cn, G, weight.numel(), bias.numel()))
        dev = x.device
        if residual is not None and not (torch.is_tensor(residual) and residual.is_cuda and residual.device == dev
                                         and residual.dtype == torch.float32 and residual.shape == x.shape):
            raise RuntimeError("gps_gaussian_amd: group_norm: residual must be an fp32 GPU tensor of the input's shape %s" % (tuple(x.shape),))
        xc = aligned16(x.detach())
        res = aligned16(residual.detach()) if residual is not None else None
        w, b = fp32_on(dev, weight, bias)
        HW = xc.numel() // (N * Cn) if N * Cn else 0
        out = torch.empty(x.shape, dtype=torch.float32, device=dev)
        mean = torch.empty((N, G), dtype=torch.float32, device=dev)
        rstd = torch.empty((N, G), dtype=torch.float32, device=dev)
        scratch = torch.empty((lib.gn_scratch_bytes(N, Cn, G, HW) // 4 + 4,), dtype=torch.float32, device=dev)
        head = (ptr(xc), DTYPE_CODE[x.dtype], ptr(w), ptr(b))
        tail = (N, Cn, G, HW, float(eps), ptr(out), ptr(mean), ptr(rstd), ptr(scratch))
        if relu:
            call("gne_forward", dev, *head, ptr(res), *tail)
        else:
            call("gn_forward", dev, *head, *tail)   # the plain op keeps its own entry point and kernels
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(xc, mean, rstd, w, *((b,) if relu else ()), *((out,) if residual is not None else ()))
            ctx.dims = (N, Cn, G, HW, x.shape, weight.dtype, bias.dtype, relu)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        lib = _capi.lib()
        N, Cn, G, HW, shape, wdt, bdt, relu = ctx.dims
        saved = ctx.saved_tensors
        xc, mean, rstd, w = saved[:4]
        out = saved[5] if len(saved) > 5 else None
        dev = xc.device
        need_x, _, need_w, need_b, _, _, need_r = ctx.needs_input_grad
        need_r = need_r and out is not None
        dc = aligned16(dout.to(torch.float32))
        dx = torch.empty_like(xc) if need_x else None
        dres = torch.empty(shape, dtype=torch.float32, device=dev) if need_r else None
        dgamma = torch.empty((Cn,), dtype=torch.float32, device=dev) if need_w or need_b else None
        dbeta = torch.empty((Cn,), dtype=torch.float32, device=dev) if need_w or need_b else None
        scratch = torch.empty((lib.gn_scratch_bytes(N, Cn, G, HW) // 4 + 4,), dtype=torch.float32, device=dev)
        head = (ptr(xc), DTYPE_CODE[xc.dtype], ptr(dc))
        stats = (ptr(mean), ptr(rstd), N, Cn, G, HW, ptr(dx))
        tail = (ptr(dgamma), ptr(dbeta), ptr(scratch))
        if relu:
            call("gne_backward", dev, *head, ptr(out), ptr(w), ptr(saved[4]), *stats, ptr(dres), *tail)
        else:
            call("gn_backward", dev, *head, ptr(w), *stats, *tail)
        if dgamma is not None and N * Cn * HW == 0:
            dgamma.zero_(), dbeta.zero_()
        return (dx.view(shape) if need_x else None, None, dgamma.to(wdt) if need_w else None, dbeta.to(bdt) if need_b else None, None, None, dres)


def group_norm(x, num_groups, weight, bias, eps=1e-5, *, relu=False, residual=None):
    """torch.nn.functional.group_norm(x, num_groups, weight, bias, eps) for a GPU tensor x [N, C, *] in fp32 or fp16; the result is fp32 (what
    autocast's fp32 policy for group_norm gives for an fp16 input), x.grad comes back in x's dtype.  The backward reads x, not the output, so the
    output may be modified in place.

    relu=True returns relu(y) instead, and relu=True with residual=r (an fp32 GPU tensor of x's shape) returns relu(r + relu(y)), each from the same
    two kernels and as ONE autograd node, with the bits of `relu_` / `+` / `relu` applied to the plain result; gradients flow to x, weight, bias
    and r.  A residual without relu=True, or one of another device, dtype or shape, is a RuntimeError."""
    if residual is not None and not relu:
        raise RuntimeError("gps_gaussian_amd: group_norm: residual= needs relu=True (the fused form is relu(residual + relu(y)))")
    return _GroupNorm.apply(x, num_groups, weight, bias, eps, bool(relu), residual)


def _fusable(m, x):
    if not (x.is_cuda and m.affine and x.dim() >= 3 and x.numel() > 0):
        return False
    if m.weight.dtype != torch.float32 or m.bias.dtype != torch.float32 or not m.weight.is_cuda:
        return False
    if x.dtype == torch.float16:
        if not (torch.is_autocast_enabled() and autocast_dtype() == torch.float16):
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
        return _GroupNorm.apply(input, self.num_groups, self.weight, self.bias, self.eps, False, None)

    def forward_relu(self, input, residual=None):
        """relu_(self(input)), and with a residual relu(residual + that): in the fused kernels where forward() would use them, otherwise with
        exactly those ops on nn.GroupNorm.forward (the reference's own: same bits), counted as a pass-through."""
        if not _fusable(self, input):
            accelerate.calls["groupnorm_passthrough"] += 1
            y = torch.relu_(nn.GroupNorm.forward(self, input))
            return y if residual is None else torch.relu(residual + y)
        accelerate.calls["groupnorm"] += 1
        if residual is None:
            return _GroupNorm.apply(input, self.num_groups, self.weight, self.bias, self.eps, True, None)
        if not (residual.is_cuda and residual.device == input.device and residual.dtype == torch.float32 and residual.shape == input.shape):
            return torch.relu(residual + _GroupNorm.apply(input, self.num_groups, self.weight, self.bias, self.eps, True, None))   # broadcast, fp64, ...
        return _GroupNorm.apply(input, self.num_groups, self.weight, self.bias, self.eps, True, residual)


class FusedGroupNormReLU(FusedGroupNorm):
    """A FusedGroupNorm that applies the ReLU which followed it in its nn.Sequential (fuse_sequential_relu put an nn.Identity there)."""

    def forward(self, input):
        return self.forward_relu(input)


def convert(module):
    """Make every nn.GroupNorm in `module`'s tree (the module itself included) a FusedGroupNorm, in place: the instance keeps its parameters, buffers,
    hooks and state_dict keys, only its class changes.  A module reachable through two parents is converted once; already converted modules and
    subclasses of nn.GroupNorm are left alone.  Returns the number converted."""
    return swap_class(module, nn.GroupNorm, FusedGroupNorm)


def fuse_sequential_relu(module):
    """In every nn.Sequential of `module`'s tree (the module itself included): a GroupNorm (plain or FusedGroupNorm) DIRECTLY followed by an nn.ReLU
    becomes a FusedGroupNormReLU and the ReLU's slot an nn.Identity -- same indices, same state_dict keys, same parameters.  A norm that sits in more
    than one place of the tree is left alone (its other users do not want the ReLU).  Idempotent; returns the number fused."""
    uses = {}
    for m in module.modules():
        for c in m.children():
            uses[id(c)] = uses.get(id(c), 0) + 1
    n = 0
    for seq, i in sequential_slots(module):
        if type(seq[i]) in (nn.GroupNorm, FusedGroupNorm) and type(seq[i + 1]) is nn.ReLU and uses.get(id(seq[i]), 0) == 1:
            seq[i].__class__ = FusedGroupNormReLU
            seq[i + 1] = nn.Identity()
            n += 1
    return n


def _own_forward(block):
    """The forward the block's class defines -- the reference's own where accelerate has rebound it to residual_block_forward."""
    return accelerate.original(block, "forward") or type(block).forward


def _norm_relu(norm, y, residual=None):
    if isinstance(norm, FusedGroupNorm):
        return norm.forward_relu(y, residual)
    y = torch.relu_(norm(y))
    return y if residual is None else torch.relu(residual + y)


def residual_block_forward(block, x):
    """The forward of a residual block with the members conv1, norm1, conv2, norm2, downsample (None or a module):
        y = relu_(norm1(conv1(x)));  y = relu_(norm2(conv2(y)));  relu(downsample(x) + y)
    with each norm + ReLU, and the add + ReLU behind the second, in one fused op (FusedGroupNorm.forward_relu).  Blocks whose norm1 / norm2 are not
    GroupNorm layers (batch, instance, none) run their class's own forward.  Counted in accelerate.calls["resblock"] / ["resblock_passthrough"]."""
    n1, n2 = getattr(block, "norm1", None), getattr(block, "norm2", None)
    if not (isinstance(n1, nn.GroupNorm) and isinstance(n2, nn.GroupNorm)):
        accelerate.calls["resblock_passthrough"] += 1
        return _own_forward(block)(block, x)
    accelerate.calls["resblock"] += 1
    y = _norm_relu(n1, block.conv1(x))
    y = block.conv2(y)
    r = x if block.downsample is None else block.downsample(x)
    return _norm_relu(n2, y, r)
