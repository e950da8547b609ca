"""The stem convolutions -- Conv2d(1 | 3, C_out, 5, stride 2, padding 2) -- forward and backward, on the HIP kernels of csrc/stem_conv.hip
(sc_forward / sc_backward of include/gpsgs.h).

The reference's two encoders open with `Conv2d(C_in, 32, 5, stride=2, padding=2)` on the full-resolution image (C_in = 3) and depth map (C_in = 1).
With so few input channels the library's implicit-GEMM kernels run a K step of 4 and transpose to NHWC and back; the kernels here convolve
directly in NCHW with the input patch of an output tile in LDS and wave-uniform weights (DESIGN.md "Stem convolution").

  conv2d(x, weight, bias, stride, padding)   the op (autograd); GPU tensors only, like every other op of this package
      out_dtype=torch.float16                ... with the result rounded once to fp16 on store (what fp16 autocast returns for this layer)
  FusedStemConv2d                            nn.Conv2d with `forward` on that op; whatever the op does not take goes to nn.Conv2d.forward
  convert(module)                            turn every supported nn.Conv2d of a module tree into a FusedStemConv2d, in place

`GPSGS_ACCELERATE=stemconv` makes the reference's UnetExtractor call convert() on itself (accelerate.py)."""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _capi, accelerate
from ._ops import DTYPE_CODE, aligned16, autocast_dtype, call, conv_inputs, dense_fp32_call, grad_buffers, param_grads, ptr, swap_class


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def supported(C_in, C_out, kernel_size, stride, padding, dilation=1, groups=1):
    """The static configuration of a layer is one the kernels implement (sc_supported, plus square / dilation 1 / groups 1)."""
    k, s, p, d = _pair(kernel_size), _pair(stride), _pair(padding), _pair(dilation)
    if isinstance(padding, str) or k[0] != k[1] or s[0] != s[1] or p[0] != p[1] or d != (1, 1) or groups != 1:
        return False
    return bool(_capi.lib().sc_supported(int(C_in), int(C_out), int(k[0]), int(s[0]), int(p[0])))


class _StemConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, out_dtype):
        xc, w, b = conv_inputs("conv2d", "[N, C_in, H, W]", "[C_out, C_in, K, K]", x, weight, bias)
        if out_dtype not in DTYPE_CODE:
            raise RuntimeError("gps_gaussian_amd: conv2d returns fp32 or fp16, not %s" % out_dtype)
        N, Ci, H, W = x.shape
        Co, Ci_w, K, K2 = weight.shape
        s, p = int(stride), int(padding)
        if Ci_w != Ci or K != K2 or bias.numel() != Co or not _capi.lib().sc_supported(Ci, Co, K, s, p):
            raise RuntimeError("gps_gaussian_amd: conv2d: unsupported configuration: input %s, weight %s, stride %d, padding %d"
                               % (tuple(x.shape), tuple(weight.shape), s, p))
        dev = x.device
        Ho, Wo = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
        y = torch.empty((N, Co, Ho, Wo), dtype=out_dtype, device=dev)
        call("sc_forward", dev, ptr(xc), ptr(w), ptr(b), N, Ci, Co, H, W, K, s, p, ptr(y), DTYPE_CODE[out_dtype])
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(xc, w)
            ctx.dims = (N, Ci, Co, H, W, K, s, p)
            ctx.like = (weight.dtype, bias.dtype)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        xc, w = ctx.saved_tensors
        N, Ci, Co, H, W, K, s, p = ctx.dims
        needs = ctx.needs_input_grad
        dyc = aligned16(dy if dy.dtype in DTYPE_CODE else dy.to(torch.float32))
        dx, dw, db, scratch = grad_buffers(xc, needs, w.shape, _capi.lib().sc_scratch_bytes, *ctx.dims)   # dx None: that kernel is not run
        call("sc_backward", xc.device, ptr(xc), ptr(w), ptr(dyc), DTYPE_CODE[dyc.dtype], N, Ci, Co, H, W, K, s, p, ptr(dx), ptr(dw), ptr(db),
             ptr(scratch))
        return (dx,) + param_grads(needs, dw, db, *ctx.like) + (None, None, None)


def conv2d(x, weight, bias, stride, padding, *, out_dtype=torch.float32):
    """torch.nn.functional.conv2d(x, weight, bias, stride, padding) for an fp32 GPU tensor x [N, C_in, H, W] and a configuration sc_supported takes
    (C_in 1 or 3, 5x5, stride 2, padding 2, C_out a multiple of 8 up to 64); anything else is a RuntimeError.  fp32 accumulation, one rounding to
    `out_dtype` (fp32 or fp16).  Gradients come back in the parameters' dtypes, x.grad in fp32; the input-gradient kernel is launched only if x
    requires grad."""
    return _StemConv.apply(x, weight, bias, stride, padding, out_dtype)


def _out_dtype(m, x):
    """The dtype the fused op returns for this call (ATen's), or None: the call is nn.Conv2d.forward's."""
    if not dense_fp32_call(m, x) or m.padding_mode != "zeros":
        return None
    if x.shape[1] != m.in_channels or not supported(m.in_channels, m.out_channels, m.kernel_size, m.stride, m.padding, m.dilation, m.groups):
        return None
    if torch.is_autocast_enabled():
        return torch.float16 if autocast_dtype() == torch.float16 else None   # conv2d is on autocast's lower-precision list; bf16 is ATen's
    return torch.float32


class FusedStemConv2d(nn.Conv2d):
    """nn.Conv2d whose forward runs the fused op for: a contiguous 4-D fp32 GPU tensor with elements in it, fp32 weights on the same device, a bias,
    zero padding and a configuration sc_supported takes.  The result has ATen's dtype: fp16 while fp16 autocast is active, otherwise fp32.
    Everything else (CPU, channels-last, fp16 / bf16 input, bf16 autocast, no bias, other configurations, empty) is nn.Conv2d.forward, counted in
    accelerate.calls["stemconv_passthrough"].  Same parameters, same state_dict."""

    def forward(self, input):
        dt = _out_dtype(self, input)
        if dt is None:
            accelerate.calls["stemconv_passthrough"] += 1
            return nn.Conv2d.forward(self, input)
        accelerate.calls["stemconv"] += 1
        return _StemConv.apply(input, self.weight, self.bias, _pair(self.stride)[0], _pair(self.padding)[0], dt)


def convert(module):
    """Make every nn.Conv2d in `module`'s tree (the module itself included) whose static configuration the kernels implement a FusedStemConv2d, in
    place: the instance keeps its parameters, hooks and state_dict keys, only its class changes.  Subclasses of nn.Conv2d, layers without a bias or
    with another padding mode, and already converted modules are left alone.  Returns the number converted."""
    return swap_class(module, nn.Conv2d, FusedStemConv2d, lambda m: m.bias is not None and m.padding_mode == "zeros" and supported(
        m.in_channels, m.out_channels, m.kernel_size, m.stride, m.padding, m.dilation, m.groups))
