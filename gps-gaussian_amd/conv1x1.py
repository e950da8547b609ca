"""The 1x1 convolution that opens the shortcut of a residual block -- Conv2d(C_in, C_out, 1, stride 1 | 2) with a bias -- forward and backward, on
the fp32 matrix-core kernels of csrc/conv1x1.hip (c1_forward / c1_backward of include/gpsgs.h).

The reference's ResidualBlock (core/extractor.py:43-45) builds `downsample = Sequential(Conv2d(in_planes, planes, 1, stride), norm3)` whenever its
input and output differ: res2[0] and res3[0] of every UnetExtractor (stride 2), the first block of each of the regresser's three decoders (stride
1), and res1[0] with the default widths.  Over contiguous NCHW a 1x1 convolution is one GEMM per image with the pixel axis contiguous on both
sides; the kernels run it on v_mfma_f32_32x32x2_f32 as it lies: exact fp32 (every sum an fmaf chain in a fixed order, the same bits on every run),
no layout transposes, no intermediate tensor (DESIGN.md "Residual-shortcut 1x1 convolutions").

  conv1x1(x, weight, bias, stride=1)      the op (autograd); GPU tensors only, like every other op of this package
  FusedConv1x1                            nn.Conv2d whose forward runs that op; what the op does not take goes to nn.Conv2d.forward
  convert(module)                         a plain supported 1x1 nn.Conv2d inside any nn.Sequential of a module tree -> FusedConv1x1
  supported(C_in, C_out, stride), tile()  what the kernels implement, and their tile sizes

`GPSGS_ACCELERATE=conv1x1` makes the reference's ResidualBlock and UnetExtractor call convert() on themselves (accelerate.py)."""
import ctypes
import functools

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _capi, accelerate
from ._ops import aligned16, call, conv_inputs, dense_fp32_call, grad_buffers, param_grads, plain_conv, ptr, sequential_slots


def supported(C_in, C_out, stride=1):
    """(C_in, C_out, stride) is one the kernels implement (c1_supported): C_in a multiple of 4 in [4, 256], C_out a multiple of 16 in [16, 128],
    stride 1 or 2."""
    return bool(_capi.lib().c1_supported(int(C_in), int(C_out), int(stride)))


@functools.lru_cache(maxsize=None)
def tile():
    """(the consecutive output pixels of a workgroup of the forward, the pixels of a tile of the weight gradient, the largest number of partial sums
    the weight gradient writes) as c1_tile reports them."""
    a, b, c = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _capi.check(_capi.lib().c1_tile(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "c1_tile")
    return a.value, b.value, c.value


class _Conv1x1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride):
        xc, w, b = conv_inputs("conv1x1", "[N, C_in, H, W]", "[C_out, C_in, 1, 1]", x, weight, bias)
        N, Ci, H, W = x.shape
        Co, stride = weight.shape[0], int(stride)
        if tuple(weight.shape[1:]) != (Ci, 1, 1) or bias.numel() != Co or x.numel() == 0 or not supported(Ci, Co, stride):
            raise RuntimeError("gps_gaussian_amd: conv1x1: unsupported configuration: input %s, weight %s, stride %s"
                               % (tuple(x.shape), tuple(weight.shape), stride))
        dev = x.device
        y = torch.empty((N, Co, (H - 1) // stride + 1, (W - 1) // stride + 1), dtype=torch.float32, device=dev)
        call("c1_forward", dev, ptr(xc), ptr(w), ptr(b), N, Ci, Co, H, W, stride, ptr(y))
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(xc, w)
            ctx.stride = stride
            ctx.like = (weight.dtype, bias.dtype)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        xc, w = ctx.saved_tensors
        N, Ci, H, W = xc.shape
        Co = w.shape[0]
        needs = ctx.needs_input_grad
        dyc = aligned16(dy.to(torch.float32))
        # dx None: that kernel is not run; where it runs it writes every element of dx, so torch.empty_like is enough
        dx, dw, db, scratch = grad_buffers(xc, needs, w.shape, _capi.lib().c1_scratch_bytes, N, Ci, Co, H, W, ctx.stride)
        call("c1_backward", xc.device, ptr(xc), ptr(w), ptr(dyc), N, Ci, Co, H, W, ctx.stride, ptr(dx), ptr(dw), ptr(db), ptr(scratch))
        return (dx,) + param_grads(needs, dw, db, *ctx.like) + (None,)


def conv1x1(x, weight, bias, stride=1):
    """torch.nn.functional.conv2d(x, weight, bias, stride=stride) for an fp32 GPU tensor x [N, C_in, H, W], a weight [C_out, C_in, 1, 1] and a bias
    [C_out] with supported(C_in, C_out, stride); anything else is a RuntimeError.  Exact fp32 arithmetic in a fixed order.  Gradients come back in
    the parameters' dtypes and shapes, x.grad in fp32 (for stride 2: +0.0 wherever the forward did not sample); the input gradient is computed only
    if x requires grad, the parameter gradients only if either parameter does."""
    return _Conv1x1.apply(x, weight, bias, stride)


def _plain(conv):
    """A convolution whose static configuration is the op's: 1x1, stride (1, 1) or (2, 2), padding 0, otherwise plain_conv's, supported channel
    counts."""
    return plain_conv(conv, 1, 0, lambda ci, co: supported(ci, co, conv.stride[0]), strides=((1, 1), (2, 2)))


@functools.lru_cache(maxsize=None)
def _compute_units(index):
    return torch.cuda.get_device_properties(index).multi_processor_count


def _fusable(m, x):
    if not dense_fp32_call(m, x) or torch.is_autocast_enabled():
        return False                                      # ... inside autocast ATen decides the dtypes (the image encoder under mixed_precision)
    if x.shape[1] != m.in_channels or not _plain(m):
        return False
    if m.stride == (1, 1):
        # the one measured layer that lost (profiles/conv1x1_shapes.md): decoder3[0], [2,192,128,128] -> 96 -- 128 workgroups of the forward on 256
        # compute units, against a plain GEMM of the BLAS library: 41 against 31 us forward, 107 against 107 us forward + backward.  With a stride
        # of 2 ATen has no plain GEMM to call and lost at the same workgroup count (res3[0], 1.6x), so the rule is for stride 1 alone.
        workgroups = x.shape[0] * -(-(x.shape[2] * x.shape[3]) // tile()[0])
        return workgroups >= _compute_units(x.device.index)
    return True


class FusedConv1x1(nn.Conv2d):
    """nn.Conv2d(C_in, C_out, 1, stride 1 | 2) whose forward is the fused op.  It runs for a contiguous 4-D fp32 GPU tensor with elements in it,
    fp32 parameters on the same device, no autocast and a plain supported configuration: 1x1, stride (1, 1) or (2, 2), padding 0, dilation 1,
    groups 1, zero padding mode, a bias, C_in a multiple of 4 up to 256, C_out a multiple of 16 up to 128 -- and, at stride 1, an input that gives
    the forward at least one workgroup (tile()[0] output pixels of one image) per compute unit of the device: the one measured row that lost to
    ATen, GSRegresser.decoder3[0] on one stereo pair, [2,192,128,128] -> 96, is 128 workgroups on 256 compute units (forward 0.75x, forward +
    backward 1.00x ATen, which runs a plain GEMM there; profiles/conv1x1_shapes.md).  Everything else is nn.Conv2d.forward, counted in
    accelerate.calls["conv1x1_passthrough"].  Same parameters, same state_dict."""

    def forward(self, input):
        counts = accelerate.counters("conv1x1")
        if _fusable(self, input):
            counts["conv1x1"] += 1
            return _Conv1x1.apply(input, self.weight, self.bias, self.stride[0])
        counts["conv1x1_passthrough"] += 1
        return nn.Conv2d.forward(self, input)


def convert(module):
    """In every nn.Sequential of `module`'s tree (the module itself included), every plain supported 1x1 nn.Conv2d (see FusedConv1x1) becomes a
    FusedConv1x1, in place: the instance keeps its parameters, hooks and state_dict key, only its class changes -- `downsample[0]` of the
    reference's ResidualBlock.  Convolutions held as plain attributes, subclasses of nn.Conv2d (gshead's FusedHeadConv among them) and already
    converted layers are left alone.  Returns the number converted."""
    n = 0
    for seq, i in sequential_slots(module, 1):
        if type(seq[i]) is nn.Conv2d and _plain(seq[i]):
            seq[i].__class__ = FusedConv1x1
            n += 1
    return n
