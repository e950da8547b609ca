"""The stride-1 3x3 convolutions of a residual block -- `conv1` and `conv2` = Conv2d(C_in, C_out, 3, padding=1) with a bias -- forward and backward,
on the fp32 matrix-core kernels of csrc/resconv.hip (rc_forward / rc_backward of include/gpsgs.h).

The reference's ResidualBlock (core/extractor.py:10-11) holds two 3x3 convolutions as plain attributes; in stage 2 the depth encoder and the
regresser's three decoders run 22 stride-1 ones per stereo pair in fp32, at (C_in, C_out) = (32,32), (48,48), (64,64), (96,96), (128,48), (192,64)
and (192,96).  The kernels are implicit GEMMs on v_mfma_f32_32x32x2_f32 over contiguous NCHW: exact fp32 (every sum an fmaf chain in a fixed
order, the same bits on every run), no layout transposes (DESIGN.md "Residual-block 3x3 convolutions").

  conv3x3(x, weight, bias)       the op (autograd); GPU tensors only, like every other op of this package
  FusedResConv3x3                nn.Conv2d whose forward runs that op; what the op does not take, or loses on, goes to nn.Conv2d.forward
  convert(model)                 conv1 / conv2 of every module of a tree that has the members conv1, norm1, conv2, norm2 -> FusedResConv3x3
  supported(C_in, C_out), tile() what the kernels implement, and the forward's output tile
  calls                          {"resconv": calls that ran fused, "resconv_passthrough": calls that went to nn.Conv2d.forward}

There is no GPSGS_ACCELERATE name for this op: it is reached through convert(model) in the caller's own script."""
import functools

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _capi, _ops
from ._ops import aligned16, call, conv_inputs, dense_fp32_call, grad_buffers, param_grads, plain_conv, ptr

calls = {"resconv": 0, "resconv_passthrough": 0}
MEMBERS = ("conv1", "norm1", "conv2", "norm2")


def supported(C_in, C_out):
    """(C_in, C_out) is one the kernels implement (rc_supported): C_in a multiple of 4 in [4, 192], C_out a multiple of 16 in [16, 96]."""
    return bool(_capi.lib().rc_supported(int(C_in), int(C_out)))


def tile():
    """(rows, columns) of the output tile of a workgroup of the forward (rc_tile)."""
    return _ops.tile("rc_tile")


class _ResConv3x3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        xc, w, b = conv_inputs("resconv.conv3x3", "[N, C_in, H, W]", "[C_out, C_in, 3, 3]", x, weight, bias)
        N, Ci, H, W = x.shape
        Co = weight.shape[0]
        if tuple(weight.shape[1:]) != (Ci, 3, 3) or bias.numel() != Co or x.numel() == 0 or not supported(Ci, Co):
            raise RuntimeError("gps_gaussian_amd: resconv.conv3x3: unsupported configuration: input %s, weight %s" % (tuple(x.shape), tuple(weight.shape)))
        dev = x.device
        y = torch.empty((N, Co, H, W), dtype=torch.float32, device=dev)
        call("rc_forward", dev, ptr(xc), ptr(w), ptr(b), N, Ci, Co, H, W, ptr(y))
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(xc, w)
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
        dx, dw, db, scratch = grad_buffers(xc, needs, w.shape, _capi.lib().rc_scratch_bytes, N, Ci, Co, H, W)   # dx None: that kernel is not run
        call("rc_backward", xc.device, ptr(xc), ptr(w), ptr(dyc), N, Ci, Co, H, W, ptr(dx), ptr(dw), ptr(db), ptr(scratch))
        return (dx,) + param_grads(needs, dw, db, *ctx.like)


def conv3x3(x, weight, bias):
    """torch.nn.functional.conv2d(x, weight, bias, stride=1, padding=1) for an fp32 GPU tensor x [N, C_in, H, W], a weight [C_out, C_in, 3, 3] and a
    bias [C_out] with supported(C_in, C_out); anything else is a RuntimeError.  Exact fp32 arithmetic in a fixed order.  Gradients come back in the
    parameters' dtypes and shapes, x.grad in fp32; the input gradient is computed only if x requires grad, the parameter gradients only if either
    parameter does."""
    return _ResConv3x3.apply(x, weight, bias)


def _plain(conv):
    """A convolution whose static configuration is the op's: 3x3, stride 1, padding 1, otherwise plain_conv's, supported channel counts."""
    return plain_conv(conv, 3, 1, supported)


@functools.lru_cache(maxsize=None)
def _compute_units(index):
    return torch.cuda.get_device_properties(index).multi_processor_count


def keeps(N, C_in, C_out, H, W, graph, compute_units):
    """The measured routing rule (the class docstring), on what a call can see: True where the fused op keeps a supported call of these sizes,
    `graph` telling whether autograd records it (forward + backward) or not (forward alone)."""
    if not graph:
        return H * W >= 512 * 512
    th, tw = tile()
    workgroups = N * -(-H // th) * -(-W // tw) * -(-C_out // 32)          # of the forward
    return C_in <= C_out and C_out % 32 == 0 and workgroups >= 4 * compute_units


def _routed(m, x):
    graph = torch.is_grad_enabled() and (x.requires_grad or m.weight.requires_grad or m.bias.requires_grad)
    return keeps(x.shape[0], m.in_channels, m.out_channels, x.shape[2], x.shape[3], graph, _compute_units(x.device.index))


def _fusable(m, x):
    if not dense_fp32_call(m, x) or torch.is_autocast_enabled():
        return False                                      # ... inside autocast ATen decides the dtypes (the image encoder under mixed_precision)
    if x.shape[1] != m.in_channels or not _plain(m):
        return False
    return _routed(m, x)


class FusedResConv3x3(nn.Conv2d):
    """nn.Conv2d(C_in, C_out, 3, padding=1) whose forward is the fused op.  It runs for a contiguous 4-D fp32 GPU tensor with elements in it, fp32
    parameters on the same device, no autocast and a plain supported configuration: 3x3, stride 1, padding 1, dilation 1, groups 1, zero padding
    mode, a bias, C_in a multiple of 4 up to 192, C_out a multiple of 16 up to 96 -- and where the measured rule keeps the call (keeps()):

      * a call that records an autograd graph (forward + backward): C_in <= C_out, C_out a multiple of 32, and at least four forward workgroups
        (tile() outputs of one sample x 32 output channels) per compute unit of the device;
      * a forward alone: a plane of at least 512 x 512 pixels.

    Everything else is nn.Conv2d.forward, counted in calls["resconv_passthrough"].  Same parameters, same state_dict.

    The rows behind the rule (profiles/resconv_shapes.md, one MI355X with 256 compute units, ATen in fresh processes under both MIOpen find modes;
    a row wins where the fused upper quartile is below ATen's lower quartile under both).  Forward + backward, fused against ATen's faster median:
    [2,32,512,512] -> 32 421 against 611 us (1.45x, 1024 workgroups) and at N = 8 1345 against 1784 us; [8,64,256,256] -> 64 1301 against 1401 us
    (2048 workgroups) -- kept.  [2,64,256,256] -> 64 (512 workgroups) 362 against 363 us, [2,96,128,128] -> 96 (192) 281 against 215 us: too few
    workgroups ([8,96,128,128] -> 96, 768 workgroups, won by 2 % and is routed away with them).  C_in > C_out lost every row: [2,128,512,512] -> 48
    2275 against 2209 us, [2,192,256,256] -> 64 985 against 892 us, [2,192,128,128] -> 96 475 against 369 us, and at N = 8 0.91x, 0.98x, 0.98x.
    C_out = 48, whose second block of output channels is half empty: 1098 against 1152 us at [2,48,512,512] and 1108 against 1142 us at
    [8,48,256,256], but 302 against 299 us at [2,48,256,256] and 4212 against 3835 us (0.91x) at [8,48,512,512]: no rule on what a call sees
    separates these, so the class is ATen's.  Forward alone: all six rows at 512 x 512 won (1.01-1.20x); at 256 x 256 two of six, at 128 x 128 the
    N = 8 rows won and the N = 2 rows lost by 0.67-0.74x (192 workgroups on 256 compute units)."""

    def forward(self, input):
        if _fusable(self, input):
            calls["resconv"] += 1
            return _ResConv3x3.apply(input, self.weight, self.bias)
        calls["resconv_passthrough"] += 1
        return nn.Conv2d.forward(self, input)


def is_block(m):
    """A duck-typed residual block: a module, not an nn.Sequential, that holds conv1, norm1, conv2 and norm2 as submodules."""
    return not isinstance(m, nn.Sequential) and all(isinstance(getattr(m, name, None), nn.Module) for name in MEMBERS)


def convert(model):
    """On every module of `model`'s tree (the model itself included) that has the members conv1, norm1, conv2 and norm2 -- the reference's
    ResidualBlock, recognised by what it holds -- `conv1` and `conv2` become a FusedResConv3x3 where they are exactly a plain supported stride-1
    3x3 nn.Conv2d (see FusedResConv3x3), in place: the instance keeps its parameters, hooks and state_dict key, only its class changes.  The
    stride-2 `conv1` of res2[0] and res3[0], subclasses of nn.Conv2d, already converted layers and every convolution inside an nn.Sequential
    (the shortcut's 1x1, the heads) are left alone, so this composes with the other conversions of this package in any order; the block's forward
    -- the reference's own or groupnorm.residual_block_forward -- reaches the layers through block.conv1(x) and block.conv2(y).  Idempotent;
    returns the number converted."""
    n = 0
    for m in model.modules():
        if is_block(m):
            for name in ("conv1", "conv2"):
                conv = getattr(m, name)
                if type(conv) is nn.Conv2d and _plain(conv):
                    conv.__class__ = FusedResConv3x3
                    n += 1
    return n
