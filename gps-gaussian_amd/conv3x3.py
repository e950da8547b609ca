"""The regresser's full-resolution 3x3 convolutions -- Conv2d(C_in, 32, 3, padding=1), optionally followed by ReLU -- forward and backward, on the
fp32 matrix-core kernels of csrc/conv3x3.hip (c3_forward / c3_backward of include/gpsgs.h).

The reference's GSRegresser (lib/gs_parm_network.py) runs `out_relu(out_conv(x))` with out_conv = Conv2d(52, 32, 3, padding=1) and opens each of its
three heads with Conv2d(32, 32, 3, padding=1), all on the full-resolution map and in fp32.  The kernels here are implicit GEMMs on
v_mfma_f32_32x32x2_f32 over contiguous NCHW: exact fp32 (every sum an fmaf chain in a fixed order, the same bits on every run), no layout
transposes (DESIGN.md "Full-resolution 3x3 convolutions").

  conv3x3(x, weight, bias, relu=False)    the op (autograd); GPU tensors only, like every other op of this package
  FusedConv3x3                            nn.Conv2d (with a `relu` attribute) whose forward runs that op; what the op does not take goes to
                                          nn.Conv2d.forward (+ torch.relu)
  convert(module)                         a plain supported 3x3 nn.Conv2d inside any nn.Sequential of a module tree -> FusedConv3x3(relu=False)
  fuse_relu(owner, conv_name, relu_name)  a conv and an nn.ReLU held as attributes and applied back to back -> FusedConv3x3(relu=True) + nn.Identity
  convert_regresser(net)                  fuse_relu(net, "out_conv", "out_relu") + convert(net)

`GPSGS_ACCELERATE=conv3x3` makes the reference's GSRegresser call convert_regresser() on itself (accelerate.py)."""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _capi, _ops, accelerate
from ._ops import aligned16, call, conv_inputs, dense_fp32_call, grad_buffers, param_grads, plain_conv, ptr, sequential_slots


def supported(C_in, C_out):
    """(C_in, C_out) is one the kernels implement (c3_supported): C_out 32, C_in a multiple of 4 in [4, 64]."""
    return bool(_capi.lib().c3_supported(int(C_in), int(C_out)))


class _Conv3x3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        xc, w, b = conv_inputs("conv3x3", "[N, C_in, H, W]", "[32, C_in, 3, 3]", x, weight, bias)
        N, Ci, H, W = x.shape
        Co = weight.shape[0]
        if tuple(weight.shape[1:]) != (Ci, 3, 3) or bias.numel() != Co or x.numel() == 0 or not supported(Ci, Co):
            raise RuntimeError("gps_gaussian_amd: conv3x3: unsupported configuration: input %s, weight %s" % (tuple(x.shape), tuple(weight.shape)))
        dev = x.device
        relu = bool(relu)
        y = torch.empty((N, Co, H, W), dtype=torch.float32, device=dev)
        call("c3_forward", dev, ptr(xc), ptr(w), ptr(b), N, Ci, H, W, int(relu), ptr(y))
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(xc, w, *((y,) if relu else ()))     # y only where its sign is the ReLU's mask
            ctx.relu = relu
            ctx.like = (weight.dtype, bias.dtype)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        xc, w = ctx.saved_tensors[:2]
        y = ctx.saved_tensors[2] if ctx.relu else None
        N, Ci, H, W = xc.shape
        needs = ctx.needs_input_grad
        dyc = aligned16(dy.to(torch.float32))
        dx, dw, db, scratch = grad_buffers(xc, needs, w.shape, _capi.lib().c3_scratch_bytes, N, Ci, H, W)   # dx None: that kernel is not run
        call("c3_backward", xc.device, ptr(xc), ptr(w), ptr(y), ptr(dyc), N, Ci, H, W, int(ctx.relu), ptr(dx), ptr(dw), ptr(db), ptr(scratch))
        return (dx,) + param_grads(needs, dw, db, *ctx.like) + (None,)


def conv3x3(x, weight, bias, relu=False):
    """torch.nn.functional.conv2d(x, weight, bias, stride=1, padding=1), then torch.relu where `relu`, for an fp32 GPU tensor x [N, C_in, H, W], a
    weight [32, C_in, 3, 3] with C_in a multiple of 4 in [4, 64] and a bias [32]; anything else is a RuntimeError.  Exact fp32 arithmetic in a fixed
    order.  Gradients come back in the parameters' dtypes and shapes, x.grad in fp32 (zero where the ReLU's output is); the input gradient is
    computed only if x requires grad, the parameter gradients only if either parameter does."""
    return _Conv3x3.apply(x, weight, bias, relu)


def _plain(conv):
    """A convolution whose static configuration is the op's: 3x3, padding 1, otherwise plain_conv's, supported channel counts."""
    return plain_conv(conv, 3, 1, supported)


def tile():
    """(rows, columns) of the output tile of a workgroup of the forward (c3_tile)."""
    return _ops.tile("c3_tile")


def _fusable(m, x):
    if not dense_fp32_call(m, x) or torch.is_autocast_enabled():
        return False                                      # ... the regresser runs outside autocast; inside it, ATen decides the dtypes
    if x.shape[1] != m.in_channels or not _plain(m):
        return False
    if torch.is_grad_enabled() and (x.requires_grad or m.weight.requires_grad or m.bias.requires_grad):
        return True                                       # forward + backward: every measured row wins (profiles/conv3x3_shapes.md)
    # a forward that records no graph: 1.16-1.24x ATen where the plane is whole tiles, but the one ragged plane measured ([2,52,511,771]: partly
    # empty edge tiles) lost to ATen's Winograd kernel by 1-3 %, so planes that are not whole tiles are ATen's
    th, tw = tile()
    return x.shape[2] % th == 0 and x.shape[3] % tw == 0


class FusedConv3x3(nn.Conv2d):
    """nn.Conv2d(C_in, 32, 3, padding=1) that computes conv(x), or relu(conv(x)) where its `relu` attribute is set (fuse_relu() leaves nn.Identity in
    the ReLU's place).  The fused op runs for a contiguous 4-D fp32 GPU tensor with elements in it, fp32 parameters on the same device, no autocast
    and a plain supported configuration: 3x3, stride 1, padding 1, dilation 1, groups 1, zero padding mode, a bias, C_out 32, C_in a multiple of 4
    up to 64 -- and, for a forward that records no autograd graph, a plane of whole tile() tiles (the one measured row that lost to ATen was such a
    forward of a ragged plane).  Everything else is nn.Conv2d.forward (then torch.relu where `relu`), counted in
    accelerate.calls["conv3x3_passthrough"].  Same parameters, same state_dict."""
    relu = False

    def forward(self, input):
        counts = accelerate.counters("conv3x3")
        if _fusable(self, input):
            counts["conv3x3"] += 1
            return _Conv3x3.apply(input, self.weight, self.bias, self.relu)
        counts["conv3x3_passthrough"] += 1
        y = nn.Conv2d.forward(self, input)
        return torch.relu(y) if self.relu else y

    def extra_repr(self):
        return "%s, relu=%s" % (nn.Conv2d.extra_repr(self), self.relu)


def _swap(conv, relu):
    conv.__class__ = FusedConv3x3
    conv.relu = relu


def convert(module):
    """In every nn.Sequential of `module`'s tree (the module itself included), every plain supported 3x3 nn.Conv2d (see FusedConv3x3) becomes a
    FusedConv3x3 with relu=False, in place: the instance keeps its parameters, hooks and state_dict key, only its class changes.  An nn.ReLU behind
    it stays where it is -- in the heads it belongs to gshead.convert(), which folds it into the 1x1 convolution that follows; the two conversions
    compose in either order.  Convolutions held as plain attributes, subclasses of nn.Conv2d and already converted layers are left alone.  Returns
    the number converted."""
    n = 0
    for seq, i in sequential_slots(module, 1):
        if type(seq[i]) is nn.Conv2d and _plain(seq[i]):
            _swap(seq[i], False)
            n += 1
    return n


def fuse_relu(owner, conv_name, relu_name):
    """`owner.<conv_name>` is a plain supported 3x3 nn.Conv2d and `owner.<relu_name>` an nn.ReLU that owner's forward applies right after it (the
    caller's claim: GSRegresser.out_conv / out_relu): the convolution becomes a FusedConv3x3 with relu=True and the ReLU attribute an nn.Identity,
    in place.  A ReLU has no state, so the state_dict is unchanged.  Returns 1, or 0 where either is something else (then nothing changes)."""
    conv, relu = getattr(owner, conv_name, None), getattr(owner, relu_name, None)
    if type(conv) is not nn.Conv2d or type(relu) is not nn.ReLU or not _plain(conv):
        return 0
    _swap(conv, True)
    setattr(owner, relu_name, nn.Identity())
    return 1


def convert_regresser(net):
    """The reference's GSRegresser: `out_conv` + `out_relu` fused, then the 3x3 layer at the top of every head.  Returns the number converted (four
    with the reference's configuration; the encoders' and decoders' 3x3 layers are attributes of ResidualBlock or have other channel counts)."""
    return fuse_relu(net, "out_conv", "out_relu") + convert(net)
