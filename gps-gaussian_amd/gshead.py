"""The tail of a Gaussian-parameter head -- ReLU -> Conv2d(C, K <= 4, 1) -> nothing | Softplus | Sigmoid -- forward and backward, as ONE pass over
the hidden tensor on the HIP kernels of csrc/gshead.hip (gsr_head_forward / gsr_head_backward of include/gpsgs.h).

The reference's three heads (lib/gs_parm_network.py:34-50) end in a 1x1 convolution from 32 channels to 4, 3 and 1 on the full-resolution map.  ATen
makes a ReLU pass over that map, a 1x1 implicit GEMM between layout transposes and an elementwise activation; the kernels here read the map once,
in NCHW as it lies, and write the K planes once (DESIGN.md "Gaussian heads").

  head(x, weight, bias, act, beta, threshold)   the op (autograd): act(conv1x1(relu(x))); GPU tensors only, like every other op of this package
  FusedHeadConv                                 nn.Conv2d whose forward IS that function: the op where it applies, the same three torch calls elsewhere
  convert(module)                               ReLU -> Conv2d 1x1 (-> Softplus | Sigmoid) inside every nn.Sequential of a module tree, in place

`GPSGS_ACCELERATE=gshead` makes the reference's GSRegresser call convert() on itself (accelerate.py)."""
import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd.function import once_differentiable

from . import _capi, accelerate
from ._ops import aligned16, call, conv_inputs, dense_fp32_call, grad_buffers, param_grads, plain_conv, ptr, sequential_slots

ACT_CODE = {"none": 0, "softplus": 1, "sigmoid": 2}   # the `act` argument of include/gpsgs.h


def supported(C_in, C_out, act="none"):
    """(C_in, C_out, act) is one the kernels implement (gsr_head_supported): C_in 16 / 32 / 64, 1 <= C_out <= 4."""
    return act in ACT_CODE and bool(_capi.lib().gsr_head_supported(int(C_in), int(C_out), ACT_CODE[act]))


class _Head(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, act, beta, threshold):
        xc, w, b = conv_inputs("head", "[N, C, H, W]", "[K, C] (or [K, C, 1, 1])", x, weight, bias, wdims=(2, 4))
        N, C, H, W = x.shape
        K = weight.shape[0]
        if weight.numel() != K * C or act not in ACT_CODE or bias.numel() != K or x.numel() == 0 or not supported(C, K, act) \
                or (act == "softplus" and not beta > 0):
            raise RuntimeError("gps_gaussian_amd: head: unsupported configuration: input %s, weight %s, act %r, beta %r"
                               % (tuple(x.shape), tuple(weight.shape), act, beta))
        dev = x.device
        y = torch.empty((N, K, H, W), dtype=torch.float32, device=dev)
        cfg = (ACT_CODE[act], float(beta), float(threshold))
        call("gsr_head_forward", dev, ptr(xc), ptr(w), ptr(b), N, C, K, H, W, *cfg, ptr(y))
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(xc, w, b)     # act' is recomputed from x: y is not kept
            ctx.cfg = cfg
            ctx.like = (weight.dtype, bias.dtype)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        xc, w, b = ctx.saved_tensors
        N, C, H, W = xc.shape
        K = w.shape[0]
        needs = ctx.needs_input_grad
        dyc = aligned16(dy.to(torch.float32))
        # nothing is computed for the input gradient unless x wants one; dw has the weight's shape, [K, C] or [K, C, 1, 1]: the same memory
        dx, dw, db, scratch = grad_buffers(xc, needs, w.shape, _capi.lib().gsr_head_scratch_bytes, N, C, K, H, W)
        call("gsr_head_backward", xc.device, ptr(xc), ptr(w), ptr(b), None, ptr(dyc), N, C, K, H, W, *ctx.cfg, ptr(dx), ptr(dw), ptr(db), ptr(scratch))
        return (dx,) + param_grads(needs, dw, db, *ctx.like) + (None, None, None)


def head(x, weight, bias, act="none", beta=1.0, threshold=20.0):
    """act(conv1x1(relu(x))) for an fp32 GPU tensor x [N, C, H, W], weight [K, C] or [K, C, 1, 1] and bias [K], with C in {16, 32, 64} and K <= 4;
    act "none", "softplus" (torch's softplus(beta, threshold)) or "sigmoid".  Anything else is a RuntimeError.  fp32 throughout; gradients come back
    in the parameters' dtypes (and the weight's shape), x.grad in fp32 and zero where x <= 0; the input gradient is computed only if x requires
    grad."""
    return _Head.apply(x, weight, bias, act, beta, threshold)


def _plain(conv):
    """A convolution whose static configuration is the op's: 1x1, no padding, otherwise plain_conv's, a supported (C_in, C_out)."""
    return plain_conv(conv, 1, 0, supported)


def _fusable(m, x):
    if not dense_fp32_call(m, x) or torch.is_autocast_enabled():
        return False                                      # ... the heads run outside autocast (lib/network.py:32-33); inside it, ATen decides the dtypes
    return x.shape[1] == m.in_channels and _plain(m) and m.act in ACT_CODE and (m.act != "softplus" or m.beta > 0)


class FusedHeadConv(nn.Conv2d):
    """nn.Conv2d(C, K, 1) that computes act(conv(relu(x))) -- the ReLU in front of it and the activation behind it are part of this module; convert()
    leaves nn.Identity in their slots.  The fused op runs for a contiguous 4-D fp32 GPU tensor with elements in it, fp32 parameters on the same
    device, no autocast and a supported (C, K).  Everything else is the same function in torch -- torch.relu, nn.Conv2d.forward, the activation --
    counted in accelerate.calls["gshead_passthrough"].  Same parameters, same state_dict."""
    act, beta, threshold = "none", 1.0, 20.0

    def forward(self, input):
        if _fusable(self, input):
            accelerate.calls["gshead"] += 1
            return _Head.apply(input, self.weight, self.bias, self.act, self.beta, self.threshold)
        accelerate.calls["gshead_passthrough"] += 1
        y = nn.Conv2d.forward(self, torch.relu(input))
        if self.act == "softplus":
            return F.softplus(y, self.beta, self.threshold)
        return torch.sigmoid(y) if self.act == "sigmoid" else y

    def extra_repr(self):
        return "%s, act=%s%s" % (nn.Conv2d.extra_repr(self), self.act, ", beta=%g, threshold=%g" % (self.beta, self.threshold) if self.act == "softplus" else "")


def convert(module):
    """In every nn.Sequential of `module`'s tree (the module itself included): an nn.ReLU directly followed by a plain nn.Conv2d -- 1x1, stride 1, no
    padding, groups 1, a bias, zero padding mode, a supported (C_in, C_out) -- and, optionally, by an nn.Softplus or nn.Sigmoid becomes one
    FusedHeadConv, in place: the convolution keeps its parameters, hooks and state_dict key and only changes class, the ReLU's and the activation's
    slots become nn.Identity (they have no state), indices stay.  A ReLU followed by anything else, subclasses of these layers and already converted
    chains are left alone.  Returns the number converted."""
    n = 0
    for seq, i in sequential_slots(module):
        relu, conv = seq[i], seq[i + 1]
        if type(relu) is not nn.ReLU or type(conv) is not nn.Conv2d or not _plain(conv):
            continue
        after = seq[i + 2] if i + 2 < len(seq) else None
        act, beta, threshold = "none", 1.0, 20.0
        if type(after) is nn.Softplus:
            act, beta, threshold = "softplus", after.beta, after.threshold
        elif type(after) is nn.Sigmoid:
            act = "sigmoid"
        if not supported(conv.in_channels, conv.out_channels, act):
            continue
        conv.__class__ = FusedHeadConv
        conv.act, conv.beta, conv.threshold = act, beta, threshold
        seq[i] = nn.Identity()
        if act != "none":
            seq[i + 2] = nn.Identity()
        n += 1
    return n
