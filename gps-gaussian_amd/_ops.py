"""The one way an op module calls the C-ABI: pointers as plain ints, the current stream appended, the device guard only when it is needed, the
return code checked under the entry point's own name.  The tensor-aware side of _capi.py (which stays free of torch).  And what the converted
layers (groupnorm.py, stemconv.py, gshead.py) say in the same words: how a parameter reaches a kernel, which input and parameters a fused
forward takes, and the two walks over a module tree that convert it in place.  And the shell of the convolution ops' autograd functions (stemconv.py,
gshead.py, conv3x3.py, conv1x1.py): conv_inputs / grad_buffers / param_grads around each op's own C-ABI calls, plain_conv and tile."""
import ctypes
import functools

import torch
from torch import nn

from . import _capi

DTYPE_CODE = {torch.float32: 0, torch.float16: 1}   # the `dtype` argument of include/gpsgs.h


def ptr(t):
    return t.data_ptr() if t is not None else None  # ctypes converts a Python int to the void* argument (boxing it in c_void_p costs ~1 us)


class _NoGuard:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


_NOGUARD = _NoGuard()


def device_guard(dev):
    # switching the current device costs ~10 us; skip it when the tensors already live on the current device
    return _NOGUARD if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)


def call(name, dev, *args):
    """One C-ABI call `name(*args, stream)` on the current stream of `dev`; a non-zero return code is a RuntimeError naming the entry point."""
    fn = getattr(_capi.lib(), name)
    with device_guard(dev):
        rc = fn(*args, torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        _capi.check(rc, name)


def aligned16(t):
    """Contiguous and 16-byte aligned (a fresh allocation always is; a view into a larger tensor may start anywhere)."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def autocast_dtype():
    get = getattr(torch, "get_autocast_dtype", None)      # newer torch; the older accessor warns there
    return get("cuda") if get is not None else torch.get_autocast_gpu_dtype()


def fp32_on(dev, weight, bias):
    """A layer's weight and bias as the kernels read them: detached, fp32, on `dev`, contiguous (one call for the pair: this is on every forward)."""
    return weight.detach().to(device=dev, dtype=torch.float32).contiguous(), bias.detach().to(device=dev, dtype=torch.float32).contiguous()


def conv_inputs(op, x_shape, w_shape, x, weight, bias, wdims=(4,)):
    """The opening lines of a convolution op's autograd forward: x must be an fp32 4-D GPU tensor, the weight have one of `wdims` dimensions and
    the bias be there -- else a RuntimeError in the op's name.  Returns x detached and aligned16, and fp32_on(weight, bias)."""
    if not x.is_cuda:
        raise RuntimeError("gps_gaussian_amd: %s input must live on a GPU (no CPU fallback)" % op)
    if x.dtype != torch.float32 or x.dim() != 4 or bias is None or weight.dim() not in wdims:
        raise RuntimeError("gps_gaussian_amd: %s takes an fp32 %s input, a %s weight and a bias" % (op, x_shape, w_shape))
    return (aligned16(x.detach()),) + fp32_on(x.device, weight, bias)


def grad_buffers(xc, needs, wshape, scratch_bytes, *dims):
    """What a convolution op's backward writes, by ctx.needs_input_grad: dx like xc where x wants a gradient (None: nothing is computed for it); dw
    [wshape], db [wshape[0]] and scratch_bytes(*dims) bytes of scratch, all fp32, where either parameter wants one (the kernels write both or
    neither), else three None."""
    dx = torch.empty_like(xc) if needs[0] else None
    if not (needs[1] or needs[2]):
        return dx, None, None, None
    new = functools.partial(torch.empty, dtype=torch.float32, device=xc.device)
    return dx, new(tuple(wshape)), new((wshape[0],)), new((scratch_bytes(*dims) // 4,))


def param_grads(needs, dw, db, wdt, bdt):
    """The parameter gradients as autograd takes them: in the parameters' dtypes, None where none was asked for."""
    return dw.to(wdt) if needs[1] else None, db.to(bdt) if needs[2] else None


def plain_conv(conv, k, pad, supported, strides=((1, 1),)):
    """A convolution whose static configuration is a fused op's: k x k, a stride among `strides` (stride 1 unless told otherwise), padding `pad`,
    dilation 1, groups 1, zero padding mode, a bias, channel counts that `supported` takes."""
    return conv.kernel_size == (k, k) and conv.stride in strides and conv.padding == (pad, pad) and conv.dilation == (1, 1) and conv.groups == 1 \
        and conv.bias is not None and conv.padding_mode == "zeros" and supported(conv.in_channels, conv.out_channels)


@functools.lru_cache(maxsize=None)
def tile(name):
    """(rows, columns) of a workgroup's output tile as the entry point `name` reports it (sc_tile, c3_tile)."""
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    _capi.check(getattr(_capi.lib(), name)(ctypes.byref(th), ctypes.byref(tw)), name)
    return th.value, tw.value


def dense_fp32_call(m, x):
    """x is a contiguous 4-D fp32 GPU tensor with elements in it (not: CPU, fp16 / bf16, empty, channels-last or any other strided view) and the
    layer m has a bias and keeps it and its weight in fp32 on x's device (one predicate for both: this is on every forward)."""
    return x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and x.numel() > 0 and x.is_contiguous() and m.bias is not None \
        and m.weight.dtype == torch.float32 and m.bias.dtype == torch.float32 and m.weight.device == x.device


def swap_class(module, old, new, test=None):
    """Every module of exactly type `old` in `module`'s tree (the module itself included; one reachable through two parents once) that passes
    `test` becomes a `new`, in place: the instance keeps its parameters, buffers, hooks and state_dict keys.  Returns the number swapped."""
    n = 0
    for m in module.modules():
        if type(m) is old and (test is None or test(m)):
            m.__class__ = new
            n += 1
    return n


def sequential_slots(module, span=2):
    """(seq, i) for every run of `span` adjacent slots i, i + 1, ... of every nn.Sequential in `module`'s tree (the module itself included)."""
    for seq in list(module.modules()):
        if isinstance(seq, nn.Sequential):
            for i in range(len(seq) - span + 1):
                yield seq, i
