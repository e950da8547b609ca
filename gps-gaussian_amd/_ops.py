"""The one way an op module calls the C-ABI: pointers as plain ints, the current stream appended, the device guard only when it is needed, the
return code checked under the entry point's own name.  The tensor-aware side of _capi.py (which stays free of torch)."""
import torch

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
