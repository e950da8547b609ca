"""GPU (-m gpu): the op layer's one call path (gps_gaussian_amd/_ops.py) -- a refused call is a RuntimeError that names its entry point, and
`ptr` hands over None as NULL and an empty tensor as whatever pointer it has.  Tiny tensors, no kernel worth timing."""
import pytest
import torch

import gps_gaussian_amd  # noqa: F401
from gps_gaussian_amd import _capi, _ops
from gps_gaussian_amd._ops import ptr

pytestmark = pytest.mark.gpu


def test_call_names_the_refused_entry_point_and_ptr_passes_null():
    dev = torch.device("cuda", torch.cuda.current_device())
    N, C, G, HW = 1, 2, 1, 4
    x = torch.randn((N, C, 2, 2), device=dev)
    w, b = torch.ones((C,), device=dev), torch.zeros((C,), device=dev)
    y, mean, rstd = (torch.full(s, 7.0, device=dev) for s in ((N, C, 2, 2), (N, G), (N, G)))
    scratch = torch.full((_capi.lib().gn_scratch_bytes(N, C, G, HW) // 4 + 4,), 7.0, device=dev)
    with pytest.raises(RuntimeError) as e:     # G = 0: refused by the argument check, before any launch
        _ops.call("gn_forward", dev, ptr(x), _ops.DTYPE_CODE[x.dtype], ptr(w), ptr(b), N, C, 0, HW, 1e-5, ptr(y), ptr(mean), ptr(rstd), ptr(scratch))
    assert "gn_forward" in str(e.value) and "invalid argument" in str(e.value)
    torch.cuda.synchronize(dev)
    assert all(bool((t == 7.0).all()) for t in (y, mean, rstd, scratch))   # nothing ran

    assert ptr(None) is None
    ex, ey, em = (torch.empty(s, device=dev) for s in ((0, C, 2, 2), (0, C, 2, 2), (0, G)))
    # an empty tensor's pointer (NULL where it has no storage) with N = 0: nothing to do, no error
    assert _ops.call("gn_forward", dev, ptr(ex), 0, ptr(w), ptr(b), 0, C, G, HW, 1e-5, ptr(ey), ptr(em), ptr(em), ptr(scratch)) is None
    torch.cuda.synchronize(dev)
    assert bool((scratch == 7.0).all())
