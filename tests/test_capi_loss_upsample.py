"""CPU: the entry points of the fused L1 + SSIM loss (fl_*) and the convex upsampling (cu_upsample_*) of the C-ABI (include/gpsgs.h): every
bad-argument case is refused before any HIP call (this machine has no GPU: a call that reached HIP would not return GPSGS_E_INVALID), empty
tensors return without a launch, and sizes a launch cannot hold -- more planes or row tiles than a grid's z or y, a tile count beyond an int, a
block count beyond 0x7fffffff -- are refused instead of truncated."""
import pytest

from gps_gaussian_amd import _capi

import capi_run
from capi_run import D

# D: a non-NULL, 16-byte aligned "pointer" that is never dereferenced: every call below must return before any HIP call
E = _capi.GPSGS_E_INVALID
OK = 0


def _lfwd(lib, pred=D, gt=D, planes=6, H=20, W=45, m1=D, m2=D, m3=D, scratch=D, out2=D):
    return lib.fl_l1_ssim_forward(pred, gt, planes, H, W, m1, m2, m3, scratch, out2, None)


def _lbwd(lib, pred=D, gt=D, m1=D, m2=D, m3=D, planes=6, H=20, W=45, gout=D, d_pred=D):
    return lib.fl_l1_ssim_backward(pred, gt, m1, m2, m3, planes, H, W, gout, d_pred, None)


def _ufwd(lib, flow=D, mask=D, out=D, N=2, C=2, H=3, W=65, f=4):
    return lib.cu_upsample_forward(flow, mask, out, N, C, H, W, f, None)


def _ubwd(lib, flow=D, mask=D, gout=D, gflow=D, gmask=D, scratch=D, N=2, C=2, H=3, W=65, f=4):
    return lib.cu_upsample_backward(flow, mask, gout, gflow, gmask, scratch, N, C, H, W, f, None)


def test_loss_scratch_bytes():
    lib = capi_run.lib()
    for planes, H, W in [(1, 1, 1), (6, 20, 45), (3, 32, 32), (3, 33, 32), (3, 32, 33), (2, 2048, 2048), (65535, 33, 71)]:
        tiles = planes * (-(-H // 32)) * (-(-W // 32))
        assert lib.fl_scratch_bytes(planes, H, W) == 8 * tiles + 16, (planes, H, W)
    assert lib.fl_scratch_bytes(-1, 4, 4) == 0 and lib.fl_scratch_bytes(1, -4, 4) == 0 and lib.fl_scratch_bytes(1, 4, -4) == 0
    assert lib.fl_scratch_bytes(0, 4, 4) == 16 and lib.fl_scratch_bytes(1, 0, 4) == 16
    assert lib.fl_scratch_bytes(1, 1, 2 ** 31 - 1) == 8 * 2 ** 26 + 16 and lib.fl_scratch_bytes(1, 2 ** 31 - 1, 1) == 8 * 2 ** 26 + 16      # no wrap in W + 31


@pytest.mark.parametrize("call", [_lfwd, _lbwd], ids=["forward", "backward"])
def test_loss_bad_arguments_are_refused_before_hip(call):
    lib = capi_run.lib()
    assert call(lib, planes=-1) == E and call(lib, H=-1) == E and call(lib, W=-20) == E
    assert call(lib, pred=None) == E and call(lib, gt=None) == E
    if call is _lfwd:
        assert call(lib, scratch=None) == E and call(lib, out2=None) == E
        for part in (dict(m1=None), dict(m2=None), dict(m3=None), dict(m1=None, m2=None), dict(m2=None, m3=None), dict(m1=None, m3=None)):
            assert call(lib, **part) == E, part                      # the derivative maps: all three or none
        for empty in (dict(planes=0), dict(H=0), dict(W=0)):
            assert call(lib, **empty) == E, empty                    # a mean over nothing
    else:
        assert call(lib, m1=None) == E and call(lib, m2=None) == E and call(lib, m3=None) == E
        assert call(lib, gout=None) == E and call(lib, d_pred=None) == E
        for empty in (dict(planes=0), dict(H=0), dict(W=0)):
            assert call(lib, **empty) == OK, empty                   # nothing to write
            assert call(lib, pred=None, gt=None, m1=None, m2=None, m3=None, d_pred=None, **empty) == OK     # torch hands out NULL for an empty tensor
        assert call(lib, planes=0, H=-1) == E                        # the sizes are still checked


@pytest.mark.parametrize("call", [_lfwd, _lbwd], ids=["forward", "backward"])
def test_loss_sizes_the_grid_cannot_hold_are_refused(call):
    lib = capi_run.lib()
    assert call(lib, planes=65536, H=1, W=1) == E                    # grid z
    assert call(lib, planes=1, H=65535 * 32 + 1, W=1) == E           # grid y: 65536 row tiles
    assert call(lib, planes=65535, H=65535 * 32, W=32) == E          # 65535 x 65535 x 1 tiles: more than an int counts
    assert call(lib, planes=2, H=65535 * 32, W=16385 * 32) == E      # 2 x 65535 x 16385 = 2^31 + 32766
    assert call(lib, planes=1, H=2 ** 31 - 1, W=2 ** 31 - 1) == E
    assert call(lib, planes=1, H=1, W=2 ** 31 - 1) == E and call(lib, planes=1, H=1, W=2 ** 31 - 31) == E      # W + 31 wraps in int


@pytest.mark.parametrize("call", [_ufwd, _ubwd], ids=["forward", "backward"])
def test_upsample_bad_arguments_are_refused_before_hip(call):
    lib = capi_run.lib()
    assert call(lib, N=-1) == E and call(lib, H=-3) == E and call(lib, W=-65) == E
    assert call(lib, C=0) == E and call(lib, C=-1) == E and call(lib, C=5) == E
    assert call(lib, f=0) == E and call(lib, f=-4) == E and call(lib, f=17) == E
    assert call(lib, flow=None) == E and call(lib, mask=None) == E
    for empty in (dict(N=0), dict(H=0), dict(W=0)):
        assert call(lib, **empty) == OK, empty
        assert call(lib, flow=None, mask=None, **empty) == OK         # torch hands out NULL for an empty tensor
        assert call(lib, C=0, **empty) == E and call(lib, f=0, **empty) == E   # the arguments are still checked
    if call is _ufwd:
        assert call(lib, out=None) == E
    else:
        assert call(lib, C=3) == E and call(lib, C=4) == E           # the backward holds two channels in registers
        assert call(lib, gout=None) == E
        assert call(lib, gflow=None, gmask=None) == E                # neither gradient
        assert call(lib, scratch=None) == E                          # grad_flow without scratch
        assert call(lib, gmask=None, scratch=None) == E
        assert call(lib, N=65536, H=1, W=1) == E and call(lib, N=1, H=65536, W=1) == E     # grid z and y


def test_upsample_scratch_bytes():
    lib = capi_run.lib()
    assert lib.cu_upsample_scratch_bytes(2, 2, 3, 65) == 2 * 9 * 2 * 3 * 65 * 4
    assert lib.cu_upsample_scratch_bytes(1, 1, 1, 1) == 36
    for bad in ((0, 2, 3, 65), (2, 0, 3, 65), (2, 2, 0, 65), (2, 2, 3, 0), (-2, 2, 3, 65), (2, -2, 3, 65), (2, 2, -3, 65), (2, 2, 3, -65)):
        assert lib.cu_upsample_scratch_bytes(*bad) == 0, bad


def test_upsample_block_counts_beyond_a_grid_are_refused():
    """One thread per output pixel (forward) resp. per flow element (k_up_bwd_flow) in blocks of 256: the count used to be cast to unsigned."""
    lib = capi_run.lib()
    # forward: N f H f W = 2^39 + 2^31 pixels -> 2^31 + 2^23 blocks (the cast kept 2^23 of them)
    assert _ufwd(lib, N=2 ** 15 + 2 ** 7, H=2 ** 10, W=2 ** 6, f=16) == E
    assert _ufwd(lib, N=1, H=2 ** 30, W=2 ** 9, f=1) == E             # exactly 2^31 blocks (the cast kept none)
    assert _ufwd(lib, N=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1, f=16) == E   # a product that does not fit 64 bits either
    # backward: N C H W = 2^39 flow elements; without grad_flow that kernel is not launched, so only the forward's sibling is refused
    assert _ubwd(lib, N=2 ** 14, C=2, H=2 ** 14, W=2 ** 10) == E
    assert _ubwd(lib, N=65535, C=2, H=65535, W=2 ** 31 - 1) == E
    # sizes the kernels form in int: f H, f W, W + 63
    for call in (_ufwd, _ubwd):
        assert call(lib, N=1, H=1, W=2 ** 31 - 1, f=16) == E and call(lib, N=1, H=2 ** 28, W=1, f=16) == E
        assert call(lib, N=1, C=1, H=1, W=2 ** 31 - 1, f=1) == E and call(lib, N=1, C=1, H=1, W=2 ** 31 - 63, f=1) == E
