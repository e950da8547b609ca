"""CPU: the 1x1-convolution entry points of the C-ABI (include/gpsgs.h, last section) -- declared, exported, bound; the configurations c1_supported
takes; the tile; the scratch formula the header states; every bad-argument case refused before any HIP call (this machine has no GPU: a call that
reached HIP would not return GPSGS_E_INVALID)."""
import ctypes as C

import pytest

from gps_gaussian_amd import _capi
from gps_gaussian_amd import conv1x1 as C1

import capi_run
from capi_run import D

NAMES = ["c1_backward", "c1_forward", "c1_scratch_bytes", "c1_supported", "c1_tile"]


def test_symbols_are_declared_exported_and_bound():
    # (with every name in PROTOTYPES and lib()'s argtypes / restype equal to the table's entry)
    lib = capi_run.check_section("c1_", _capi.C1_SYMBOLS, NAMES)
    # the header's argument lists and the ctypes prototypes agree in length
    for name in NAMES:
        assert capi_run.declared_arg_count(name) == len(_capi.PROTOTYPES[name][1]), name
    assert len(lib.c1_forward.argtypes) == 11 and len(lib.c1_backward.argtypes) == 14
    assert lib.c1_scratch_bytes.restype is C.c_size_t
    assert not set(_capi.C1_SYMBOLS) & set(_capi.SYMBOLS + _capi.GN_SYMBOLS + _capi.GNE_SYMBOLS + _capi.SC_SYMBOLS + _capi.C3_SYMBOLS)


def test_supported_is_exactly_the_table():
    lib = capi_run.lib()
    for Ci in list(range(-8, 72)) + [124, 128, 192, 252, 255, 256, 257, 260, 512]:
        for Co in (-16, 0, 1, 8, 15, 16, 17, 24, 32, 48, 64, 96, 112, 128, 129, 144, 256):
            for s in (-1, 0, 1, 2, 3, 4):
                want = int(4 <= Ci <= 256 and Ci % 4 == 0 and 16 <= Co <= 128 and Co % 16 == 0 and s in (1, 2))
                assert lib.c1_supported(Ci, Co, s) == want, (Ci, Co, s)
                assert C1.supported(Ci, Co, s) is bool(want)
    # the shortcuts of the reference's two width configurations (config/stage2.yaml and the defaults [64, 96, 128])
    for Ci, Co, s in ((32, 48, 2), (48, 96, 2), (192, 96, 1), (192, 64, 1), (128, 48, 1), (32, 64, 1), (64, 96, 2), (96, 128, 2), (256, 128, 1)):
        assert lib.c1_supported(Ci, Co, s) == 1, (Ci, Co, s)


def _formula(N, Ci, Co, H, W, s):
    cdiv = lambda a, b: -(-a // b)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    parts = min(512, N * cdiv(Ho * Wo, 32))
    return 4 * Co * (Ci + 1) * (parts + cdiv(parts, 32))


def test_tile_and_the_scratch_formula():
    lib = capi_run.lib()
    TP, WP, PARTS = C1.tile()
    assert TP > 0 and WP > 0 and PARTS > 0 and (WP, PARTS) == (32, 512)          # the two numbers the header's formula states
    a, b = C.c_int(0), C.c_int(0)
    E = _capi.GPSGS_E_INVALID
    assert lib.c1_tile(None, None, None) == E and lib.c1_tile(C.byref(a), C.byref(b), None) == E
    assert lib.c1_tile(None, C.byref(a), C.byref(b)) == E and lib.c1_tile(C.byref(a), None, C.byref(b)) == E
    f = lib.c1_scratch_bytes
    shapes = [(2, 32, 48, 512, 512, 2), (2, 48, 96, 256, 256, 2), (2, 192, 96, 128, 128, 1), (2, 192, 64, 256, 256, 1), (2, 128, 48, 512, 512, 1),
              (8, 32, 64, 512, 512, 1), (1, 4, 16, 1, 1, 1), (1, 4, 16, 1, 1, 2), (3, 32, 48, 5, 7, 2), (2, 48, 96, 6, 8, 2), (1, 256, 128, 3, 5, 1),
              (1, 4, 16, 1, WP * PARTS, 1), (1, 4, 16, 1, WP * PARTS + 1, 1), (1, 4, 16, 33, 32, 1), (1, 4, 16, 2, 2 * WP * 32 + 1, 2)]
    for N, Ci, Co, H, W, s in shapes:
        assert f(N, Ci, Co, H, W, s) == _formula(N, Ci, Co, H, W, s) > 0, (N, Ci, Co, H, W, s)
    # sized by the grid, not by the tile count
    assert f(2, 128, 48, 512, 512, 1) == f(8, 128, 48, 512, 512, 1) == f(2, 128, 48, 1024, 1024, 2) < 16 << 20
    assert f(1, 256, 128, 1024, 1024, 1) < 80 << 20                                # the largest partial there is, 512 times and the group sums
    # monotone in N, H and W; stride 2 never needs more than stride 1
    for n in range(1, 200, 7):
        assert f(n + 7, 8, 16, 30, 30, 1) >= f(n, 8, 16, 30, 30, 1) > 0
    for h in range(1, 100, 5):
        assert f(2, 32, 48, h + 5, 77, 2) >= f(2, 32, 48, h, 77, 2) > 0 and f(2, 32, 48, 77, 3 * h + 15, 1) >= f(2, 32, 48, 77, 3 * h, 1) > 0
        assert f(2, 32, 48, h, 77, 2) <= f(2, 32, 48, h, 77, 1)
    assert f(2, 32, 48, 4, 8, 1) > f(1, 32, 48, 4, 8, 1) and f(1, 32, 48, 5, 8, 1) > f(1, 32, 48, 4, 8, 1) and f(1, 32, 48, 4, 9, 1) > f(1, 32, 48, 4, 8, 1)
    # refused shapes: 0
    assert f(0, 32, 48, 16, 16, 1) == 0 and f(-1, 32, 48, 16, 16, 1) == 0 and f(2, 32, 48, 0, 16, 1) == 0 and f(2, 32, 48, 16, -4, 1) == 0
    assert f(2, 3, 48, 16, 16, 1) == 0 and f(2, 30, 48, 16, 16, 1) == 0 and f(2, 260, 48, 16, 16, 1) == 0 and f(2, 0, 48, 16, 16, 1) == 0
    assert f(2, 32, 40, 16, 16, 1) == 0 and f(2, 32, 144, 16, 16, 1) == 0 and f(2, 32, 8, 16, 16, 1) == 0
    assert f(2, 32, 48, 16, 16, 0) == 0 and f(2, 32, 48, 16, 16, 3) == 0
    assert f(1, 256, 16, 4096, 2048, 1) == 0 and f(1, 4, 64, 8192, 8192, 1) == 0                  # 2^31 elements in x / 2^32 in y (x: 2^28)
    assert f(1, 4, 64, 8192, 8192, 2) > 0                                                            # stride 2: y has 2^30
    assert f(1, 4, 16, 65536, 65536, 1) == 0 and f(2147483647, 4, 16, 2147483647, 2147483647, 2) == 0


# D: a non-NULL, 16-byte aligned "pointer" that is never dereferenced: every call below must return before any HIP call
def _fwd(lib, x=D, w=D, bias=D, N=2, Ci=32, Co=48, H=16, W=16, stride=2, y=D):
    return lib.c1_forward(x, w, bias, N, Ci, Co, H, W, stride, y, None)


def _bwd(lib, x=D, w=D, dy=D, N=2, Ci=32, Co=48, H=16, W=16, stride=2, dx=D, dw=D, dbias=D, scratch=D):
    return lib.c1_backward(x, w, dy, N, Ci, Co, H, W, stride, dx, dw, dbias, scratch, None)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["forward", "backward"])
def test_bad_arguments_are_refused_before_hip(call):
    lib = capi_run.lib()
    E = _capi.GPSGS_E_INVALID
    assert call(lib, Ci=0) == E and call(lib, Ci=3) == E and call(lib, Ci=30) == E and call(lib, Ci=260) == E and call(lib, Ci=-4) == E
    assert call(lib, Co=0) == E and call(lib, Co=8) == E and call(lib, Co=40) == E and call(lib, Co=144) == E and call(lib, Co=-16) == E
    assert call(lib, stride=0) == E and call(lib, stride=3) == E and call(lib, stride=-1) == E and call(lib, stride=4) == E
    assert call(lib, N=0) == E and call(lib, N=-1) == E and call(lib, H=0) == E and call(lib, W=0) == E and call(lib, H=-16) == E
    assert call(lib, x=None) == E and call(lib, w=None) == E
    assert call(lib, x=D + 4) == E and call(lib, w=D + 2) == E                                     # misaligned
    assert call(lib, N=1, Ci=256, Co=16, H=4096, W=2048) == E                                      # x: 2^31 elements
    assert call(lib, N=1, Ci=4, Co=128, H=8192, W=8192, stride=1) == E                             # x fits (2^28), y: 2^33 elements
    assert call(lib, N=1, Ci=4, Co=16, H=65536, W=65536) == E
    if call is _fwd:
        assert call(lib, bias=None) == E and call(lib, y=None) == E
        assert call(lib, y=D + 8) == E and call(lib, bias=D + 1) == E
    else:
        assert call(lib, dy=None) == E and call(lib, scratch=None) == E
        assert call(lib, dw=None) == E and call(lib, dbias=None) == E                              # one without the other
        assert call(lib, dy=D + 4) == E and call(lib, dx=D + 8) == E and call(lib, dw=D + 2) == E
        assert call(lib, dbias=D + 1) == E and call(lib, scratch=D + 8) == E


def test_nothing_asked_for_launches_nothing():
    lib = capi_run.lib()
    assert _bwd(lib, dx=None, dw=None, dbias=None, scratch=None) == 0
    assert _bwd(lib, dx=None, dw=None, dbias=None, scratch=None, stride=1) == 0
    assert _bwd(lib, dx=None, dw=None, dbias=None, scratch=None, Ci=6) == _capi.GPSGS_E_INVALID    # the arguments are still checked
    assert _bwd(lib, dx=None, dw=None, dbias=None, scratch=None, stride=3) == _capi.GPSGS_E_INVALID
