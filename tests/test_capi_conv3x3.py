"""CPU: the 3x3-convolution entry points of the C-ABI (include/gpsgs.h, last section) -- declared, exported, bound; the channel counts c3_supported
takes; the tile; the scratch formula the header states; every bad-argument case refused before any HIP call (this machine has no GPU: a call that
reached HIP would not return GPSGS_E_INVALID)."""
import ctypes as C

import pytest

from gps_gaussian_amd import _capi, _ops

import capi_run
from capi_run import D


def test_symbols_are_declared_exported_and_bound():
    # (with every name in PROTOTYPES and lib()'s argtypes / restype equal to the table's entry)
    lib = capi_run.check_section("c3_", _capi.C3_SYMBOLS, ["c3_backward", "c3_forward", "c3_scratch_bytes", "c3_supported", "c3_tile"])
    # the header's argument lists and the ctypes prototypes agree in length
    for name in _capi.C3_SYMBOLS:
        assert capi_run.declared_arg_count(name) == len(getattr(lib, name).argtypes), name
    assert len(lib.c3_forward.argtypes) == 10 and len(lib.c3_backward.argtypes) == 14
    assert lib.c3_scratch_bytes.restype is C.c_size_t
    assert not set(_capi.C3_SYMBOLS) & set(_capi.SYMBOLS + _capi.GN_SYMBOLS + _capi.GNE_SYMBOLS + _capi.SC_SYMBOLS)


def test_supported_is_exactly_the_table():
    lib = capi_run.lib()
    for Ci in range(-8, 80):
        for Co in (-32, 0, 1, 8, 16, 31, 32, 33, 48, 64):
            want = int(Co == 32 and 4 <= Ci <= 64 and Ci % 4 == 0)
            assert lib.c3_supported(Ci, Co) == want, (Ci, Co)
    assert lib.c3_supported(52, 32) == 1 and lib.c3_supported(32, 32) == 1          # the reference's two shapes


def _tile(lib):
    return _ops.tile("c3_tile")


def _formula(N, Ci, H, W):
    cdiv = lambda a, b: -(-a // b)
    parts = min(512, N * cdiv(H, 4) * cdiv(W, 32))
    return 4 * 32 * (9 * Ci + 1) * (parts + cdiv(parts, 32))


def test_tile_and_the_scratch_formula():
    lib = capi_run.lib()
    TH, TW = _tile(lib)
    assert TH > 0 and TW > 0
    assert lib.c3_tile(None, None) == _capi.GPSGS_E_INVALID
    th = C.c_int(0)
    assert lib.c3_tile(C.byref(th), None) == _capi.GPSGS_E_INVALID and lib.c3_tile(None, C.byref(th)) == _capi.GPSGS_E_INVALID
    f = lib.c3_scratch_bytes
    shapes = [(2, 52, 1024, 1024), (8, 32, 1024, 1024), (1, 4, 1, 1), (3, 8, 2, 3), (1, 52, 37, 41), (2, 64, 33, 65), (2, 52, TH, TW),
              (2, 52, 2 * TH + 1, 2 * TW + 1), (1, 32, 4, 32 * 32), (1, 32, 4, 32 * 33), (1, 32, 4, 32 * 512), (1, 32, 4, 32 * 513)]
    for N, Ci, H, W in shapes:
        assert f(N, Ci, H, W) == _formula(N, Ci, H, W) > 0, (N, Ci, H, W)
    # sized by the grid, not by the tile count: the reference's largest layer stays far below one partial per tile
    assert f(2, 52, 1024, 1024) == f(8, 52, 1024, 1024) == f(2, 52, 2048, 2048) < 64 << 20
    # monotone in N, H and W
    for n in range(1, 200, 7):
        assert f(n + 7, 8, 30, 30) >= f(n, 8, 30, 30) > 0
    for h in range(1, 12 * TH, 5):
        assert f(2, 52, h + 5, 77) >= f(2, 52, h, 77) > 0 and f(2, 52, 77, 3 * h + 15) >= f(2, 52, 77, 3 * h) > 0
    assert f(2, 52, 9, 65) > f(1, 52, 9, 65) and f(1, 52, 9, 65) > f(1, 52, 4, 65) and f(1, 52, 4, 65) > f(1, 52, 4, 64)
    # refused shapes: 0
    assert f(0, 52, 16, 16) == 0 and f(-1, 52, 16, 16) == 0 and f(2, 52, 0, 16) == 0 and f(2, 52, 16, -4) == 0
    assert f(2, 3, 16, 16) == 0 and f(2, 50, 16, 16) == 0 and f(2, 68, 16, 16) == 0 and f(2, 0, 16, 16) == 0
    assert f(8, 32, 8192, 8192) == 0 and f(1, 64, 8192, 4096) == 0                # 2^31 elements or more in y / in x
    assert f(1, 4, 65536, 65536) == 0 and f(2147483647, 4, 2147483647, 2147483647) == 0


# D: a non-NULL, 16-byte aligned "pointer" that is never dereferenced: every call below must return before any HIP call
def _fwd(lib, x=D, w=D, bias=D, N=2, Ci=52, H=16, W=16, relu=1, y=D):
    return lib.c3_forward(x, w, bias, N, Ci, H, W, relu, y, None)


def _bwd(lib, x=D, w=D, y=D, dy=D, N=2, Ci=52, H=16, W=16, relu=1, dx=D, dw=D, dbias=D, scratch=D):
    return lib.c3_backward(x, w, y, dy, N, Ci, H, W, relu, dx, dw, dbias, scratch, None)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["forward", "backward"])
def test_bad_arguments_are_refused_before_hip(call):
    lib = capi_run.lib()
    E = _capi.GPSGS_E_INVALID
    assert call(lib, Ci=0) == E and call(lib, Ci=3) == E and call(lib, Ci=50) == E and call(lib, Ci=68) == E and call(lib, Ci=-4) == E
    assert call(lib, N=0) == E and call(lib, N=-1) == E and call(lib, H=0) == E and call(lib, W=0) == E and call(lib, H=-16) == E
    assert call(lib, relu=2) == E and call(lib, relu=-1) == E
    assert call(lib, x=None) == E and call(lib, w=None) == E
    assert call(lib, x=D + 4) == E and call(lib, w=D + 2) == E                                     # misaligned
    assert call(lib, N=1, Ci=64, H=8192, W=4096) == E                                              # x: 2^31 elements
    assert call(lib, N=4, Ci=4, H=8192, W=8192) == E                                               # x fits (2^30), y: 2^33 elements
    assert call(lib, N=1, Ci=4, H=65536, W=65536) == E
    if call is _fwd:
        assert call(lib, bias=None) == E and call(lib, y=None) == E
        assert call(lib, y=D + 8) == E and call(lib, bias=D + 1) == E
    else:
        assert call(lib, dy=None) == E and call(lib, scratch=None) == E
        assert call(lib, y=None) == E                                                              # the ReLU form needs the saved output
        assert call(lib, dw=None) == E and call(lib, dbias=None) == E                              # one without the other
        assert call(lib, dy=D + 4) == E and call(lib, y=D + 8) == E and call(lib, dx=D + 8) == E and call(lib, dw=D + 2) == E
        assert call(lib, dbias=D + 1) == E and call(lib, scratch=D + 8) == E


def test_nothing_asked_for_launches_nothing():
    lib = capi_run.lib()
    assert _bwd(lib, dx=None, dw=None, dbias=None, scratch=None) == 0
    assert _bwd(lib, dx=None, dw=None, dbias=None, scratch=None, relu=0, y=None) == 0              # without ReLU y may be NULL
    assert _bwd(lib, dx=None, dw=None, dbias=None, scratch=None, Ci=6) == _capi.GPSGS_E_INVALID    # the arguments are still checked
