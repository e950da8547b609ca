"""CPU: the residual-block 3x3-convolution entry points of the C-ABI (include/gpsgs.h, the section before the decoder glue) -- declared, exported,
bound; the channel counts rc_supported takes; the tile; the scratch formula the header states and its 64 MiB ceiling; every bad-argument case
refused before any HIP call (this machine has no GPU: a call that reached HIP would not return GPSGS_E_INVALID); a backward that is asked for
nothing launches nothing."""
import ctypes as C

import pytest

from gps_gaussian_amd import _capi, _ops

import capi_run
from capi_run import D

NAMES = ["rc_backward", "rc_forward", "rc_scratch_bytes", "rc_supported", "rc_tile"]
E = _capi.GPSGS_E_INVALID


def test_symbols_are_declared_exported_and_bound():
    lib = capi_run.check_section("rc_", _capi.RC_SYMBOLS, NAMES)
    for name in NAMES:
        assert capi_run.declared_arg_count(name) == len(getattr(lib, name).argtypes), name
    assert len(lib.rc_forward.argtypes) == 10 and len(lib.rc_backward.argtypes) == 13
    assert lib.rc_scratch_bytes.restype is C.c_size_t
    assert _capi.SECTIONS[-2] == _capi.RC_SYMBOLS and _capi.SECTIONS[-1] == _capi.UC_SYMBOLS     # before the decoder glue, which stays last
    assert not set(_capi.RC_SYMBOLS) & set(sum(_capi.SECTIONS[:-2], ()) + _capi.UC_SYMBOLS)
    head = capi_run.header()
    assert head.index("int rc_backward(") < head.index("int uc_supported(") and head.index("int c1_backward(") < head.index("int rc_supported(")


def _want(Ci, Co):
    return int(4 <= Ci <= 192 and Ci % 4 == 0 and 16 <= Co <= 96 and Co % 16 == 0)


def test_supported_is_exactly_the_table():
    lib = capi_run.lib()
    for Ci in sorted(set(range(-8, 204)) | {0, 3, 100, 192, 196, 256}):
        for Co in (-16, 0, 1, 8, 15, 16, 17, 24, 32, 40, 48, 64, 80, 95, 96, 97, 100, 112, 128):
            assert lib.rc_supported(Ci, Co) == _want(Ci, Co), (Ci, Co)
    for Ci in (0, 3, 196):
        assert lib.rc_supported(Ci, 48) == 0
    for Co in (0, 24, 112):
        assert lib.rc_supported(100, Co) == 0
    assert lib.rc_supported(100, 16) == 1 and lib.rc_supported(192, 96) == 1 and lib.rc_supported(4, 16) == 1
    for pair in ((32, 32), (48, 48), (64, 64), (96, 96), (128, 48), (192, 64), (192, 96)):           # stage 2's seven
        assert lib.rc_supported(*pair) == 1, pair


def _cdiv(a, b):
    return -(-a // b)


def _parts(N, Ci, Co, H, W):
    return min(512 // (_cdiv(Co, 32) * _cdiv(Ci, 64)), N * _cdiv(H, 4) * _cdiv(W, 32))


def _formula(N, Ci, Co, H, W):
    parts = _parts(N, Ci, Co, H, W)
    return 4 * Co * (9 * Ci + 1) * (parts + _cdiv(parts, 32))


def test_tile_and_the_scratch_formula():
    lib = capi_run.lib()
    TH, TW = _ops.tile("rc_tile")
    assert TH > 0 and TW > 0
    assert lib.rc_tile(None, None) == E
    th = C.c_int(0)
    assert lib.rc_tile(C.byref(th), None) == E and lib.rc_tile(None, C.byref(th)) == E
    f = lib.rc_scratch_bytes
    shapes = [(2, 32, 32, 512, 512), (2, 128, 48, 512, 512), (8, 192, 64, 256, 256), (2, 192, 96, 128, 128), (1, 4, 16, 1, 1), (3, 8, 16, 2, 3),
              (1, 52, 48, 37, 41), (2, 36, 80, 9, TW + 3), (2, 100, 48, TH, TW), (1, 4, 16, 4, 32 * 32), (1, 4, 16, 4, 32 * 33), (1, 4, 16, 4, 32 * 512),
              (1, 4, 16, 4, 32 * 513), (1, 192, 96, 4, 32 * 56), (1, 192, 96, 4, 32 * 57), (1, 68, 48, 4, 32 * 128), (1, 68, 48, 4, 32 * 129)]
    for s in shapes:
        assert f(*s) == _formula(*s) > 0, s
    # sized by the grid, not by the tile count
    assert f(2, 192, 96, 128, 128) == f(8, 192, 96, 128, 128) == f(2, 192, 96, 2048, 2048)
    # monotone in N, H and W
    for n in range(1, 200, 7):
        assert f(n + 7, 8, 16, 30, 30) >= f(n, 8, 16, 30, 30) > 0
    for h in range(1, 12 * TH, 5):
        assert f(2, 52, 48, h + 5, 77) >= f(2, 52, 48, h, 77) > 0 and f(2, 52, 48, 77, 3 * h + 15) >= f(2, 52, 48, 77, 3 * h) > 0
    # refused dimensions: 0
    assert f(0, 48, 48, 16, 16) == 0 and f(-1, 48, 48, 16, 16) == 0 and f(2, 48, 48, 0, 16) == 0 and f(2, 48, 48, 16, -4) == 0
    assert f(2, 3, 48, 16, 16) == 0 and f(2, 50, 48, 16, 16) == 0 and f(2, 196, 48, 16, 16) == 0 and f(2, 0, 48, 16, 16) == 0
    assert f(2, 48, 0, 16, 16) == 0 and f(2, 48, 24, 16, 16) == 0 and f(2, 48, 112, 16, 16) == 0 and f(2, 48, 8, 16, 16) == 0
    assert f(8, 16, 96, 4096, 4096) == 0 and f(1, 192, 16, 4096, 4096) == 0            # 2^31 elements or more in y / in x
    assert f(1, 4, 16, 65536, 65536) == 0 and f(2147483647, 4, 16, 2147483647, 2147483647) == 0


def test_the_scratch_stays_under_64_mib():
    lib = capi_run.lib()
    f, cap = lib.rc_scratch_bytes, 64 << 20
    worst = 0
    for h in [1 << k for k in range(12)]:                                                # planes from 1 x 1 to 2048^2 at the widest layer
        got = f(1, 192, 96, h, h)
        assert 0 < got <= cap, h
        worst = max(worst, got)
    assert f(2, 192, 96, 1500, 1500) == worst                                            # larger planes: the same partition count (2048^2 x 2 is refused)
    for Ci in range(4, 193, 4):                                                          # and every supported width, at a plane that reaches the cap
        for Co in range(16, 97, 16):
            got = f(1, Ci, Co, 512, 512)
            assert 0 < got <= cap and got == _formula(1, Ci, Co, 512, 512), (Ci, Co)


# D: a non-NULL, 16-byte aligned "pointer" that is never dereferenced: every call below must return before any HIP call
def _fwd(lib, x=D, w=D, bias=D, N=2, Ci=48, Co=48, H=16, W=16, y=D):
    return lib.rc_forward(x, w, bias, N, Ci, Co, H, W, y, None)


def _bwd(lib, x=D, w=D, dy=D, N=2, Ci=48, Co=48, H=16, W=16, dx=D, dw=D, dbias=D, scratch=D):
    return lib.rc_backward(x, w, dy, N, Ci, Co, H, W, dx, dw, dbias, scratch, None)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["forward", "backward"])
def test_bad_arguments_are_refused_before_hip(call):
    lib = capi_run.lib()
    assert call(lib, Ci=0) == E and call(lib, Ci=3) == E and call(lib, Ci=50) == E and call(lib, Ci=196) == E and call(lib, Ci=-4) == E
    assert call(lib, Co=0) == E and call(lib, Co=24) == E and call(lib, Co=112) == E and call(lib, Co=8) == E and call(lib, Co=-16) == E
    assert call(lib, N=0) == E and call(lib, N=-1) == E and call(lib, H=0) == E and call(lib, W=0) == E and call(lib, H=-16) == E
    assert call(lib, x=None) == E and call(lib, w=None) == E
    assert call(lib, x=D + 4) == E and call(lib, w=D + 2) == E                                     # misaligned
    assert call(lib, N=1, Ci=192, Co=16, H=4096, W=4096) == E                                      # x: more than 2^31 elements
    assert call(lib, N=8, Ci=16, Co=96, H=4096, W=4096) == E                                       # x: exactly 2^31 elements
    assert call(lib, N=4, Ci=4, Co=96, H=4096, W=4096) == E                                        # x fits (2^28), y: more than 2^31 elements
    assert call(lib, N=2, Ci=4, Co=16, H=16384, W=16384) == E                                      # x: exactly 2^31 elements
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
    assert _bwd(lib, dx=None, dw=None, dbias=None, scratch=None, Ci=192, Co=96, H=128, W=128) == 0
    assert _bwd(lib, dx=None, dw=None, dbias=None, scratch=None, Ci=6) == E                        # the arguments are still checked
    assert _bwd(lib, dx=None, dw=None, dbias=None, scratch=None, Co=40) == E
