"""CPU: the stem-convolution entry points of the C-ABI (include/gpsgs.h, last section) -- declared, exported, bound; the configurations sc_supported
takes; the scratch formula the header states; every bad-argument case refused before any HIP call (this machine has no GPU: a call that reached HIP
would not return GPSGS_E_INVALID)."""
import pytest

from gps_gaussian_amd import _capi, _ops

import capi_run
from capi_run import D


def test_symbols_are_declared_exported_and_bound():
    lib = capi_run.check_section("sc_", _capi.SC_SYMBOLS, ["sc_backward", "sc_forward", "sc_scratch_bytes", "sc_supported", "sc_tile"])
    assert len(lib.sc_forward.argtypes) == 14 and len(lib.sc_backward.argtypes) == 17
    assert not set(_capi.SC_SYMBOLS) & set(_capi.SYMBOLS + _capi.GN_SYMBOLS + _capi.GNE_SYMBOLS)


def test_supported_is_exactly_the_table():
    lib = capi_run.lib()
    for Ci in (1, 3):
        for Co in range(8, 65, 8):
            assert lib.sc_supported(Ci, Co, 5, 2, 2) == 1, (Ci, Co)
    # the neighbours
    assert lib.sc_supported(3, 32, 3, 2, 2) == 0 and lib.sc_supported(3, 32, 3, 2, 1) == 0 and lib.sc_supported(3, 32, 7, 2, 3) == 0   # K
    assert lib.sc_supported(3, 32, 5, 1, 2) == 0 and lib.sc_supported(3, 32, 5, 3, 2) == 0                                            # stride
    assert lib.sc_supported(3, 32, 5, 2, 1) == 0 and lib.sc_supported(3, 32, 5, 2, 0) == 0 and lib.sc_supported(3, 32, 5, 2, 3) == 0   # pad
    for Ci in (0, 2, 4, -1):
        assert lib.sc_supported(Ci, 32, 5, 2, 2) == 0, Ci
    for Co in (0, 4, 12, 72, -8, 7, 9):
        assert lib.sc_supported(1, Co, 5, 2, 2) == 0 and lib.sc_supported(3, Co, 5, 2, 2) == 0, Co


def _tile(lib):
    return _ops.tile("sc_tile")


def _formula(TH, TW, N, Ci, Co, H, W, K=5, S=2, P=2):
    cdiv = lambda a, b: -(-a // b)
    Ho, Wo = (H + 2 * P - K) // S + 1, (W + 2 * P - K) // S + 1
    tiles = N * cdiv(Ho, TH) * cdiv(Wo, TW)
    return 4 * Co * (Ci * K * K + 1) * (tiles + cdiv(tiles, 64))


def test_tile_and_the_scratch_formula():
    lib = capi_run.lib()
    TH, TW = _tile(lib)
    assert TH > 0 and TW > 0
    assert lib.sc_tile(None, None) == _capi.GPSGS_E_INVALID
    shapes = [(2, 3, 32, 1024, 1024), (8, 1, 32, 1024, 1024), (2, 3, 32, 2048, 2048), (1, 1, 8, 1, 1), (3, 1, 64, 2, 3), (2, 3, 40, 5, 7),
              (1, 3, 32, 37, 41), (2, 3, 32, 2 * TH, 2 * TW), (2, 3, 32, 2 * TH + 1, 2 * TW + 1), (2, 1, 32, 2 * TH - 1, 2 * TW - 1),
              (65, 1, 8, 2 * TH, 2 * TW), (64, 1, 8, 2 * TH, 2 * TW)]          # 65 and 64 tiles: either side of the two-stage sum's group size
    for N, Ci, Co, H, W in shapes:
        got = lib.sc_scratch_bytes(N, Ci, Co, H, W, 5, 2, 2)
        assert got == _formula(TH, TW, N, Ci, Co, H, W) > 0, (N, Ci, Co, H, W)
    base = (2, 3, 32, 4 * TH + 3, 4 * TW + 3)
    f = lambda N, Ci, Co, H, W: lib.sc_scratch_bytes(N, Ci, Co, H, W, 5, 2, 2)
    assert f(3, 3, 32, base[3], base[4]) > f(*base) and f(2, 3, 32, base[3] + 2 * TH, base[4]) > f(*base) and f(2, 3, 32, base[3], base[4] + 2 * TW) > f(*base)
    for n in range(1, 200, 7):
        assert f(n + 7, 1, 8, 30, 30) >= f(n, 1, 8, 30, 30)
    for h in range(1, 12 * TH, 5):
        assert f(2, 3, 32, h + 5, 77) >= f(2, 3, 32, h, 77) and f(2, 3, 32, 77, 3 * h + 15) >= f(2, 3, 32, 77, 3 * h)
    # bad arguments: 0
    assert f(0, 3, 32, 16, 16) == 0 and f(-1, 3, 32, 16, 16) == 0 and f(2, 3, 32, 0, 16) == 0 and f(2, 3, 32, 16, -4) == 0
    assert f(2, 2, 32, 16, 16) == 0 and f(2, 3, 12, 16, 16) == 0
    assert lib.sc_scratch_bytes(2, 3, 32, 16, 16, 3, 2, 2) == 0 and lib.sc_scratch_bytes(2, 3, 32, 16, 16, 5, 1, 2) == 0
    assert lib.sc_scratch_bytes(2, 3, 32, 16, 16, 5, 2, 1) == 0
    assert f(8, 3, 32, 8192, 16384) == 0                                    # 2^31 elements or more


# D: a non-NULL, 16-byte aligned "pointer" that is never dereferenced: every call below must return before any HIP call
def _fwd(lib, x=D, w=D, bias=D, N=2, Ci=3, Co=32, H=16, W=16, K=5, stride=2, pad=2, y=D, dtype=0):
    return lib.sc_forward(x, w, bias, N, Ci, Co, H, W, K, stride, pad, y, dtype, None)


def _bwd(lib, x=D, w=D, dy=D, dtype=0, N=2, Ci=3, Co=32, H=16, W=16, K=5, stride=2, pad=2, dx=D, dw=D, dbias=D, scratch=D):
    return lib.sc_backward(x, w, dy, dtype, N, Ci, Co, H, W, K, stride, pad, dx, dw, dbias, scratch, None)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["forward", "backward"])
def test_bad_arguments_are_refused_before_hip(call):
    lib = capi_run.lib()
    E = _capi.GPSGS_E_INVALID
    assert call(lib, K=3) == E and call(lib, stride=1) == E and call(lib, pad=1) == E               # unsupported configurations
    assert call(lib, Ci=2) == E and call(lib, Ci=4) == E and call(lib, Co=4) == E and call(lib, Co=12) == E and call(lib, Co=72) == E
    assert call(lib, N=0) == E and call(lib, N=-1) == E and call(lib, H=0) == E and call(lib, W=0) == E and call(lib, H=-16) == E
    assert call(lib, dtype=2) == E and call(lib, dtype=-1) == E
    assert call(lib, x=None) == E and call(lib, w=None) == E
    assert call(lib, x=D + 4) == E and call(lib, w=D + 2) == E                                     # misaligned
    assert call(lib, N=8, Ci=3, H=8192, W=16384) == E                                              # x: 3 * 2^30 elements
    assert call(lib, N=8, Ci=1, Co=64, H=8192, W=8192) == E                                        # x fits (2^29), y: 2^33 elements
    if call is _fwd:
        assert call(lib, bias=None) == E and call(lib, y=None) == E
        assert call(lib, y=D + 8) == E and call(lib, bias=D + 1) == E
    else:
        assert call(lib, dy=None) == E and call(lib, scratch=None) == E
        assert call(lib, dw=None) == E and call(lib, dbias=None) == E                              # one without the other
        assert call(lib, dy=D + 4) == E and call(lib, dx=D + 8) == E and call(lib, dw=D + 2) == E and call(lib, scratch=D + 8) == E


def test_nothing_asked_for_launches_nothing():
    lib = capi_run.lib()
    assert _bwd(lib, dx=None, dw=None, dbias=None, scratch=None) == 0
    assert _bwd(lib, dx=None, dw=None, dbias=None, scratch=None, K=3) == _capi.GPSGS_E_INVALID     # the arguments are still checked
