"""CPU: the Gaussian-head entry points of the C-ABI (include/gpsgs.h, gsr_head_*) -- declared, exported, bound in the core table; the
configurations gsr_head_supported takes; the scratch formula the header states; every bad-argument case refused before any HIP call (this machine
has no GPU: a call that reached HIP would not return GPSGS_E_INVALID)."""
import ctypes as C

import pytest

from gps_gaussian_amd import _capi

import capi_run
from capi_run import D

NAMES = ["gsr_head_backward", "gsr_head_forward", "gsr_head_scratch_bytes", "gsr_head_supported", "gsr_head_tile"]


def test_symbols_are_declared_exported_and_bound():
    # the core table: no tuple of their own, no new prefix
    lib = capi_run.check_section("gsr_head_", [n for n in _capi.SYMBOLS if n.startswith("gsr_head_")], NAMES)
    assert not set(NAMES) & set(_capi.GN_SYMBOLS + _capi.GNE_SYMBOLS + _capi.SC_SYMBOLS)
    assert len(lib.gsr_head_forward.argtypes) == 13 and len(lib.gsr_head_backward.argtypes) == 18
    assert lib.gsr_head_scratch_bytes.restype is C.c_size_t


def test_supported_is_exactly_the_table():
    lib = capi_run.lib()
    for Ci in range(-1, 130):
        for K in range(-1, 8):
            for act in range(-1, 5):
                want = int(Ci in (16, 32, 64) and 1 <= K <= 4 and act in (0, 1, 2))
                assert lib.gsr_head_supported(Ci, K, act) == want, (Ci, K, act)


def _formula(T, N, Ci, K, H, W):
    parts = N * -(-(H * W) // T)
    return 4 * K * (Ci + 1) * (parts + -(-parts // 64))


def test_tile_and_the_scratch_formula():
    lib = capi_run.lib()
    T = lib.gsr_head_tile()
    assert T > 0 and T % 256 == 0
    f = lib.gsr_head_scratch_bytes
    for N, Ci, K, H, W in [(2, 32, 4, 1024, 1024), (8, 32, 3, 1024, 1024), (2, 32, 1, 1024, 1024), (1, 16, 1, 1, 1), (2, 32, 4, 5, 7), (1, 32, 2, 1, T - 1),
                           (1, 32, 2, 1, T), (1, 32, 2, 1, T + 1), (3, 16, 3, 9, 257), (2, 64, 4, 17, 64), (64, 16, 2, 1, 8), (65, 16, 2, 1, 8),
                           (1, 64, 4, 1, 65 * T)]:
        assert f(N, Ci, K, H, W) == _formula(T, N, Ci, K, H, W) > 0, (N, Ci, K, H, W)
    # monotone in N * H * W
    prev = 0
    for n in range(1, 200, 7):
        assert f(n, 32, 4, 30, 30) >= prev
        prev = f(n, 32, 4, 30, 30)
    prev = 0
    for hw in range(1, 12 * T, 97):
        assert f(2, 32, 3, 1, hw) >= prev and f(2, 32, 3, hw, 1) == f(2, 32, 3, 1, hw)
        prev = f(2, 32, 3, 1, hw)
    assert f(3, 32, 4, 100, 100) > f(2, 32, 4, 100, 100) and f(2, 32, 4, 200, 100) > f(2, 32, 4, 100, 100)
    # refused arguments: 0
    assert f(0, 32, 4, 16, 16) == 0 and f(-1, 32, 4, 16, 16) == 0 and f(2, 32, 4, 0, 16) == 0 and f(2, 32, 4, 16, -4) == 0
    assert f(2, 24, 4, 16, 16) == 0 and f(2, 32, 5, 16, 16) == 0 and f(2, 32, 0, 16, 16) == 0
    assert f(1, 32, 4, 65536, 32768) == 0                         # H * W = 2^31
    assert f(1, 32, 4, 1, 2 ** 31 - 1 - T) > 0 and f(1, 32, 4, 1, 2 ** 31 - T) == 0          # the last plane size a pixel index (+ one tile) fits
    assert f(2 ** 31 - 1, 32, 4, 1, 1) > 0 and f(2 ** 31 - 1, 32, 4, 1, T + 1) == 0           # more workgroups than a grid is wide


# D: a non-NULL, aligned "pointer" that is never dereferenced: every call below must return before any HIP call
def _fwd(lib, h=D, w=D, bias=D, N=2, Ci=32, K=3, H=16, W=16, act=1, beta=100.0, threshold=20.0, y=D):
    return lib.gsr_head_forward(h, w, bias, N, Ci, K, H, W, act, beta, threshold, y, None)


def _bwd(lib, h=D, w=D, bias=D, y=None, dy=D, N=2, Ci=32, K=3, H=16, W=16, act=1, beta=100.0, threshold=20.0, dh=D, dw=D, dbias=D, scratch=D):
    return lib.gsr_head_backward(h, w, bias, y, dy, N, Ci, K, H, W, act, beta, threshold, dh, dw, dbias, scratch, None)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["forward", "backward"])
def test_bad_arguments_are_refused_before_hip(call):
    lib = capi_run.lib()
    E = _capi.GPSGS_E_INVALID
    T = lib.gsr_head_tile()
    assert call(lib, Ci=24) == E and call(lib, Ci=0) == E and call(lib, Ci=128) == E and call(lib, K=0) == E and call(lib, K=5) == E   # unsupported (C, K)
    assert call(lib, act=3) == E and call(lib, act=-1) == E
    assert call(lib, N=0) == E and call(lib, N=-1) == E and call(lib, H=0) == E and call(lib, W=0) == E and call(lib, H=-16) == E
    assert call(lib, beta=0.0) == E and call(lib, beta=-1.0) == E and call(lib, beta=float("nan")) == E                                 # softplus needs beta > 0
    assert call(lib, h=None) == E and call(lib, w=None) == E and call(lib, bias=None) == E
    assert call(lib, h=D + 2) == E and call(lib, w=D + 1) == E                                                                         # off a 4-byte boundary
    assert call(lib, N=1, H=65536, W=32768) == E and call(lib, N=1, H=1, W=2 ** 31 - T) == E                                            # the plane index
    assert call(lib, N=2 ** 31 - 1, H=1, W=T + 1) == E                                                                                  # the grid
    if call is _fwd:
        assert call(lib, y=None) == E and call(lib, y=D + 2) == E
    else:
        assert call(lib, dy=None) == E and call(lib, scratch=None) == E
        assert call(lib, dw=None) == E and call(lib, dbias=None) == E                              # one without the other
        assert call(lib, dy=D + 2) == E and call(lib, dh=D + 1) == E and call(lib, dw=D + 2) == E and call(lib, scratch=D + 3) == E


def test_beta_is_read_for_softplus_only_and_nothing_asked_for_launches_nothing():
    lib = capi_run.lib()
    E = _capi.GPSGS_E_INVALID
    none = dict(dh=None, dw=None, dbias=None, scratch=None)
    assert _bwd(lib, **none) == 0                                                                   # neither gradient wanted: GPSGS_OK, no launch
    assert _bwd(lib, act=0, beta=0.0, **none) == 0 and _bwd(lib, act=2, beta=-3.0, **none) == 0     # beta belongs to softplus
    assert _bwd(lib, beta=0.0, **none) == E and _bwd(lib, K=5, **none) == E                         # the arguments are still checked
    assert _bwd(lib, y=D, **none) == 0 and _bwd(lib, y=None, **none) == 0                           # y is not read: NULL is fine
