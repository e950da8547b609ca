"""CPU: the Gaussian-head entry points of the C-ABI (include/gpsgs.h, gsr_head_*) -- declared, exported, bound in the core table; the
configurations gsr_head_supported takes; the scratch formula the header states; every bad-argument case refused before any HIP call (this machine
has no GPU: a call that reached HIP would not return GPSGS_E_INVALID)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

import gps_gaussian_amd  # noqa: F401
from gps_gaussian_amd import _capi

NAMES = ["gsr_head_backward", "gsr_head_forward", "gsr_head_scratch_bytes", "gsr_head_supported", "gsr_head_tile"]


def _lib():
    gps_gaussian_amd.build()
    return _capi.lib()


def test_symbols_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "gpsgs.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(?:int|size_t)\s+(gsr_head_[a-z0-9_]+)\s*\(", code)))
    assert declared == NAMES
    assert all(n in _capi.SYMBOLS for n in NAMES)                                       # the core table: no fifth tuple, no new prefix
    assert not set(NAMES) & set(_capi.GN_SYMBOLS + _capi.GNE_SYMBOLS + _capi.SC_SYMBOLS)
    assert "gsr_head_forward / gsr_head_backward" in src.split("#ifndef GPSGS_H")[0]   # the list at the top of the header names them
    lib = _lib()
    raw = C.CDLL(_capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == _capi.PROTOTYPES[name][1] and getattr(lib, name).restype is _capi.PROTOTYPES[name][0]
    assert len(lib.gsr_head_forward.argtypes) == 13 and len(lib.gsr_head_backward.argtypes) == 18
    assert lib.gsr_head_scratch_bytes.restype is C.c_size_t
    assert lib.gpsgs_abi_version() == 4


def test_supported_is_exactly_the_table():
    lib = _lib()
    for Ci in range(-1, 130):
        for K in range(-1, 8):
            for act in range(-1, 5):
                want = int(Ci in (16, 32, 64) and 1 <= K <= 4 and act in (0, 1, 2))
                assert lib.gsr_head_supported(Ci, K, act) == want, (Ci, K, act)


def _formula(T, N, Ci, K, H, W):
    parts = N * -(-(H * W) // T)
    return 4 * K * (Ci + 1) * (parts + -(-parts // 64))


def test_tile_and_the_scratch_formula():
    lib = _lib()
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


P = 0x10000   # a non-NULL, aligned "pointer" that is never dereferenced: every call below must return before any HIP call


def _fwd(lib, h=P, w=P, bias=P, N=2, Ci=32, K=3, H=16, W=16, act=1, beta=100.0, threshold=20.0, y=P):
    return lib.gsr_head_forward(h, w, bias, N, Ci, K, H, W, act, beta, threshold, y, None)


def _bwd(lib, h=P, w=P, bias=P, y=None, dy=P, N=2, Ci=32, K=3, H=16, W=16, act=1, beta=100.0, threshold=20.0, dh=P, dw=P, dbias=P, scratch=P):
    return lib.gsr_head_backward(h, w, bias, y, dy, N, Ci, K, H, W, act, beta, threshold, dh, dw, dbias, scratch, None)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["forward", "backward"])
def test_bad_arguments_are_refused_before_hip(call):
    lib = _lib()
    E = _capi.GPSGS_E_INVALID
    T = lib.gsr_head_tile()
    assert call(lib, Ci=24) == E and call(lib, Ci=0) == E and call(lib, Ci=128) == E and call(lib, K=0) == E and call(lib, K=5) == E   # unsupported (C, K)
    assert call(lib, act=3) == E and call(lib, act=-1) == E
    assert call(lib, N=0) == E and call(lib, N=-1) == E and call(lib, H=0) == E and call(lib, W=0) == E and call(lib, H=-16) == E
    assert call(lib, beta=0.0) == E and call(lib, beta=-1.0) == E and call(lib, beta=float("nan")) == E                                 # softplus needs beta > 0
    assert call(lib, h=None) == E and call(lib, w=None) == E and call(lib, bias=None) == E
    assert call(lib, h=P + 2) == E and call(lib, w=P + 1) == E                                                                         # off a 4-byte boundary
    assert call(lib, N=1, H=65536, W=32768) == E and call(lib, N=1, H=1, W=2 ** 31 - T) == E                                            # the plane index
    assert call(lib, N=2 ** 31 - 1, H=1, W=T + 1) == E                                                                                  # the grid
    if call is _fwd:
        assert call(lib, y=None) == E and call(lib, y=P + 2) == E
    else:
        assert call(lib, dy=None) == E and call(lib, scratch=None) == E
        assert call(lib, dw=None) == E and call(lib, dbias=None) == E                              # one without the other
        assert call(lib, dy=P + 2) == E and call(lib, dh=P + 1) == E and call(lib, dw=P + 2) == E and call(lib, scratch=P + 3) == E


def test_beta_is_read_for_softplus_only_and_nothing_asked_for_launches_nothing():
    lib = _lib()
    E = _capi.GPSGS_E_INVALID
    none = dict(dh=None, dw=None, dbias=None, scratch=None)
    assert _bwd(lib, **none) == 0                                                                   # neither gradient wanted: GPSGS_OK, no launch
    assert _bwd(lib, act=0, beta=0.0, **none) == 0 and _bwd(lib, act=2, beta=-3.0, **none) == 0     # beta belongs to softplus
    assert _bwd(lib, beta=0.0, **none) == E and _bwd(lib, K=5, **none) == E                         # the arguments are still checked
    assert _bwd(lib, y=P, **none) == 0 and _bwd(lib, y=None, **none) == 0                           # y is not read: NULL is fine
