"""CPU: the decoder-glue entry points of the C-ABI (include/gpsgs.h, last section) -- declared, exported, bound; what uc_supported takes; the tile;
every bad-argument case refused before any HIP call (this machine has no GPU: a call that reached HIP would not return GPSGS_E_INVALID); a backward
that is asked for nothing launches nothing."""
import ctypes as C

import pytest

from gps_gaussian_amd import _capi
from gps_gaussian_amd import upcat

import capi_run
from capi_run import D

NAMES = ["uc_backward", "uc_forward", "uc_supported", "uc_tile"]
E = _capi.GPSGS_E_INVALID


def _ints(v):
    return None if v is None else (C.c_int * len(v))(*v)


def _ptrs(v):
    return None if v is None else (C.c_void_p * len(v))(*v)


def test_symbols_are_declared_exported_and_bound():
    lib = capi_run.check_section("uc_", _capi.UC_SYMBOLS, NAMES)
    for name in NAMES:
        assert capi_run.declared_arg_count(name) == len(_capi.PROTOTYPES[name][1]), name
    assert len(lib.uc_forward.argtypes) == 10 and len(lib.uc_backward.argtypes) == 9
    assert _capi.SECTIONS[-1] == _capi.UC_SYMBOLS
    assert not set(_capi.UC_SYMBOLS) & set(sum(_capi.SECTIONS[:-1], ()))


def test_supported_and_tile():
    lib = capi_run.lib()
    assert lib.uc_supported(0, None) == 1 and lib.uc_supported(0, _ints([5])) == 1
    assert lib.uc_supported(1, _ints([1])) == 1 and lib.uc_supported(2, _ints([3, 1])) == 1 and lib.uc_supported(3, _ints([48, 48, 7])) == 1
    assert lib.uc_supported(-1, None) == 0 and lib.uc_supported(4, _ints([1, 1, 1, 1])) == 0 and lib.uc_supported(1, None) == 0
    assert lib.uc_supported(1, _ints([0])) == 0 and lib.uc_supported(3, _ints([1, -2, 1])) == 0 and lib.uc_supported(2, _ints([1, 0])) == 0
    a, b = C.c_int(0), C.c_int(0)
    assert lib.uc_tile(None, None) == E and lib.uc_tile(C.byref(a), None) == E and lib.uc_tile(None, C.byref(b)) == E
    assert lib.uc_tile(C.byref(a), C.byref(b)) == 0
    TH, TW = upcat.tile()
    assert (a.value, b.value) == (TH, TW) and TH >= 4 and TH % 2 == 0 and TW >= 8 and TW % 4 == 0


# D: a non-NULL, 16-byte aligned "pointer" that is never dereferenced: every call below must return before any HIP call
def _fwd(lib, a=D, skips=(D, D), channels=(3, 1), K=None, N=2, Ca=4, h=8, w=8, out=D):
    return lib.uc_forward(a, _ptrs(skips), _ints(channels), len(channels) if K is None else K, N, Ca, h, w, out, None)


def _bwd(lib, dout=D, channels=(3, 1), K=None, N=2, Ca=4, h=8, w=8, da=D, **ignored):
    return lib.uc_backward(dout, _ints(channels), len(channels) if K is None else K, N, Ca, h, w, da, None)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["forward", "backward"])
def test_bad_arguments_are_refused_before_hip(call):
    lib = capi_run.lib()
    # non-positive sizes
    assert call(lib, N=0) == E and call(lib, N=-1) == E and call(lib, Ca=0) == E and call(lib, Ca=-4) == E
    assert call(lib, h=0) == E and call(lib, h=-8) == E and call(lib, w=0) == E and call(lib, w=-8) == E
    # K outside 0..3
    assert call(lib, K=-1) == E and call(lib, skips=(D,) * 4, channels=(1,) * 4) == E and call(lib, skips=(D,) * 4, channels=(1,) * 4, K=7) == E
    # a skip channel count below 1; no counts at all
    assert call(lib, channels=(3, 0)) == E and call(lib, channels=(-1, 1)) == E and call(lib, skips=(D,), channels=(0,)) == E
    assert call(lib, channels=None, K=2) == E
    # 2^31 elements or more: in out alone (a: 2^29), in out through a skip, in one plane, and sizes whose products leave 32 or 64 bits
    assert call(lib, N=4, Ca=2, h=8192, w=8192, skips=(), channels=()) == E               # out: 2^31
    assert call(lib, N=1, Ca=1, h=8192, w=8192, skips=(D,), channels=(7,)) == E           # out: 2^28 (1 + 7) = 2^31
    assert call(lib, N=1, Ca=1, h=32768, w=16384, skips=(), channels=()) == E             # one plane of out: 2^31
    assert call(lib, N=2147483647, Ca=2147483647, h=1, w=1, skips=(), channels=()) == E
    assert call(lib, N=1, Ca=1, h=2147483647, w=2147483647, skips=(), channels=()) == E
    assert call(lib, N=1, Ca=1, h=1, w=1, skips=(D, D, D), channels=(2147483647,) * 3) == E
    if call is _fwd:
        assert call(lib, a=None) == E and call(lib, out=None) == E and call(lib, skips=None) == E
        assert call(lib, skips=(D, None)) == E and call(lib, skips=(None, D)) == E
        assert call(lib, a=D + 2) == E and call(lib, out=D + 1) == E and call(lib, skips=(D, D + 2)) == E and call(lib, skips=(D + 3, D)) == E
    else:
        assert call(lib, dout=None) == E and call(lib, dout=D + 2) == E and call(lib, da=D + 2) == E and call(lib, dout=D + 1, da=None) == E


def test_the_largest_refused_size_is_the_limit_itself():
    """2^31 - 1 elements would pass the size check (and only then reach HIP): the check is at 2^31, not below.  Shown on the backward asked for
    nothing, which returns before any HIP call."""
    lib = capi_run.lib()
    assert _bwd(lib, N=1, Ca=1, h=8192, w=8192, channels=(6,), da=None) == 0               # out: 7 * 2^28 < 2^31
    assert _bwd(lib, N=1, Ca=1, h=8192, w=8192, channels=(7,), da=None) == E               # out: 2^31


def test_nothing_asked_for_launches_nothing():
    lib = capi_run.lib()
    assert _bwd(lib, da=None) == 0
    assert _bwd(lib, da=None, channels=(), K=0) == 0
    assert _bwd(lib, da=None, dout=D + 4) == 0                                             # 4-byte alignment is enough
    assert _bwd(lib, da=None, h=0) == E and _bwd(lib, da=None, channels=(0, 1)) == E       # the arguments are still checked
    assert _bwd(lib, da=None, dout=None) == E
