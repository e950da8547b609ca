"""CPU: the entry points of the 1-D correlation sampler (cs_forward / cs_backward) and the fused multi-level lookup (cs_lookup_forward /
cs_lookup_backward) of the C-ABI (include/gpsgs.h): every bad-argument case is refused before any HIP call (this machine has no GPU: a call that
reached HIP would return neither GPSGS_E_INVALID nor GPSGS_OK), empty tensors return without a launch, and sizes the kernels or a launch cannot
hold -- more (n, y, x) rows than an int counts, a block count beyond 0x7fffffff, a radius whose 2 r + 1 overflows -- are refused instead of
truncated."""
import ctypes as C

import pytest

from gps_gaussian_amd import _capi

import capi_run
from capi_run import D

# D: a non-NULL, 16-byte aligned "pointer" that is never dereferenced: every call below must return before any HIP call
E = _capi.GPSGS_E_INVALID
OK = 0
I31 = 2 ** 31 - 1


def _levels(ptrs):
    return None if ptrs is None else (C.c_void_p * 4)(*ptrs)


def _sfwd(lib, volume=D, coords=D, out=D, N=2, H1=3, W1=5, W2=8, r=4, dtype=0, **_):
    return lib.cs_forward(volume, coords, out, N, H1, W1, W2, r, dtype, None)


def _sbwd(lib, coords=D, gout=D, gvol=D, N=2, H1=3, W1=5, W2=8, r=4, dtype=0, **_):
    return lib.cs_backward(coords, gout, gvol, N, H1, W1, W2, r, dtype, None)


def _lfwd(lib, pyr=(D, D, D, D), coords=D, out=D, N=2, H1=3, W1=5, W2=8, levels=4, r=4, dtype=0, **_):
    return lib.cs_lookup_forward(_levels(pyr), coords, out, N, H1, W1, W2, levels, r, dtype, None)


def _lbwd(lib, coords=D, gout=D, pyr=(D, D, D, D), N=2, H1=3, W1=5, W2=8, levels=4, r=4, dtype=0, **_):
    return lib.cs_lookup_backward(coords, gout, _levels(pyr), N, H1, W1, W2, levels, r, dtype, None)


CALLS = [_sfwd, _sbwd, _lfwd, _lbwd]
IDS = ["cs_forward", "cs_backward", "cs_lookup_forward", "cs_lookup_backward"]
# no call below may get as far as a launch (the pointers are fake): every one is either refused (E) or empty (OK)


@pytest.mark.parametrize("call", CALLS, ids=IDS)
def test_bad_arguments_are_refused_before_hip(call):
    lib = capi_run.lib()
    assert call(lib, N=-1) == E and call(lib, H1=-3) == E and call(lib, W1=-5) == E and call(lib, W2=-8) == E
    assert call(lib, dtype=2) == E and call(lib, dtype=-1) == E
    assert call(lib, r=-1) == E and call(lib, r=-2 ** 31) == E
    assert call(lib, coords=None) == E
    if call in (_sfwd, _lfwd):
        assert call(lib, out=None) == E
    else:
        assert call(lib, gout=None) == E
    if call is _sfwd:
        assert call(lib, volume=None) == E
    if call is _sbwd:
        assert call(lib, gvol=None) == E
    if call in (_lfwd, _lbwd):
        assert call(lib, levels=0) == E and call(lib, levels=5) == E and call(lib, levels=-1) == E
        assert call(lib, pyr=None) == E
    # the arguments are still checked when the tensors are empty
    for empty in (dict(N=0), dict(H1=0), dict(W1=0)):
        assert call(lib, r=-1, **empty) == E and call(lib, dtype=2, **empty) == E and call(lib, W2=-1, **empty) == E
        if call in (_lfwd, _lbwd):
            assert call(lib, levels=0, **empty) == E and call(lib, levels=5, **empty) == E


@pytest.mark.parametrize("call", CALLS, ids=IDS)
def test_empty_tensors_return_ok_with_null_pointers(call):
    lib = capi_run.lib()
    null = dict(volume=None, coords=None, out=None, gout=None, gvol=None, pyr=(None, None, None, None))
    for empty in (dict(N=0), dict(H1=0), dict(W1=0), dict(N=0, H1=0, W1=0, W2=0)):
        assert call(lib, **empty) == OK, empty
        assert call(lib, **dict(null, **empty)) == OK, empty          # torch hands out NULL for an empty tensor
        assert call(lib, **dict(null, r=0, **empty)) == OK
    if call in (_sbwd, _lbwd):
        assert call(lib, **dict(null, W2=0)) == OK                    # no gradient element to write
    # huge sizes next to an empty one: nothing to index, nothing to launch
    assert call(lib, N=0, H1=I31, W1=I31, W2=I31) == OK and call(lib, N=I31, H1=I31, W1=0, W2=I31) == OK


@pytest.mark.parametrize("call", [_lfwd, _lbwd], ids=IDS[2:])
def test_null_level_is_accepted_exactly_where_the_level_is_empty(call):
    """W2 >> l == 0: the level has no element and torch hands out NULL for it.  Here: a NULL at every level that HAS elements is refused.  A call
    that passes this check goes on to launch, so the accepting side runs on the GPU with real buffers
    (tests/test_gpu_corr_lookup_edges.py::test_capi_null_pointers_of_empty_levels_are_accepted)."""
    lib = capi_run.lib()
    for W2 in (1, 2, 3, 4, 7, 8, 9):
        for levels in (1, 2, 3, 4):
            for l in range(levels):
                ptrs = [D] * 4
                ptrs[l] = None
                if (W2 >> l) > 0:
                    assert call(lib, pyr=tuple(ptrs), W2=W2, levels=levels) == E, (W2, levels, l)
    # levels beyond `levels` are never looked at
    assert call(lib, pyr=(D, None, None, None), N=0, levels=1) == OK


@pytest.mark.parametrize("call", CALLS, ids=IDS)
def test_more_rows_than_an_int_counts_are_refused(call):
    lib = capi_run.lib()
    assert call(lib, N=2, H1=2 ** 15, W1=2 ** 15) == E                # N*H1*W1 = 2^31
    assert call(lib, N=1, H1=2 ** 16, W1=2 ** 16) == E                # 2^32: an int product would wrap to 0
    assert call(lib, N=I31, H1=I31, W1=I31) == E                      # a product that does not fit 64 bits either
    assert call(lib, N=I31, H1=I31, W1=I31, W2=I31) == E
    assert call(lib, N=2 ** 16, H1=2 ** 16, W1=2 ** 16, W2=2 ** 16) == E   # 2^64 elements: the size_t product used to wrap to 0 and return OK
    assert call(lib, N=2 ** 11, H1=2 ** 11, W1=2 ** 11, W2=1) == E    # 2^33 rows


@pytest.mark.parametrize("call", [_sbwd, _lbwd], ids=[IDS[1], IDS[3]])
def test_backward_block_counts_beyond_a_grid_are_refused(call):
    """One thread per gradient element (per quad: k_cs_bwd4) in blocks of 256; the count used to be cast to unsigned."""
    lib = capi_run.lib()
    # 2^30 rows x 2^11 columns = 2^41 elements -> 2^33 blocks (the cast kept none of them); as quads 2^31 blocks
    assert call(lib, N=2 ** 10, H1=2 ** 10, W1=2 ** 10, W2=2 ** 11) == E
    # I31 rows x 513 columns (odd: the scalar kernel in both): 2^31 + 2^23 + ... blocks (the cast kept a few million)
    assert call(lib, N=1, H1=1, W1=I31, W2=513) == E
    assert call(lib, N=1, H1=I31, W1=1, W2=I31) == E
    if call is _lbwd:
        # 2^30 x 2^10 = 2^40 elements = 2^32 blocks of single elements: the lookup has no quad kernel
        assert call(lib, N=2 ** 10, H1=2 ** 10, W1=2 ** 10, W2=2 ** 10) == E
    else:
        # quads are counted where W2 % 4 == 0 and the pointer is 16-byte aligned: 2^30 x 2^11 / 4 = 2^39 quads = 2^31 blocks, one too many ...
        assert call(lib, N=2 ** 10, H1=2 ** 10, W1=2 ** 10, W2=2 ** 11) == E
        # ... and the same elements through a misaligned pointer are 2^33 blocks of the scalar kernel
        assert call(lib, gvol=D + 4, N=2 ** 10, H1=2 ** 10, W1=2 ** 10, W2=2 ** 11) == E
        # 2^40 elements: 2^30 blocks of quads would fit, 2^32 blocks of the scalar kernel (misaligned pointer) do not
        assert call(lib, gvol=D + 4, N=2 ** 10, H1=2 ** 10, W1=2 ** 10, W2=2 ** 10) == E


@pytest.mark.parametrize("call", CALLS, ids=IDS)
def test_a_radius_whose_window_overflows_an_int_is_refused(call):
    lib = capi_run.lib()
    assert call(lib, r=2 ** 30) == E and call(lib, r=I31) == E        # 2 r + 1 = 2^31 + 1
    assert call(lib, r=2 ** 30, N=0) == E                             # checked before the empty return
    assert call(lib, r=2 ** 30 - 1, N=0) == OK                        # 2 r + 1 = INT_MAX: the largest radius there is
