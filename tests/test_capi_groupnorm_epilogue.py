"""CPU: the fused-epilogue GroupNorm entry points of the C-ABI (gne_forward / gne_backward, include/gpsgs.h, GroupNorm section) -- declared,
exported, bound; every bad-argument case refused before any HIP call (on a machine without a GPU a call that reached HIP would not return
GPSGS_E_INVALID); and the gn_* list still the four it was."""
import os

import pytest

from conftest import ROOT

from gps_gaussian_amd import _capi

import capi_run
from capi_run import D


def test_symbols_are_declared_exported_and_bound():
    lib = capi_run.check_section("gne_", _capi.GNE_SYMBOLS, ["gne_backward", "gne_forward"])
    assert len(lib.gne_forward.argtypes) == 15 and len(lib.gne_backward.argtypes) == 18
    # the plain entry points are what they were
    assert _capi.GN_SYMBOLS == ("gn_chunk_elems", "gn_scratch_bytes", "gn_forward", "gn_backward")
    assert capi_run.declared("gn_") == sorted(_capi.GN_SYMBOLS)
    assert len(lib.gn_forward.argtypes) == 14 and len(lib.gn_backward.argtypes) == 15
    # and build() checks the new ones
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_capi.GNE_SYMBOLS" in entry


# D: a non-NULL, 16-byte aligned "pointer" that is never dereferenced: every call below must return before any HIP call
def _fwd(lib, x=D, dtype=0, gamma=D, beta=D, residual=D, N=2, Cn=8, G=2, HW=16, out=D, mean=D, rstd=D, scratch=D):
    return lib.gne_forward(x, dtype, gamma, beta, residual, N, Cn, G, HW, 1e-5, out, mean, rstd, scratch, None)


def _bwd(lib, x=D, dtype=0, dout=D, out=D, gamma=D, beta=D, mean=D, rstd=D, N=2, Cn=8, G=2, HW=16, dx=D, dres=D, dgamma=D, dbeta=D, scratch=D):
    return lib.gne_backward(x, dtype, dout, out, gamma, beta, mean, rstd, N, Cn, G, HW, dx, dres, dgamma, dbeta, scratch, None)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["forward", "backward"])
@pytest.mark.parametrize("residual_form", [True, False], ids=["relu_add_relu", "relu"])
def test_bad_arguments_are_refused_before_hip(call, residual_form):
    lib = capi_run.lib()
    E = _capi.GPSGS_E_INVALID
    form = {} if residual_form else (dict(residual=None) if call is _fwd else dict(out=None, dres=None))
    bad = lambda **kw: call(lib, **dict(form, **kw))
    assert bad(G=0) == E and bad(G=-2) == E
    assert bad(G=3) == E                       # 8 % 3
    assert bad(dtype=2) == E and bad(dtype=-1) == E
    assert bad(N=-1) == E and bad(Cn=-8) == E and bad(HW=-1) == E
    assert bad(x=None) == E and bad(gamma=None) == E and bad(beta=None) == E and bad(scratch=None) == E
    assert bad(mean=None) == E and bad(rstd=None) == E
    assert bad(x=D + 4) == E and bad(scratch=D + 4) == E       # not 16-byte / 8-byte aligned
    assert bad(Cn=2, G=1, HW=2 ** 30) == E                     # a row of 2^31 elements
    if call is _fwd:
        assert bad(out=None) == E and bad(out=D + 8) == E
        if residual_form:
            assert bad(residual=D + 4) == E
    else:
        assert bad(dout=None) == E and bad(dout=D + 4) == E and bad(dx=D + 8) == E
        assert bad(dgamma=None) == E and bad(dbeta=None) == E      # one without the other
        assert bad(dgamma=None, N=0) == E                           # ... even for an empty tensor
        if residual_form:
            assert bad(out=D + 4) == E and bad(dres=D + 8) == E
        assert call(lib, out=None, dres=D) == E                     # dres without out
        assert call(lib, out=None, dres=D, N=0) == E                # ... even for an empty tensor


def test_empty_tensors_return_ok_and_launch_nothing():
    lib = capi_run.lib()
    for kw in (dict(N=0), dict(Cn=0), dict(HW=0)):
        assert _fwd(lib, **kw) == 0 and _bwd(lib, **kw) == 0
        assert _fwd(lib, x=None, residual=None, out=None, scratch=None, **kw) == 0        # torch hands out NULL for an empty tensor
        assert _bwd(lib, x=None, dout=None, out=None, dx=None, dres=None, scratch=None, **kw) == 0
    assert _fwd(lib, N=0, G=0) == _capi.GPSGS_E_INVALID                                   # the arguments are still checked
    # nothing asked for: no launch either
    assert _bwd(lib, dx=None, dres=None, dgamma=None, dbeta=None) == 0
    assert _bwd(lib, out=None, dx=None, dres=None, dgamma=None, dbeta=None) == 0
