"""CPU: the GroupNorm entry points of the C-ABI (include/gpsgs.h, last section) -- declared, exported, bound; the scratch formula the header states;
every bad-argument case refused before any HIP call (this machine has no GPU: a call that reached HIP would not return GPSGS_E_INVALID)."""
import pytest

from gps_gaussian_amd import _capi

import capi_run
from capi_run import D


def test_symbols_are_declared_exported_and_bound():
    lib = capi_run.check_section("gn_", _capi.GN_SYMBOLS, ["gn_backward", "gn_chunk_elems", "gn_forward", "gn_scratch_bytes"])
    assert len(lib.gn_forward.argtypes) == 14 and len(lib.gn_backward.argtypes) == 15


def _formula(K, N, Cn, G, HW):
    cdiv = lambda a, b: -(-a // b)
    return 8 * N * (Cn + max(cdiv(Cn * HW, K) + G, Cn * cdiv(HW, K)))


def test_chunk_and_the_scratch_formula():
    lib = capi_run.lib()
    K = lib.gn_chunk_elems()
    assert K > 0 and K % 8 == 0      # a chunk is whole 16-byte vectors of either dtype
    cdiv = lambda a, b: -(-a // b)
    shapes = [(2, 32, 8, 512 * 512), (2, 32, 4, 512 * 512), (2, 48, 6, 256 * 256), (2, 96, 12, 128 * 128), (8, 64, 8, 256 * 256), (3, 8, 1, 1),
              (2, 6, 2, 35), (1, 4, 2, K - 1), (1, 4, 2, K), (1, 4, 2, K + 1), (1, 6, 3, K // 2), (1, 6, 2, K // 2), (1, 1, 1, 1)]
    for N, Cn, G, HW in shapes:
        got = lib.gn_scratch_bytes(N, Cn, G, HW)
        assert got == _formula(K, N, Cn, G, HW), (N, Cn, G, HW)
        L = Cn // G * HW
        # room for the plane sums AND ceil(L / chunk) partials per row, resp. ceil(HW / chunk) per plane
        assert got >= 8 * (N * Cn + N * G * cdiv(L, K)) and got >= 8 * (N * Cn + N * Cn * cdiv(HW, K)), (N, Cn, G, HW)
    base = (2, 24, 2, K + 5)
    for k, bigger in enumerate([(3, 24, 2, K + 5), (2, 48, 2, K + 5), (2, 24, 2, 3 * K)]):
        assert lib.gn_scratch_bytes(*bigger) > lib.gn_scratch_bytes(*base), k
    assert lib.gn_scratch_bytes(2, 24, 3, K + 5) >= lib.gn_scratch_bytes(*base)
    assert lib.gn_scratch_bytes(1, 2, 2, K // 4) > lib.gn_scratch_bytes(1, 2, 1, K // 4)   # where the row partials decide, more groups = more bytes
    for G in range(1, 24):           # monotone in G even where G * ceil(L / chunk) itself is not (C = 6, HW = K / 2: 3, 4, 3 partials for G = 1, 2, 3)
        assert lib.gn_scratch_bytes(1, 6, G + 1, K // 2) >= lib.gn_scratch_bytes(1, 6, G, K // 2)
    for HW in range(1, 3 * K, 977):
        assert lib.gn_scratch_bytes(2, 8, 2, HW + 977) >= lib.gn_scratch_bytes(2, 8, 2, HW)
    assert lib.gn_scratch_bytes(-1, 8, 2, 16) == 0 and lib.gn_scratch_bytes(1, 8, 0, 16) == 0 and lib.gn_scratch_bytes(1, 8, 2, -16) == 0
    assert lib.gn_scratch_bytes(0, 8, 2, 16) == 0


# D: a non-NULL, 16-byte aligned "pointer" that is never dereferenced: every call below must return before any HIP call
def _fwd(lib, x=D, dtype=0, gamma=D, beta=D, N=2, Cn=8, G=2, HW=16, y=D, mean=D, rstd=D, scratch=D):
    return lib.gn_forward(x, dtype, gamma, beta, N, Cn, G, HW, 1e-5, y, mean, rstd, scratch, None)


def _bwd(lib, x=D, dtype=0, dy=D, gamma=D, mean=D, rstd=D, N=2, Cn=8, G=2, HW=16, dx=D, dgamma=D, dbeta=D, scratch=D):
    return lib.gn_backward(x, dtype, dy, gamma, mean, rstd, N, Cn, G, HW, dx, dgamma, dbeta, scratch, None)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["forward", "backward"])
def test_bad_arguments_are_refused_before_hip(call):
    lib = capi_run.lib()
    E = _capi.GPSGS_E_INVALID
    assert call(lib, G=0) == E and call(lib, G=-2) == E
    assert call(lib, G=3) == E                       # 8 % 3
    assert call(lib, dtype=2) == E and call(lib, dtype=-1) == E
    assert call(lib, N=-1) == E and call(lib, Cn=-8) == E and call(lib, HW=-1) == E
    assert call(lib, x=None) == E and call(lib, gamma=None) == E and call(lib, scratch=None) == E
    assert call(lib, x=D + 4) == E                   # not 16-byte aligned
    assert call(lib, Cn=2, G=1, HW=2 ** 30) == E     # a row of 2^31 elements
    if call is _fwd:
        assert call(lib, beta=None) == E and call(lib, y=None) == E and call(lib, mean=None) == E and call(lib, rstd=None) == E
        assert call(lib, y=D + 8) == E
    else:
        assert call(lib, dy=None) == E and call(lib, mean=None) == E and call(lib, rstd=None) == E
        assert call(lib, dgamma=None) == E and call(lib, dbeta=None) == E      # one without the other
        assert call(lib, dgamma=None, N=0) == E                               # ... even for an empty tensor
        assert call(lib, dy=D + 4) == E and call(lib, dx=D + 8) == E


def test_empty_tensors_return_ok_and_launch_nothing():
    lib = capi_run.lib()
    for kw in (dict(N=0), dict(Cn=0), dict(HW=0)):
        assert _fwd(lib, **kw) == 0 and _bwd(lib, **kw) == 0
        assert _fwd(lib, x=None, y=None, scratch=None, **kw) == 0              # torch hands out NULL for an empty tensor
        assert _bwd(lib, x=None, dy=None, dx=None, scratch=None, **kw) == 0
    assert _fwd(lib, N=0, G=0) == _capi.GPSGS_E_INVALID                        # the arguments are still checked
    # nothing asked for: no launch either (dx NULL, both parameter gradients NULL)
    assert _bwd(lib, dx=None, dgamma=None, dbeta=None) == 0
