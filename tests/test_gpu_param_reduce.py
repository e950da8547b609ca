"""GPU (-m gpu): the parameter gradients of the stem convolution, the Gaussian heads and the 3x3 convolution are THE ordered sums the documentation
promises -- the workgroups' partials added in index order from 0.f, in groups of G (64, 64, 32) and then the groups in index order -- bit for bit.

Each case calls the C-ABI backward directly (dx = NULL; dw, dbias and scratch given) on seeded normal data, so every add rounds, then reads the
scratch back: partials [parts][M], then (where parts > G) the group sums [ceil(parts / G)][M] (include/gpsgs.h).  The same adds are made on the host
as a loop over float32 arrays and compared with np.array_equal on the uint32 views.  The scratch is filled with 0xFF bytes (NaN) before the call, so
a partial that was never written cannot pass.  No ATen convolution runs on the GPU here.  The other GPU tests of these ops bound the error for any
order and demand exact answers on integers, which any order gives: a changed group size or a swapped pair of loop bounds fails only here."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import gps_gaussian_amd  # noqa: F401
from gps_gaussian_amd import _capi
from gps_gaussian_amd._ops import call, ptr

pytestmark = pytest.mark.gpu
GROUP = {"heads": 64, "stem": 64, "c3": 32}      # partials per first-stage group: each op's own constant, as tests/test_capi_* hardcode them
C3_PARTS, C3_WTILE = 512, (4, 32)                 # the 3x3 weight gradient: workgroups at most, and the pixel tile one of them walks
ACT = {"none": 0, "softplus": 1, "sigmoid": 2}


def _cdiv(a, b):
    return -(-a // b)


def _tile2(name):
    th, tw = C.c_int(0), C.c_int(0)
    assert getattr(_capi.lib(), name)(C.byref(th), C.byref(tw)) == 0
    return th.value, tw.value


def _randn(gen, *shape, dtype=torch.float32):
    return torch.randn(shape, generator=gen).to(device="cuda", dtype=dtype)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ordered_sum(rows):
    """The fp32 running sum rows[0] + rows[1] + ... from zeros, one rounding per add, as the kernel makes it."""
    s = np.zeros(rows.shape[1], dtype=np.float32)
    for t in range(rows.shape[0]):
        s = s + rows[t]
    return s


def _check(op, parts, want_parts, M, nbytes, backward):
    """`backward(scratch)` makes the call and returns (dw, db), flat fp32 tensors of MW and M - MW elements."""
    G = GROUP[op]
    groups = _cdiv(parts, G)
    assert parts == want_parts, "the tile changed: this is no longer the case it was written as"
    assert nbytes == 4 * M * (parts + groups)
    scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda").view(torch.float32)
    dw, db = backward(scratch)
    torch.cuda.synchronize()
    s = scratch.cpu().numpy()
    got = np.concatenate([dw.cpu().numpy().ravel(), db.cpu().numpy().ravel()])
    assert got.shape == (M,)
    P = s[: parts * M].reshape(parts, M)
    assert np.isfinite(P).all(), "a partial was not written (or is not finite)"
    if parts <= G:
        assert np.array_equal(_bits(got), _bits(_ordered_sum(P)))
        return
    S = s[parts * M: (parts + groups) * M].reshape(groups, M)
    want = np.stack([_ordered_sum(P[g * G: min(parts, (g + 1) * G)]) for g in range(groups)])
    assert np.array_equal(_bits(S), _bits(want)), "the group sums"
    assert np.array_equal(_bits(got), _bits(_ordered_sum(S))), "the sum of the group sums"


HEADS = {"3_parts": (1, 32, 3, 1, None, "none", 3), "64+1": (65, 64, 4, 1, 8, "sigmoid", 65), "64+64+1": (129, 16, 1, 1, 8, "softplus", 129)}


@pytest.mark.parametrize("name", list(HEADS))
def test_heads(name):
    lib = _capi.lib()
    T = lib.gsr_head_tile()
    N, Ci, K, H, W, act, want_parts = HEADS[name]
    W = 2 * T + 5 if W is None else W
    gen = _gen("heads", name)
    h, w, b, dy = _randn(gen, N, Ci, H, W), _randn(gen, K, Ci) * 0.3, _randn(gen, K), _randn(gen, N, K, H, W)
    dev = h.device

    def backward(scratch):
        dw, db = torch.empty(K * Ci, device=dev), torch.empty(K, device=dev)
        call("gsr_head_backward", dev, ptr(h), ptr(w), ptr(b), None, ptr(dy), N, Ci, K, H, W, ACT[act], 1.0, 20.0, None, ptr(dw), ptr(db), ptr(scratch))
        return dw, db

    _check("heads", N * _cdiv(H * W, T), want_parts, K * Ci + K, lib.gsr_head_scratch_bytes(N, Ci, K, H, W), backward)


STEM = {"8_ragged_tiles": (2, 3, 8, 18, 130, torch.float16, 8), "64+1": (65, 1, 8, 2, 2, torch.float32, 65)}


@pytest.mark.parametrize("name", list(STEM))
def test_stem(name):
    lib = _capi.lib()
    TH, TW = _tile2("sc_tile")
    N, Ci, Co, H, W, dt, want_parts = STEM[name]
    Ho, Wo = (H + 4 - 5) // 2 + 1, (W + 4 - 5) // 2 + 1
    gen = _gen("stem", name)
    x, w, dy = _randn(gen, N, Ci, H, W), _randn(gen, Co, Ci, 5, 5) * 0.2, _randn(gen, N, Co, Ho, Wo, dtype=dt)
    dev = x.device

    def backward(scratch):
        dw, db = torch.empty(Co * Ci * 25, device=dev), torch.empty(Co, device=dev)
        call("sc_backward", dev, ptr(x), ptr(w), ptr(dy), {torch.float32: 0, torch.float16: 1}[dt], N, Ci, Co, H, W, 5, 2, 2, None, ptr(dw), ptr(db),
             ptr(scratch))
        return dw, db

    _check("stem", N * _cdiv(Ho, TH) * _cdiv(Wo, TW), want_parts, Co * (Ci * 25 + 1), lib.sc_scratch_bytes(N, Ci, Co, H, W, 5, 2, 2), backward)


CONV3 = {"1_part": (1, 4, 4, 32, 0, 1), "32+4": (3, 4, 9, 97, 1, 36), "513_tiles_on_512": (1, 4, 76, 864, 0, 512)}


@pytest.mark.parametrize("name", list(CONV3))
def test_conv3x3(name):
    lib = _capi.lib()
    N, Ci, H, W, relu, want_parts = CONV3[name]
    tiles = N * _cdiv(H, C3_WTILE[0]) * _cdiv(W, C3_WTILE[1])
    if name == "513_tiles_on_512":
        assert tiles == C3_PARTS + 1           # one workgroup walks two tiles
    gen = _gen("c3", name)
    x, w, b, dy = _randn(gen, N, Ci, H, W), _randn(gen, 32, Ci, 3, 3) * 0.2, _randn(gen, 32), _randn(gen, N, 32, H, W)
    dev = x.device
    y = None
    if relu:                                   # the mask is the sign of the forward's own output
        y = torch.empty((N, 32, H, W), device=dev)
        call("c3_forward", dev, ptr(x), ptr(w), ptr(b), N, Ci, H, W, 1, ptr(y))

    def backward(scratch):
        dw, db = torch.empty(32 * Ci * 9, device=dev), torch.empty(32, device=dev)
        call("c3_backward", dev, ptr(x), ptr(w), ptr(y), ptr(dy), N, Ci, H, W, relu, None, ptr(dw), ptr(db), ptr(scratch))
        return dw, db

    _check("c3", min(tiles, C3_PARTS), want_parts, 32 * (9 * Ci + 1), lib.c3_scratch_bytes(N, Ci, H, W), backward)
