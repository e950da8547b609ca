"""CPU: the bounds of upcat_ref.py are reachable and tight enough to mean something, on every input test_gpu_upcat.py uses.

An fp32 NumPy evaluation of the op in the order csrc/upcat.hip states (and with the two axes exchanged: the same number of roundings) has to stay
inside the bounds; the fp64 restatement with ONE error planted has to leave them on every case the error can show on at all (which cases those are
is written next to each mutant).  So the GPU test, which holds the kernels to the same bounds on the same inputs, cannot pass on a kernel that makes
one of these errors.  And the unmutated restatement is nn.Upsample(scale_factor=2, mode="bilinear") + torch.cat and its autograd, in fp64."""
import functools

import numpy as np
import pytest

import gps_gaussian_amd
from gps_gaussian_amd import upcat

import upcat_ref as R

F32 = np.float32


@functools.lru_cache(maxsize=None)
def _tile():
    gps_gaussian_amd.build()
    return upcat.tile()


CASES = sorted(R.cases(16, 256))


@functools.lru_cache(maxsize=None)
def _case(name, integers=False):
    c = R.make_case(name, *_tile(), integers=integers)
    Ca = c["a"].shape[1]
    return c, R.forward(c["a"], c["skips"]), R.forward_bound(c["a"]), R.backward(c["dout"], Ca), R.backward_bound(c["dout"], Ca)


def test_the_case_table_does_not_depend_on_the_tile_for_its_names():
    assert sorted(R.cases(*_tile())) == CASES
    TH, TW = _tile()
    assert TH % 2 == 0 and TW % 4 == 0 and TH >= 4 and TW >= 8


def _fma32(m, p, q):
    """fmaf(m, p, 0.25 q) for m = 0.75: the product and the quarter are exact in fp64, the sum is rounded to fp32 once (fp64's own rounding of the
    sum is 2^29 times finer)."""
    return (m * p.astype(np.float64) + 0.25 * q.astype(np.float64)).astype(F32)


def _up_axis32(v, axis):
    """o[2i] = fmaf(0.75, v[i], 0.25 v[max(i-1, 0)]), o[2i+1] = fmaf(0.75, v[i], 0.25 v[min(i+1, n-1)]) along `axis`, in fp32."""
    v = np.moveaxis(v, axis, -1)
    n = v.shape[-1]
    i = np.arange(n)
    o = np.empty(v.shape[:-1] + (2 * n,), F32)
    o[..., 0::2] = _fma32(0.75, v, v[..., np.maximum(i - 1, 0)])
    o[..., 1::2] = _fma32(0.75, v, v[..., np.minimum(i + 1, n - 1)])
    return np.moveaxis(o, -1, axis)


def _gather_axis32(d, axis):
    """g[i] = fmaf(0.75, d[2i] + d[2i+1], 0.25 (d[clamp(2i-1)] + d[clamp(2i+2)])) along `axis`, in fp32."""
    d = np.moveaxis(d, axis, -1)
    n2 = d.shape[-1]
    i = np.arange(n2 // 2)
    inner = (d[..., 2 * i] + d[..., 2 * i + 1]).astype(F32)
    outer = (d[..., np.maximum(2 * i - 1, 0)] + d[..., np.minimum(2 * i + 2, n2 - 1)]).astype(F32)
    return np.moveaxis(_fma32(0.75, inner, outer), -1, axis)


def forward32(a, skips, x_first=True):
    up = _up_axis32(_up_axis32(a, 3), 2) if x_first else _up_axis32(_up_axis32(a, 2), 3)
    return np.concatenate([up] + list(skips), axis=1)


def backward32(dout, Ca, x_first=True):
    d = np.ascontiguousarray(dout[:, :Ca])
    return _gather_axis32(_gather_axis32(d, 3), 2) if x_first else _gather_axis32(_gather_axis32(d, 2), 3)


@pytest.mark.parametrize("name", CASES)
def test_fp32_evaluations_stay_inside_the_bounds(name):
    c, out, ob, da, db = _case(name)
    Ca = c["a"].shape[1]
    for x_first in (True, False):
        got, gda = forward32(c["a"], c["skips"], x_first), backward32(c["dout"], Ca, x_first)
        qf, qb = R.worst_ratio(got[:, :Ca], out[:, :Ca], ob), R.worst_ratio(gda, da, db)
        print(name, "x first" if x_first else "y first", qf, qb)
        assert qf <= 1.0 and qb <= 1.0
        assert (got[:, Ca:] == out[:, Ca:]).all()
    assert (ob > 0).all() and (db > 0).all()


@pytest.mark.parametrize("name", CASES)
def test_whole_numbers_are_exact(name):
    c, out, _, da, _ = _case(name, integers=True)
    Ca = c["a"].shape[1]
    assert (forward32(c["a"], c["skips"]).astype(np.float64) == out).all()
    assert (backward32(c["dout"], Ca).astype(np.float64) == da).all()
    assert out[:, :Ca, 0, 0].tolist() == c["a"][:, :, 0, 0].tolist() and out[:, :Ca, -1, -1].tolist() == c["a"][:, :, -1, -1].tolist()


def _shape(c):
    return c["a"].shape[2], c["a"].shape[3], len(c["skips"])


# mutant -> the cases it can show on
SHOWS = {
    "weights_swapped": lambda h, w, K: h > 1 or w > 1,             # an axis of length 1 is duplicated whatever the weights are
    "low_clamp_missing": lambda h, w, K: True,
    "high_clamp_off_by_one": lambda h, w, K: h > 1 or w > 1,      # with one element, index n - 2 clamps back onto it
    "even_odd_exchanged": lambda h, w, K: h > 1 or w > 1,
    "skip_offset_off_by_one": lambda h, w, K: K >= 1,
    "skips_reversed": lambda h, w, K: K >= 2,
    "da_missing_folded_tap": lambda h, w, K: True,
}


@pytest.mark.parametrize("mutant", R.FORWARD_MUTANTS)
def test_a_single_error_in_the_forward_leaves_the_bounds(mutant):
    shown = 0
    for name in CASES:
        c, out, ob, _, _ = _case(name)
        if not SHOWS[mutant](*_shape(c)):
            continue
        Ca = c["a"].shape[1]
        got = R.forward(c["a"], c["skips"], mutant)
        q = R.worst_ratio(got[:, :Ca], out[:, :Ca], ob)
        assert q > 16.0 or (got[:, Ca:] != out[:, Ca:]).any(), (name, q)
        shown += 1
    assert shown >= 2


@pytest.mark.parametrize("mutant", R.BACKWARD_MUTANTS)
def test_a_single_error_in_the_backward_leaves_the_bounds(mutant):
    shown = 0
    for name in CASES:
        c, _, _, da, db = _case(name)
        if not SHOWS[mutant](*_shape(c)):
            continue
        q = R.worst_ratio(R.backward(c["dout"], c["a"].shape[1], mutant), da, db)
        assert q > 16.0, (name, q)
        shown += 1
    assert shown >= 3


@pytest.mark.parametrize("name", CASES)
def test_the_restatement_is_upsample_and_cat_in_fp64(name):
    import torch
    from torch import nn
    u64 = 2.0 ** -53
    for integers in (False, True):
        c, out, ob, da, db = _case(name, integers)
        Ca = c["a"].shape[1]
        a = torch.from_numpy(c["a"]).double().requires_grad_(True)
        y = torch.cat([nn.Upsample(scale_factor=2, mode="bilinear")(a)] + [torch.from_numpy(s).double() for s in c["skips"]], dim=1)
        y.backward(torch.from_numpy(c["dout"]).double())
        dy, dg = np.abs(y.detach().numpy() - out), np.abs(a.grad.numpy() - da)
        if integers:
            assert dy.max() == 0.0 and dg.max() == 0.0
        # a handful of fp64 roundings on either side of 4 (16) taps: 16 u64 (64 u64) of the weighted absolute sum
        assert (dy[:, :Ca] <= 16 * u64 * ob / (R.K_FWD * R.U32)).all() and (dy[:, Ca:] == 0).all()
        assert (dg <= 64 * u64 * db / (R.K_BWD * R.U32)).all()
