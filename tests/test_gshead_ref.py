"""CPU: the bounds of gshead_ref.py are reachable and tight enough to mean something, on every input test_gpu_gshead.py uses.

An fp32 NumPy evaluation of the op -- the kernel's decomposition (per-tile partials of the weight and bias sums, then the tiles), in three summation
orders -- has to stay inside the bounds; the same evaluation with ONE error planted has to leave them, in at least one of y, dh, dw, db, on every
case the error can show on at all (a sigmoid mutant cannot show where the activation is softplus; which cases those are is written next to each
mutant).  So the GPU test, which holds the kernels to the same bounds on the same inputs, cannot pass on a kernel that makes one of these errors."""
import functools

import numpy as np
import pytest

import gps_gaussian_amd  # noqa: F401
from gps_gaussian_amd import _capi

import gshead_ref as R

F32 = np.float32


@functools.lru_cache(maxsize=None)
def _tile():
    gps_gaussian_amd.build()
    return int(_capi.lib().gsr_head_tile())


@functools.lru_cache(maxsize=None)
def _case(name):
    c = R.make_case(name, _tile())
    args = (c["h"], c["w"], c["b"], c["dy"], c["act"], c["beta"], c["threshold"])
    return c, R.reference(*args), R.bounds(*args)


CASES = sorted(R.cases(1024))


def _sum32(terms, order):
    """The fp32 sum of the fp32 arrays in `terms` (a list, or an array summed over axis 0) in one of three orders."""
    terms = [np.asarray(t, dtype=F32) for t in terms]
    if order == "pairwise":
        return np.sum(np.stack(terms), axis=0, dtype=F32)
    acc = np.zeros_like(terms[0])
    for t in (terms if order == "index" else terms[::-1]):
        acc = (acc + t).astype(F32)
    return acc


def _sigmoid32(t):
    with np.errstate(over="ignore"):
        return (F32(1) / (F32(1) + np.exp(-t, dtype=F32))).astype(F32)


def evaluate32(c, order="index", mutant=None, T=1024):
    """y, dh, dw, db in fp32 arithmetic, decomposed as the kernels decompose them; `mutant` plants one error."""
    h, w, b, dy, act, beta, thr = c["h"], c["w"], c["b"], c["dy"], c["act"], F32(c["beta"]), F32(c["threshold"])
    N, C, H, W = h.shape
    K, P = w.shape[0], H * W
    h, dy = h.reshape(N, C, P), dy.reshape(N, K, P)
    r = h if mutant == "relu_omitted" else np.maximum(h, F32(0))
    wf = w.reshape(-1)
    wk = (lambda k, c_: wf[c_ * K + k]) if mutant == "w_indexed_ck" else (lambda k, c_: w[k, c_])
    z = np.stack([_sum32(([] if mutant == "bias_dropped" else [np.full((N, P), b[k], F32)]) + [wk(k, c_) * r[:, c_] for c_ in range(C)], order)
                  for k in range(K)], axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        if act == "none":
            y, slope = z, np.ones_like(z)
        elif act == "sigmoid":
            y = _sigmoid32(z)
            slope = y if mutant == "sigmoid_slope_y" else y * (F32(1) - y)
        else:
            bz = beta * z
            soft = (np.log1p(np.exp(bz, dtype=F32), dtype=F32) / beta).astype(F32)
            above = np.zeros_like(bz, dtype=bool) if mutant == "threshold_ignored" else bz > thr
            y = np.where(above, z, soft)
            slope = np.where(above, F32(1), _sigmoid32(z if mutant == "slope_without_beta" else bz))
    dz = (dy * slope).astype(F32)
    mask = (h >= 0) if mutant == "relu_mask_ge" else (h > 0)
    dh = np.stack([_sum32([wk(k, c_) * dz[:, k] for k in range(K)], order) for c_ in range(C)], axis=1) * mask
    # per (sample, tile) partials, then the partials in index order
    tiles = -(-P // T)
    pad = tiles * T - P
    rp = np.pad(np.maximum(h, F32(0)) if mutant == "relu_omitted" else r, ((0, 0), (0, 0), (0, pad))).reshape(N, C, tiles, T)
    dzp = np.pad(dz, ((0, 0), (0, 0), (0, pad))).reshape(N, K, tiles, T)
    pw = np.einsum("nktp,nctp->ntkc", dzp, rp, dtype=F32, optimize=False).reshape(N * tiles, K, C)
    pb = dzp.sum(axis=3, dtype=F32).transpose(0, 2, 1).reshape(N * tiles, K)
    if mutant == "db_missing_from_one_partial":
        pb[0] = 0
    if mutant == "last_partial_dropped_from_dw":
        pw = pw[:-1]
    dw = _sum32(list(pw), order) if len(pw) else np.zeros((K, C), F32)
    db = _sum32(list(pb), order)
    return dict(y=y.reshape(N, K, H, W), dh=dh.reshape(N, C, H, W), dw=dw, db=db)


def _ratios(got, ref, bnd):
    return {k: R.worst_ratio(got[k], ref[k], bnd[k]) for k in R.KEYS}


def test_the_case_table_does_not_depend_on_the_tile_for_its_names():
    assert sorted(R.cases(_tile())) == CASES


@pytest.mark.parametrize("name", CASES)
def test_fp32_evaluations_stay_inside_the_bounds(name):
    c, ref, bnd = _case(name)
    for order in ("index", "reversed", "pairwise"):
        got = evaluate32(c, order, T=_tile())
        q = _ratios(got, ref, bnd)
        print(name, order, q)
        assert all(np.isfinite(got[k]).all() for k in R.KEYS)
        assert max(q.values()) <= 1.0, (order, q)
        assert (got["dh"][c["h"] == 0] == 0).all()


def test_the_planted_pixels_are_where_they_should_be():
    for name in CASES:
        c, ref, _ = _case(name)
        N, C, H, W = c["h"].shape
        z0, y0 = ref["z"][:, 0].reshape(N, -1), ref["y"][:, 0].reshape(N, -1)
        assert 0.35 < (c["h"] < 0).mean() < 0.6 and (c["h"] == 0).sum() >= 8
        got = {what: (z0[n, p], y0[n, p]) for what, n, p in c["planted"]}
        assert got["all_negative"][0] == float(c["b"][0])
        if c["act"] == "sigmoid":
            assert abs(got["z=+90"][0] - 90) < 1e-3 and abs(got["z=-90"][0] + 90) < 1e-3
        if c["act"] == "softplus":
            bz = {k: c["beta"] * v[0] for k, v in got.items()}
            assert 19.97 < bz["below_1e-3"] < 19.99 < 20.01 < bz["above_1e-3"] < 20.03
            assert 19.999 < bz["below_1e-5"] < 20.0 < bz["above_1e-5"] < 20.001 and abs(bz["beta_z=-200"] + 200) < 1e-2
            assert (c["beta"] * ref["z"] > 89).any()          # where an implementation without the threshold overflows


# mutant -> the cases it can show on
MUTANTS = {
    "relu_omitted": lambda c: True,
    "relu_mask_ge": lambda c: True,                                          # every case has exact zeros in h
    "bias_dropped": lambda c: True,
    "w_indexed_ck": lambda c: c["w"].shape[0] > 1,                           # with K = 1, [c, k] and [k, c] are the same element
    "threshold_ignored": lambda c: c["act"] == "softplus",
    "slope_without_beta": lambda c: c["act"] == "softplus",
    "sigmoid_slope_y": lambda c: c["act"] == "sigmoid",
    "db_missing_from_one_partial": lambda c: True,
    "last_partial_dropped_from_dw": lambda c: True,
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_a_single_error_leaves_the_bounds(mutant):
    shown = 0
    for name in CASES:
        c, ref, bnd = _case(name)
        if not MUTANTS[mutant](c):
            continue
        with np.errstate(all="ignore"):
            q = _ratios(evaluate32(c, "index", mutant, T=_tile()), ref, bnd)
        assert max(q.values()) > 2.0, (name, q)
        shown += 1
    assert shown >= 3
