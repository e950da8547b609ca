"""CPU: the references of the correlation lookup against each other, so that the GPU edge tests (tests/test_gpu_corr_lookup_edges.py) lean on more
than the C twin, which shares the kernels' `floorf` / `dx` / tap-index arithmetic.

  1. the twin (oracle/aux_oracle.c cs_oracle_*), forward and backward, against the hat function and its autograd (tests/corr_edge_ref.py) within
     the derived bound 4 * 2^-24 * S, at the special coordinates of every (W2, r) of the sampler table;
  2. oracle/corr_oracle.py lookup / lookup_backward (fp64) against the hat function at 1e-12 * S, 1 to 4 levels, zero-width levels included;
  3. the reference's own pure-torch path (CorrBlock1D: grid_sample on a height-1 image, align_corners=True, zero padding) against the hat function:
     this ties the hat function to the reference's semantics.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import corr_edge_ref as R
from oracle import corr_oracle as CO


@pytest.mark.parametrize("r", R.SAMPLER_R)
def test_twin_is_within_the_derived_bound_of_the_hat_function(r):
    worst_f = worst_b = 0.0
    for W2 in R.SAMPLER_W2:
        c = R.special_coords(W2, r).reshape(1, 1, 1, -1)
        W1 = c.shape[-1]
        vol = R.randn((1, 1, W1, W2), ("twin", W2, r))
        gout = R.randn((1, 2 * r + 1, 1, W1), ("twin-g", W2, r))
        rf = R.bound_ratio(R.twin_forward(vol, c, r), R.hat_lookup([vol], c, r), R.hat_magnitude([vol], c, r))
        (gref,), (gmag,) = R.hat_backward([W2], c, gout, r)
        rb = R.bound_ratio(R.twin_backward(c, gout, W2, r), gref, gmag)
        assert rf <= 1.0 and rb <= 1.0, (W2, r, rf, rb)
        worst_f, worst_b = max(worst_f, rf), max(worst_b, rb)
    R.report(dict(test="twin_vs_hat", family="cpu twin, r=%d" % r, forward_over_bound=worst_f, backward_over_bound=worst_b))


@pytest.mark.parametrize("levels", R.LOOKUP_LEVELS)
def test_numpy_oracle_agrees_with_the_hat_function(levels):
    """fp64 against fp64: 1e-12 * S leaves four decimal digits over the roundings of either side."""
    worst_f = worst_b = 0.0
    for W2 in R.ORACLE_W2:
        for r in R.LOOKUP_R:
            c = R.special_coords(W2, r).reshape(1, 1, 1, -1)
            W1 = c.shape[-1]
            wl = R.widths(W2, levels)
            pyr = [R.randn((1, 1, W1, w), ("oracle", W2, r, l)).double() for l, w in enumerate(wl)]
            gout = R.randn((1, levels * (2 * r + 1), 1, W1), ("oracle-g", W2, r, levels)).double()
            out = torch.from_numpy(CO.lookup([p.numpy() for p in pyr], c.numpy(), r))
            err = (out - R.hat_lookup(pyr, c, r)).abs()
            tol = 1e-12 * R.hat_magnitude(pyr, c, r)
            assert bool((err <= tol).all()), (W2, r, float((err - tol).max()))
            worst_f = max(worst_f, float((err / tol.clamp_min(1e-300)).max()))
            grefs, gmags = R.hat_backward(wl, c, gout, r)
            got = CO.lookup_backward(wl, c.numpy(), gout.numpy(), r)
            for l, w in enumerate(wl):
                assert got[l].shape == (1, 1, W1, w)
                e = (torch.from_numpy(got[l]) - grefs[l]).abs()
                t = 1e-12 * gmags[l]
                assert bool((e <= t).all()), (W2, r, l)
                if w:
                    worst_b = max(worst_b, float((e / t.clamp_min(1e-300)).max()))
            for l, w in enumerate(wl):      # a level of width 0 contributes zero channels
                if w == 0:
                    assert not out[:, l * (2 * r + 1):(l + 1) * (2 * r + 1)].any()
    R.report(dict(test="numpy_oracle_vs_hat", family="fp64 oracle, %d levels" % levels, forward_over_tolerance=worst_f, backward_over_tolerance=worst_b))


def _grid_sample_path(vol, coords, r):
    """CorrBlock1D.__call__ for one level (core/corr.py:127-146 -> bilinear_sampler, core/utils/utils.py:59-74), as
    tests/test_gpu_corr.py::test_autograd_function_as_the_reference_wraps_it restates it, in the dtype of `vol`."""
    N, H1, W1, W2 = vol.shape
    dx = torch.linspace(-r, r, 2 * r + 1, dtype=vol.dtype).view(1, 1, 2 * r + 1, 1)
    x0 = dx + coords.to(vol.dtype).reshape(N * H1 * W1, 1, 1, 1)
    grid = torch.cat([2 * x0 / (W2 - 1) - 1, torch.zeros_like(x0)], dim=-1)
    samp = F.grid_sample(vol.reshape(N * H1 * W1, 1, 1, W2), grid, align_corners=True)
    return samp.view(N, H1, W1, -1).permute(0, 3, 1, 2)


# W2 == 1 is left out: the path above divides by W2 - 1 = 0 there (the reference never builds a level that narrow)
@pytest.mark.parametrize("W2", [w for w in R.SAMPLER_W2 if w >= 2])
def test_grid_sample_path_of_the_reference_agrees_with_the_hat_function(W2):
    """In fp64 the reference's path IS the hat function: its only extra error is that of the normalised grid, 2 x0 / (W2 - 1) - 1 and back, a few
    fp64 ulp of the position times the slope of the row (<= 2 max |V|) -- 1e-12 max |V| leaves three digits.  In fp32 the same detour costs up to
    about W2 * 2^-23 in position, so the fp32 path is held to its OWN measured error: max |fp32 path - fp64 path|, the error of grid_sample's fp32
    arithmetic on these inputs, which is recorded; the tolerance is twice that (once for the fp32 path itself, and room for the 1e-12 above)."""
    for r in (0, 1, 4):
        c = R.special_coords(W2, r).reshape(1, 1, 1, -1)
        W1 = c.shape[-1]
        vol = R.randn((1, 1, W1, W2), ("gs", W2, r))
        gout = R.randn((1, 2 * r + 1, 1, W1), ("gs-g", W2, r))
        hat = R.hat_lookup([vol], c, r)
        (ghat,), _ = R.hat_backward([W2], c, gout, r)
        res = {}
        for dt in (torch.float64, torch.float32):
            v = vol.to(dt).clone().requires_grad_(True)
            out = _grid_sample_path(v, c, r)
            out.backward(gout.to(dt))
            res[dt] = (out.detach().double(), v.grad.double())
        vmax, gmax = float(vol.abs().max()), float(gout.abs().max())
        assert float((res[torch.float64][0] - hat).abs().max()) <= 1e-12 * vmax
        assert float((res[torch.float64][1] - ghat).abs().max()) <= 1e-12 * gmax
        own_f = float((res[torch.float32][0] - res[torch.float64][0]).abs().max())
        own_b = float((res[torch.float32][1] - res[torch.float64][1]).abs().max())
        err_f = float((res[torch.float32][0] - hat).abs().max())
        err_b = float((res[torch.float32][1] - ghat).abs().max())
        R.report(dict(test="grid_sample_vs_hat", family="W2=%d r=%d" % (W2, r), own_error_forward=own_f / vmax, own_error_backward=own_b / gmax,
                      error_vs_hat_forward=err_f / vmax, error_vs_hat_backward=err_b / gmax))
        assert err_f <= 2.0 * own_f and err_b <= 2.0 * own_b, (W2, r, err_f, own_f, err_b, own_b)
        # the measured error is what the derivation says: a position error of a few ulp of W2 times the slope, never a misplaced tap
        assert own_f <= 8 * W2 * R.U * 2 * vmax and own_b <= 8 * W2 * R.U * 2 * gmax, (W2, r, own_f, own_b)


def test_special_coords_hold_what_the_header_promises():
    for W2, r in ((1, 0), (8, 4), (64, 7)):
        c = R.special_coords(W2, r).numpy()
        ints = np.arange(-r - 2, W2 + r + 3, dtype=np.float32)
        assert np.isin(ints, c).all() and np.isin(ints + np.float32(0.5), c).all()
        nz = ints[ints != 0]
        assert np.isin(np.nextafter(nz, np.float32(np.inf)), c).all() and np.isin(np.nextafter(nz, np.float32(-np.inf)), c).all()
        assert np.isin(np.array(R.FAR, np.float32), c).all() and np.signbit(c[c == 0]).any()
        assert c.size == 4 * ints.size + len(R.FAR) + 64 and c.dtype == np.float32
        assert np.isfinite(c).all() and not ((c != 0) & (np.abs(c) < R.TINY)).any()
        # x in (-2^-25, 0): dx = x - floor(x) rounds to 1
        x = c[(c < 0) & (c > -2.0 ** -25)]
        assert x.size >= 3 and ((x - np.floor(x)) == np.float32(1.0)).all()
        g = R.coords_grid(W2, r, 2, 2)
        assert g.shape[:3] == (2, 1, 2) and g.numel() >= c.size and np.array_equal(g.reshape(-1)[:c.size].numpy(), c, equal_nan=False)
