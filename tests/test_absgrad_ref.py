"""CPU: the two references of the absolute screen-space gradient (tests/absgrad_ref.py) agree with each other and with the oracle's own backward
before they judge a kernel (tests/test_gpu_raster_absgrad.py).

Tolerances: the replay against the per-pixel Jacobian of the fp64 renderer 1e-4 -- a tenth of the suite's 1e-3 gradient tolerance, so that the
references' own error cannot eat it; the replay's SIGNED sums against OracleRasterizer.backward() 1e-3, the suite's tolerance (the oracle's backward
is fp32).  Both in the suite's normalised error |a - ref| / (|ref| + 1e-3 max|ref|).
"""
import numpy as np
import pytest

from conftest import fragile_bounds, oracle_render

from absgrad_ref import absgrad_jacobian, absgrad_replay, norm_err, tiny_scene
from raster_run import small


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_replay_equals_the_jacobian_on_tiny_scenes(seed):
    """24 x 16 pixels, 40 Gaussians: the tile replay gives what one autograd backward per pixel through the fp64 renderer gives.  The oracle reports
    no fragile pixel on these scenes -- the GPU test against the Jacobian relies on it (nobody is excused there)."""
    g = tiny_scene(seed)
    dpix = np.random.default_rng(100 + seed).standard_normal((3, g["H"], g["W"])).astype(np.float32)
    o, _, radii = oracle_render(g)
    solid, touched, _ = fragile_bounds(o, dpix)
    assert solid.all() and not touched.any()
    rab, rsg = absgrad_replay(o, dpix)
    jab, jsg = absgrad_jacobian(g, dpix)
    assert (jab > 0).any(axis=1).sum() >= 10
    e_abs, e_sg = norm_err(rab, jab).max(), norm_err(rsg, jsg).max()
    print("seed %d: replay vs Jacobian, normalised error: absolute sums %.3e, signed sums %.3e" % (seed, e_abs, e_sg))
    assert e_abs <= 1e-4  # (the signed sums cancel; they are pinned against the oracle's backward below, at the suite's tolerance)
    assert (rab[radii == 0] == 0).all()
    # the triangle inequality, and real cancellation: the absolute sum is the larger one by a margin for the typical Gaussian
    assert (np.abs(jsg) <= jab * (1 + 1e-12) + 1e-300).all()
    vis = jab[:, 0] > 0
    assert np.median(jab[vis, 0] / np.maximum(np.abs(jsg[vis, 0]), 1e-300)) > 1.5


@pytest.mark.parametrize("name", ["96x64", "256"])
def test_replay_signed_sums_equal_the_oracle_backward(name):
    """The replay's signed sums are the oracle's dL/dmeans2D: the walk, the recurrence and the units are the backward's own."""
    from gps_gaussian_amd import synthetic as S
    g = small() if name == "96x64" else S.make_scene(256, 30000)
    dpix = np.random.default_rng(7).standard_normal((3, g["H"], g["W"])).astype(np.float32)
    o, _, _ = oracle_render(g)
    ref = o.backward(dpix)["means2D"][:, :2]
    rab, rsg = absgrad_replay(o, dpix)
    e = norm_err(rsg, ref).max()
    print("%s: replay signed sums vs oracle backward, normalised error %.3e" % (name, e))
    assert e <= 1e-3
    assert (np.abs(rsg) <= rab * (1 + 1e-12) + 1e-300).all()
    nz = np.abs(ref[:, 0]) > 0
    print("%s: median absgrad / |grad| = %.2f" % (name, np.median(rab[nz, 0] / np.abs(ref[nz, 0]))))
