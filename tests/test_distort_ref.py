"""CPU: the two references of the depth-distortion map (tests/distort_ref.py) agree with each other before they judge a kernel
(tests/test_gpu_raster_distortion.py), and the pairwise double sum equals the list-order form the kernels accumulate.

Tolerances, in the suite's normalised error |a - ref| / (|ref| + 1e-3 max|ref|): the replay against the definition 1e-5 for the map and 1e-4 for the
gradients -- a tenth of the suite's 1e-4 image and 1e-3 gradient tolerances, so that the references' own error cannot eat them (the replay takes its
geometry from the fp32 oracle: its error is a few fp32 roundings).  The two forms of the sum in fp64: 1e-12.
"""
import numpy as np
import pytest

from conftest import fragile_bounds, oracle_render

from absgrad_ref import norm_err, tiny_scene
from distort_ref import distort_definition, distort_replay, means3D_chain


def _g(scene, seed):
    return np.random.default_rng(seed).standard_normal((scene["H"], scene["W"])).astype(np.float32)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_replay_equals_the_definition_on_tiny_scenes(seed):
    """24 x 16 pixels, 40 Gaussians: the gap-form tile replay gives what fp64 autograd through the pairwise double sum gives -- the map, dL/dopacity,
    dL/dmeans2D, and dL/dmeans3D through the projection chain (which carries the replay's dL/dconic and dL/dz).  The oracle reports no fragile pixel
    on these scenes and they have no depth tie: the GPU test against the definition relies on both."""
    s = tiny_scene(seed)
    g = _g(s, 200 + seed)
    o, _, radii = oracle_render(s)
    solid, touched, _ = fragile_bounds(o)
    assert solid.all() and not touched.any()
    z = o.geom()["depth"][radii > 0]
    assert len(np.unique(z.astype(np.float32))) == len(z)
    dmap, ref = distort_definition(s, g)
    rmap, part = distort_replay(o, g)
    assert (dmap > 0).sum() >= 300 and (dmap >= 0).all() and (rmap >= 0).all()
    m3, m3_without = means3D_chain(s, o, part)
    e = dict(map=norm_err(rmap, dmap).max(), opacities=norm_err(part["opacities"], ref["opacities"][:, 0]).max(),
             means2D=norm_err(part["means2D"], ref["means2D"][:, :2]).max(), means3D=norm_err(m3, ref["means3D"]).max())
    print("seed %d: replay vs definition, %d of %d pixels non-zero, normalised errors %s" % (
        seed, (dmap > 0).sum(), dmap.size, ", ".join("%s %.3e" % kv for kv in e.items())))
    assert e["map"] <= 1e-5
    assert max(e["opacities"], e["means2D"], e["means3D"]) <= 1e-4
    # the depth term is a real part of dL/dmeans3D (without it the chain misses the definition), and it is what the view matrix's third row carries
    assert norm_err(m3_without, ref["means3D"]).max() > 1e-2
    np.testing.assert_allclose(m3 - m3_without, part["dz"][:, None] * (radii > 0)[:, None] * np.asarray(s["view"], np.float64).reshape(4, 4)[:3, 2][None, :],
                               rtol=1e-9, atol=1e-10 * np.abs(m3).max())
    for k in ("opacities", "means2D", "dz"):
        assert (part[k][radii == 0] == 0).all()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_pairwise_and_ordered_forms_agree(seed):
    """sum_i sum_j w_i w_j |z_i - z_j| = 2 sum_i w_i (z_i A_<i - D_<i) when the list is in depth order: fp64, the weights of the tiny scenes."""
    import torch
    from distort_ref import _t64, blend_weights, ordered, pairwise, view_depth
    s = tiny_scene(seed)
    t = _t64(s)
    with torch.no_grad():
        w = blend_weights(s, t, None)
        z = view_depth(t["means3D"], t["view"])
        a, b = pairwise(w, z).numpy(), ordered(w, z).numpy()
    e = np.abs(a - b).max() / np.abs(a).max()
    print("seed %d: pairwise vs ordered form, max |difference| / max %.3e" % (seed, e))
    assert a.max() > 0 and e <= 1e-12
    # invariant under a shift of z, homogeneous of degree 1 in z
    with torch.no_grad():
        assert np.abs(pairwise(w, z + 5.0).numpy() - a).max() <= 1e-12 * a.max()
        assert np.abs(pairwise(w, 3.0 * z).numpy() - 3.0 * a).max() <= 1e-12 * a.max()


def test_replay_closed_forms():
    """Two splats that cover a pixel fully enough to be blended: dist = 2 w_0 w_1 (z_1 - z_0); one splat: 0."""
    from conftest import gaussians, simple_scene
    cam = simple_scene(16, 16, 20.0)
    for n, zs in ((1, [2.0]), (2, [2.0, 2.5])):
        s = dict(cam, **gaussians(np.array([[0.0, 0.0, z] for z in zs]), np.ones((n, 3)) * 0.5, np.full(n, 0.6), np.full((n, 3), 2.0)))
        o, _, radii = oracle_render(s)
        assert (radii > 0).all()
        rmap, _ = distort_replay(o, np.ones((16, 16), np.float32))
        if n == 1:
            assert (rmap == 0).all()
            continue
        co = o.geom()["conic_opacity"].astype(np.float64)
        xy = o.geom()["xy"].astype(np.float64)
        zz = o.geom()["depth"].astype(np.float64)
        ys, xs = np.mgrid[0:16, 0:16]
        al = []
        for i in range(2):
            dx, dy = xy[i, 0] - xs, xy[i, 1] - ys
            al.append(np.minimum(0.99, co[i, 3] * np.exp(-0.5 * (co[i, 0] * dx * dx + co[i, 2] * dy * dy) - co[i, 1] * dx * dy)))
        assert min(a.min() for a in al) > 0.05  # every pixel blends both
        closed = 2.0 * al[0] * (1.0 - al[0]) * al[1] * (zz[1] - zz[0])
        assert norm_err(rmap, closed).max() <= 1e-6


def test_dense_definition_equals_the_definition_on_a_stack():
    """65 faint, wide splats at distinct depths on an 8 x 8 image: every one is blended into every pixel, and the closed-form blend gives what the
    one-hot renders give (the GPU test walks stacks of up to 129 with it)."""
    from distort_ref import dense_definition, stack
    s = stack(65, 8, 8, 0.02, 2.0, 65)
    g = _g(s, 65)
    dmap, ref = distort_definition(s, g)
    emap, got = dense_definition(s, g)
    assert (dmap > 0).all()
    e = dict(map=norm_err(emap, dmap).max(), **{k: norm_err(got[k], ref[k]).max() for k in ("means3D", "opacities", "scales", "rotations", "means2D", "colors")})
    print("dense vs one-hot definition: %s" % ", ".join("%s %.3e" % kv for kv in e.items()))
    assert max(e.values()) <= 1e-9
    with pytest.raises(ValueError):
        dense_definition(tiny_scene(1), _g(tiny_scene(1), 1))
