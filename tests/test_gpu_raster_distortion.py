"""GPU (-m gpu): the opt-in depth-distortion map of the rasteriser (include/gpsgs.h GsrDistort; rasterizer.rasterize_gaussians(return_distortion=True);
render_api.render_ex(distortion=True); render_api.pts2render(with_distortion=True)).

The spec: per pixel, over the splats blended into the image there, distortion = sum_i sum_j w_i w_j |z_i - z_j| (w = alpha T, z the view-space depth),
differentiable.  Checked against two references that do not reuse the kernel's running-sum form (tests/distort_ref.py: fp64 autograd through the
pairwise double sum, and a gap-form replay of the fp32 oracle's blend; tests/test_distort_ref.py pins them against each other) at the project's image
and gradient tolerances -- 1e-4 and 1e-3 in the normalised error |a - ref| / (|ref| + 1e-3 max|ref|) -- and against closed forms, bounds and
bit identities.  Every comparison prints its measured maximum before it asserts.
"""
import numpy as np
import pytest

from conftest import fragile_bounds, oracle_render
from distort_ref import stack as _stack
from raster_run import batch as _batch, decode, leaves, rasterize, render_ex_rows, run_view, scene as _scene, settings, valu_fixture

pytestmark = pytest.mark.gpu

MAP_TOL, GRAD_TOL = 1e-4, 1e-3
GRADS = ("means3D", "opacities", "scales", "rotations", "means2D", "colors")

_valu = valu_fixture()  # the runs without the map that the distortion runs are compared with use the VALU family too (the distortion runs always do)


def _run(g, distortion=True, gdist=None, dpix=None, gdepth=None, galpha=None, **kw):
    """run_view with the map on by default, then (if any gradient is given) the backward of sum(dist * gdist) + sum(img * dpix) + sum(depth * gdepth)
    + sum(alpha * galpha).  dist comes back as [H, W]."""
    return run_view(g, dict(dist=gdist, img=dpix, depth=gdepth, alpha=galpha), distortion=distortion, **kw)


def _rand(g, seed, ch=None):
    shape = (g["H"], g["W"]) if ch is None else (ch, g["H"], g["W"])
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _equal_grads(a, b):
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ---- tiny scenes against the definition -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mixed", [False, True], ids=["g", "g+img+depth+alpha"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_tiny_scenes_against_the_definition(seed, mixed):
    """24 x 16 pixels, 40 Gaussians, no fragile pixel and no depth tie (tests/test_distort_ref.py asserts both): the map and every gradient against
    fp64 autograd through the pairwise double sum -- with the map's gradient alone, and together with gradients of the image, depth and alpha maps."""
    from absgrad_ref import norm_err, tiny_scene
    from distort_ref import distort_definition
    g = tiny_scene(seed)
    gd = _rand(g, 200 + seed)
    kw = dict(dpix=_rand(g, 300 + seed, 3), gdepth=_rand(g, 400 + seed), galpha=_rand(g, 500 + seed)) if mixed else {}
    r = _run(g, gdist=gd, extras=mixed, **kw)
    ref_map, ref = distort_definition(g, gd, **kw)
    e_map = norm_err(r["dist"], ref_map).max()
    e = {k: norm_err(r["grads"][k], ref[k]).max() for k in GRADS}
    print("seed %d %s: map %.3e; gradients %s" % (seed, "mixed" if mixed else "g alone", e_map, ", ".join("%s %.3e" % kv for kv in e.items())))
    assert (ref_map > 0).sum() >= 300
    assert e_map <= MAP_TOL
    for k in GRADS:
        assert e[k] <= GRAD_TOL, k
    assert np.abs(ref["means3D"]).max() > 0 and np.abs(ref["scales"]).max() > 0


def test_camera_gradient_includes_the_depth_term():
    """camera_grad: dL/dviewmatrix and dL/dprojmatrix of sum g dist against the definition (the view matrix's third column carries the new dL/dz)."""
    from absgrad_ref import norm_err, tiny_scene
    from distort_ref import distort_definition
    g = tiny_scene(2)
    gd = _rand(g, 77)
    r = _run(g, gdist=gd, cam=True)
    _, ref = distort_definition(g, gd, camera=True)
    plain = _run(g, gdist=gd)
    for k in plain["grads"]:
        np.testing.assert_array_equal(r["grads"][k], plain["grads"][k], err_msg=k)  # the per-Gaussian gradients keep their bits
    ev, ep = norm_err(r["grads"]["view"], ref["view"]).max(), norm_err(r["grads"]["proj"], ref["proj"]).max()
    print("camera gradients vs definition: view %.3e, proj %.3e; |dL/dview[:, 2]| max %.3e" % (ev, ep, np.abs(ref["view"][:, 2]).max()))
    assert np.abs(ref["view"][:, 2]).max() > 0
    assert ev <= GRAD_TOL and ep <= GRAD_TOL


# ---- make_scene(256, 30000) against the replay of the fp32 oracle ----------------------------------------------------------------------------------------

def test_256_scene_against_the_oracle_replay():
    """The map on the solid pixels, dL/dopacity, dL/dmeans2D and dL/dmeans3D on the visible Gaussians that take part in no fragile pixel.  dL/dmeans3D's
    reference is the replay's partials pushed through the fp64 projection: (kernel - the chain without dL/dz) must be dL/dz * viewmatrix[:, 2]."""
    from absgrad_ref import norm_err
    from distort_ref import distort_replay, means3D_chain
    g = _scene("256")
    gd = _rand(g, 13)
    r = _run(g, gdist=gd)
    o, _, oradii = oracle_render(g)
    np.testing.assert_array_equal(r["radii"] > 0, oradii > 0)
    solid, touched, _ = fragile_bounds(o)
    visible = oradii > 0
    strict = visible & ~touched
    left_px, left_g = 1.0 - solid.mean(), 1.0 - strict.sum() / max(1, visible.sum())
    rmap, part = distort_replay(o, gd)
    m3, m3_without = means3D_chain(g, o, part)
    e_map = norm_err(r["dist"], rmap)
    e_op = norm_err(r["grads"]["opacities"][:, 0], part["opacities"])
    e_m2 = norm_err(r["grads"]["means2D"][:, :2], part["means2D"])
    e_m3 = norm_err(r["grads"]["means3D"], m3)
    zpart = m3 - m3_without
    print("256: %.4f %% of the pixels and %.3f %% of the visible Gaussians left out; map %.3e (all pixels %.3e); opacities %.3e, means2D %.3e, means3D %.3e; "
          "max|dL/dz v| / max|dL/dmeans3D| = %.3f" % (100 * left_px, 100 * left_g, e_map[solid].max(), e_map.max(), e_op[strict].max(), e_m2[strict].max(),
                                                     e_m3[strict].max(), np.abs(zpart).max() / np.abs(m3).max()))
    assert left_px <= 1e-3 and left_g <= 1e-2
    assert (rmap[solid] > 0).sum() > 1000 and (np.abs(part["opacities"][strict]) > 0).sum() > 1000
    assert e_map[solid].max() <= MAP_TOL
    assert e_op[strict].max() <= GRAD_TOL and e_m2[strict].max() <= GRAD_TOL
    # dL/dmeans3D minus the part that does not come through z equals dL/dz * viewmatrix[:, 2], to the tolerance of the whole gradient
    assert np.abs(zpart).max() > 1e-2 * np.abs(m3).max()
    np.testing.assert_allclose(zpart[visible], (part["dz"][:, None] * np.asarray(g["view"], np.float64).reshape(4, 4)[:3, 2][None, :])[visible], rtol=1e-9, atol=1e-10 * np.abs(m3).max())
    allowed = GRAD_TOL * (np.abs(m3) + GRAD_TOL * np.abs(m3).max())
    assert (np.abs((r["grads"]["means3D"] - m3_without) - zpart) <= allowed)[strict].all()


# ---- kernel edges: round boundaries of the running and suffix sums, saturation, closed forms -------------------------------------------------------------

@pytest.mark.parametrize("n,W,H", [(63, 8, 8), (64, 17, 9), (65, 8, 8), (129, 17, 9)])
def test_stacks_across_round_boundaries(n, W, H):
    """n splats at distinct depths, opacity 0.02, every one blended into every pixel (0.98^129 = 0.07: nobody saturates): the forward's running sums and
    the backward's suffix sums cross the 64-entry rounds.  Against the definition in its closed form for such scenes (distort_ref.dense_definition,
    pinned against the one-hot renders in tests/test_distort_ref.py)."""
    from absgrad_ref import norm_err
    from distort_ref import dense_definition
    g = _stack(n, W, H, 0.02, 2.0, n)
    gd = _rand(g, n)
    r = _run(g, gdist=gd, extras=True)
    assert (r["radii"] > 0).all()
    ref_map, ref = dense_definition(g, gd)
    assert (ref_map > 0).all()
    e_map = norm_err(r["dist"], ref_map).max()
    e = {k: norm_err(r["grads"][k], ref[k]).max() for k in GRADS}
    print("stack of %d on %dx%d: map %.3e; gradients %s" % (n, W, H, e_map, ", ".join("%s %.3e" % kv for kv in e.items())))
    assert e_map <= MAP_TOL
    for k in GRADS:
        assert e[k] <= GRAD_TOL, k
    # every splat is blended everywhere: alpha is 1 - prod(1 - alpha_i) and the bound holds with the stack's own depth range
    assert (r["dist"] <= r["alpha"][0] ** 2 * (0.005 * (n - 1)) * (1 + 1e-5)).all()


def test_stack_in_which_some_pixels_saturate_mid_list():
    """70 splats of opacity 0.6 and 3 pixels of sigma on a 17 x 9 image: the central pixels stop after about ten entries, their neighbours walk the whole
    list.  Against the replay of the fp32 oracle (the decisions are fp32 ones) on the solid pixels and untouched Gaussians."""
    from absgrad_ref import norm_err
    from distort_ref import distort_replay
    g = _stack(70, 17, 9, 0.6, 0.3, 5, spread=0.02)
    gd = _rand(g, 6)
    r = _run(g, gdist=gd)
    o, _, oradii = oracle_render(g)
    b = o.binning()
    nc, fT = b["n_contrib"], b["final_T"]
    assert ((nc > 0) & (nc < 64)).any() and (fT < 1e-3).any() and ((nc > 64) & (fT > 1e-2)).any()  # stopped early / walked past a round boundary
    solid, touched, _ = fragile_bounds(o)
    strict = (oradii > 0) & ~touched
    rmap, part = distort_replay(o, gd)
    e_map = norm_err(r["dist"], rmap)
    e_op = norm_err(r["grads"]["opacities"][:, 0], part["opacities"])
    e_m2 = norm_err(r["grads"]["means2D"][:, :2], part["means2D"])
    print("saturating stack: %d solid pixels of %d, %d strict Gaussians of 70; map %.3e; opacities %.3e, means2D %.3e" % (
        solid.sum(), solid.size, strict.sum(), e_map[solid].max(), e_op[strict].max() if strict.any() else 0.0, e_m2[strict].max() if strict.any() else 0.0))
    assert solid.mean() > 0.8 and strict.sum() >= 35
    assert e_map[solid].max() <= MAP_TOL
    assert e_op[strict].max() <= GRAD_TOL and e_m2[strict].max() <= GRAD_TOL


def test_one_splat_and_equal_depths_give_zero():
    """One splat: no pair, the map is exactly 0 and its gradients vanish (up to the rounding of w, which the backward re-derives).  Ten splats at one depth: |z_i - z_j| = 0, the map is exactly 0 (forward
    only: at an exact tie the pairwise form has a kink)."""
    g = _stack(1, 8, 8, 0.7, 2.0, 1)
    r = _run(g, gdist=np.ones((8, 8), np.float32), extras=True)
    assert (r["alpha"] > 0.1).all()
    assert (r["dist"] == 0).all()
    for k, v in r["grads"].items():
        assert np.abs(v).max() <= 1e-5, k  # (64 pixels x one ulp of w <= 1, |g| = 1)
    g = _stack(10, 17, 9, 0.3, 2.0, 2, dz=0.0)
    r = _run(g, extras=True)
    assert (r["alpha"] > 0.5).all()
    assert (r["dist"] == 0).all()
    # ... and two splats against the closed form 2 w_0 w_1 (z_1 - z_0), w from the run's own alpha maps of the two splats alone
    g = _stack(2, 8, 8, 0.5, 2.0, 3, dz=0.5, spread=0.0)
    r = _run(g, extras=True)
    first = _run({k: (v[:1] if k in ("means3D", "colors", "opacities", "scales", "rotations") else v) for k, v in g.items()}, extras=True)["alpha"][0]
    w1 = r["alpha"][0] - first
    closed = 2.0 * first.astype(np.float64) * w1 * 0.5
    assert closed.min() > 0.05
    assert (np.abs(r["dist"] - closed) <= 1e-4 * closed).all(), np.abs(r["dist"] - closed).max()


# ---- structure at the benchmark's sizes -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["config2", "2048"])
def test_structure(name):
    """Finite, never negative, at most alpha^2 (z_max - z_min) over the visible Gaussians (every |z_i - z_j| is), 0 where nothing is blended."""
    g = _scene(name)
    r = _run(g, extras=True)
    d, a = r["dist"], r["alpha"][0]
    z = (g["means3D"].astype(np.float64) @ np.asarray(g["view"], np.float64)[:3, 2] + float(g["view"][3, 2]))[r["radii"] > 0]
    spread = z.max() - z.min()
    print("%s: distortion max %.3e, mean %.3e; depth range of the visible Gaussians %.3f; max dist / (alpha^2 range) %.3e" % (
        name, d.max(), d.mean(), spread, (d / np.maximum(a.astype(np.float64) ** 2 * spread, 1e-30))[a > 0].max()))
    assert np.isfinite(d).all() and (d >= 0).all()
    assert (d > 0).sum() > 1000
    assert (d <= a.astype(np.float64) ** 2 * spread * (1 + 1e-4) + 1e-7).all()
    assert (d[a == 0] == 0).all()


# ---- option off, zero gradient, bits -----------------------------------------------------------------------------------------------------------------------

def test_option_off_zero_gradient_and_reproducibility():
    """With the option on, the image, radii, depth and alpha maps and the gradients of a loss over them have the bits of the run without it; with a zero
    gradient of the map every gradient has the bits of the depth / alpha run; two runs give the same bits; return_distortion=False is the call without
    the keyword."""
    g = _scene("256")
    dpix, gdp, gal, gd = _rand(g, 3, 3), _rand(g, 4), _rand(g, 5), _rand(g, 6)
    kw = dict(dpix=dpix, extras=True, gdepth=gdp, galpha=gal)
    off = _run(g, distortion=False, **kw)
    on = _run(g, **kw)  # the map is returned but takes no part in the loss
    for k in ("img", "radii", "depth", "alpha"):
        np.testing.assert_array_equal(on[k], off[k], err_msg=k)
    _equal_grads(on["grads"], off["grads"])
    zero = _run(g, gdist=np.zeros_like(gd), **kw)
    _equal_grads(zero["grads"], off["grads"])
    np.testing.assert_array_equal(zero["dist"], on["dist"])
    a, b = _run(g, gdist=gd, **kw), _run(g, gdist=gd, **kw)
    np.testing.assert_array_equal(a["dist"], b["dist"])
    _equal_grads(a["grads"], b["grads"])
    assert any(not np.array_equal(a["grads"][k], off["grads"][k]) for k in ("means3D", "opacities", "scales", "rotations", "means2D"))
    np.testing.assert_array_equal(a["grads"]["colors"], off["grads"]["colors"])  # dL/dcolour = w dL/dpixel does not see the map
    # without depth / alpha: the map is the same, and nothing else is returned
    alone = _run(g)
    np.testing.assert_array_equal(alone["dist"], on["dist"])
    np.testing.assert_array_equal(alone["img"], off["img"])
    plain = _run(g, distortion=False, dpix=dpix)
    kwoff = decode(rasterize(settings(g), leaves(g), return_distortion=False), g, False)
    assert len(kwoff) == 2
    np.testing.assert_array_equal(kwoff["color"].cpu().numpy(), plain["img"])


# ---- combinations and host paths ---------------------------------------------------------------------------------------------------------------------------

def test_combinations():
    """Antialiasing, SH colours, precomputed covariances, colours without gradient: the map follows the blend, the gradients stay finite and the
    refusals come before any launch."""
    import torch
    from absgrad_ref import norm_err
    from gps_gaussian_amd import synthetic as S
    g = _scene("256")
    P = g["means3D"].shape[0]
    gd = _rand(g, 21)
    base = _run(g, gdist=gd)
    # SH colours: the same geometry and opacities, so the same map and the same geometry gradients of it
    shs = S.random_shs(P, 16)
    r = _run(g, gdist=gd, shs=shs)
    np.testing.assert_array_equal(r["dist"], base["dist"])
    for k in ("means2D", "opacities", "scales", "rotations"):
        np.testing.assert_array_equal(r["grads"][k], base["grads"][k], err_msg=k)
    assert (r["grads"]["shs"] == 0).all()
    # precomputed covariances
    cov = S.covariances_from(g["scales"], g["rotations"]).astype(np.float32)
    r = _run(g, gdist=gd, cov=cov)
    e = np.abs(r["dist"].astype(np.float64) - base["dist"]).mean() / base["dist"].mean()
    print("cov3D_precomp: map against the scales + rotations run, mean |difference| / mean %.3e, worst pixel %.3e" % (e, norm_err(r["dist"], base["dist"]).max()))
    assert np.isfinite(r["dist"]).all() and (r["dist"] >= 0).all()
    assert e <= 1e-3  # (covariances rounded to fp32 on the host perturb the input by 1e-7: the mean is robust against a flipped decision at a pixel)
    assert np.isfinite(r["grads"]["cov3D_precomp"]).all() and np.abs(r["grads"]["cov3D_precomp"]).max() > 0
    # antialiasing: smaller opacities, another map; finite gradients
    r = _run(g, gdist=gd, aa=True)
    assert np.isfinite(r["dist"]).all() and (r["dist"] >= 0).all() and not np.array_equal(r["dist"], base["dist"])
    for k, v in r["grads"].items():
        assert np.isfinite(v).all() and np.abs(v).max() > 0 or k == "colors", k
    # colours that need no gradient (GSR_FLAG_NO_COLOR_GRAD is a tile-family matter: the VALU records are the same)
    r = _run(g, gdist=gd, color_grad=False)
    assert "colors" not in r["grads"]
    for k in r["grads"]:
        np.testing.assert_array_equal(r["grads"][k], base["grads"][k], err_msg=k)
    # the three refusals, on GPU tensors
    rs, t, dev = settings(g), leaves(g), torch.device("cuda:0")
    for kw, what in ((dict(features=torch.ones(P, 2, device=dev)), "features"), (dict(return_contrib=True), "return_contrib"),
                     (dict(return_absgrad=True), "return_absgrad")):
        with pytest.raises(RuntimeError, match="return_distortion cannot be combined with %s" % what):
            rasterize(rs, t, return_distortion=True, **kw)
    torch.cuda.synchronize()


def test_list_forms(monkeypatch):
    """Both list forms blend in the same order: the same map, bit for bit; the gradients agree to rounding (the record slots may be summed in another order)."""
    g = _scene("256")
    gd = _rand(g, 8)
    res = {}
    for lists in ("direct", "scanned"):
        monkeypatch.setenv("GPSGS_LISTS", lists)
        res[lists] = _run(g, gdist=gd)
    np.testing.assert_array_equal(res["direct"]["dist"], res["scanned"]["dist"])
    assert (res["direct"]["dist"] > 0).any()
    for k in ("opacities", "means2D", "means3D"):
        a, b = res["direct"]["grads"][k], res["scanned"]["grads"][k]
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6 * np.abs(b).max(), err_msg=k)


def test_capacity_repair_gives_the_unforced_bits(monkeypatch):
    """A forward whose first attempt overflows (capacity forced tiny) is repaired in sync mode: the map and the gradients of the repaired view have the
    bits of an unforced run (the totals plane is written again by the repair)."""
    from gps_gaussian_amd import rasterizer as RZ
    g = _scene("256")
    gd = _rand(g, 9)
    ref = _run(g, gdist=gd)
    real = RZ._capacity_for
    calls = []
    monkeypatch.setattr(RZ, "_capacity_for", lambda st, P: (calls.append(1), 1500 if len(calls) == 1 else real(st, P))[1])
    r = _run(g, gdist=gd)
    assert len(calls) >= 2  # the first attempt overflowed and was re-run
    np.testing.assert_array_equal(r["dist"], ref["dist"])
    _equal_grads(r["grads"], ref["grads"])
    assert (r["dist"] > 0).any()


def test_unrepaired_overflow_gives_zeros(monkeypatch):
    """GPSGS_CHECK=none with a capacity far too small: the zero image and a zero map; the backward runs (and does nothing)."""
    from gps_gaussian_amd import rasterizer as RZ
    g = _scene("256")
    monkeypatch.setenv("GPSGS_CHECK", "none")
    monkeypatch.setattr(RZ, "_capacity_for", lambda st, P: 1500)
    r = _run(g, gdist=_rand(g, 10))
    assert (r["img"] == 0).all()
    assert (r["dist"] == 0).all()


def test_empty_and_all_culled_views():
    """P = 0 and a view whose Gaussians are all behind the camera: zero maps; the backward of the culled view runs."""
    g = _stack(20, 17, 9, 0.5, 0.3, 4)
    e = dict(g, **{k: g[k][:0] for k in ("means3D", "colors", "opacities", "scales", "rotations")})
    r = _run(e)
    assert r["dist"].shape == (9, 17) and (r["dist"] == 0).all()
    behind = dict(g, means3D=g["means3D"] * np.array([1.0, 1.0, -1.0], np.float32))
    r = _run(behind, gdist=_rand(g, 12))
    assert (r["radii"] == 0).all()
    assert (r["dist"] == 0).all()


# ---- pts2render ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["batch", "loop"])
def test_pts2render_against_four_render_ex_calls(form, monkeypatch):
    """pts2render(with_distortion=True) at B = 4: 'distortion_pred' has the bits of four render_ex(distortion=True) calls on the same packed rows, the
    image is the plain call's, depth / alpha are written only when asked for, and the map's gradient reaches the source views' points with the bits
    of the four calls' gradients."""
    import torch
    from gps_gaussian_amd import render_api
    from gps_gaussian_amd.pack import pack_views
    monkeypatch.setenv("GPSGS_PTS2RENDER", form)
    B = 4
    bg = [0.2, 0.3, 0.4]
    data = _batch(B)
    out = render_api.pts2render(data, bg, with_distortion=True)
    nv = out["novel_view"]
    dmap = nv["distortion_pred"]
    assert tuple(dmap.shape) == (B, 1, 64, 64) and dmap.dtype == torch.float32 and dmap.requires_grad
    if form == "batch":
        assert "depth_pred" not in nv and "alpha_pred" not in nv
    plain = render_api.pts2render(_batch(B), bg)["novel_view"]["img_pred"]
    np.testing.assert_array_equal(nv["img_pred"].detach().cpu().numpy(), plain.detach().cpu().numpy())
    both = render_api.pts2render(_batch(B), bg, with_depth_alpha=True, with_distortion=True)["novel_view"]
    assert "depth_pred" in both and "alpha_pred" in both
    np.testing.assert_array_equal(both["distortion_pred"].detach().cpu().numpy(), dmap.detach().cpu().numpy())
    wgt = torch.from_numpy(np.random.default_rng(3).standard_normal((B, 1, 64, 64)).astype(np.float32)).cuda()
    (dmap * wgt).sum().backward()

    data2 = _batch(B)
    xyz, rgb, rot, scale, opacity, offsets = pack_views(data2)
    maps = []
    for i, sl, r in render_ex_rows(data2, (xyz, rgb, rot, scale, opacity), offsets, bg, distortion=True):
        assert set(r) == {"img", "depth", "alpha", "distortion"} and tuple(r["distortion"].shape) == (1, 64, 64)
        maps.append(r["distortion"])
    ref = torch.stack(maps)
    assert float(ref.detach().max()) > 0
    np.testing.assert_array_equal(dmap.detach().cpu().numpy(), ref.detach().cpu().numpy())
    (ref * wgt).sum().backward()
    for v in ("lmain", "rmain"):
        a, b = data[v]["xyz"].grad, data2[v]["xyz"].grad
        assert a is not None and float(a.abs().max()) > 0
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
