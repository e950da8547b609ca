"""GPU (-m gpu): the opt-in antialiasing of the rasteriser (include/gpsgs.h GSR_FLAG_ANTIALIAS; rasterize_gaussians / GaussianRasterizer.forward
(antialiasing=True), render_api.render / render_ex / pts2render, RasterSession).

The spec: every visible splat's opacity becomes opacity * k, k = sqrt(max(rho, 2.5e-5)), rho = det(cov0) / det(cov0 + 0.3 I) -- everything else
(conic, radii, bin rects, depth order) unchanged.  Checked by a known answer on the optical axis, by the alpha mass of one splat against the
undilated footprint, against the dense fp64 autograd reference (tests/aa_ref.py) and, on the suite's larger scenes, against the C oracles run with
opacity_eff whose dL/dopacity_eff is chained through the fp64 vector-Jacobian product of k.
"""
import math

import numpy as np
import pytest

from conftest import assert_grad_parity, fragile_bounds, gaussians, oracle_render, simple_scene

from aa_ref import aa_grads_dense, aa_vjp, chain_oracle, opacity_eff
from raster_run import batch_data, batch_with_xyz_grad, leaves, rasterize, render_ex_rows, run_view, scene, settings, to_dev

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4
GRAD_TOL = 1e-3


def _render(g, aa=True, dpix=None, settings_attr=False, keyword=True, **kw):
    """run_view with antialiasing on by default, always with the forward's state (st).  settings_attr: the flag travels as the `antialiasing`
    attribute of a settings object of the newer upstream shape, not as the keyword; keyword=False: the call without the keyword."""
    make = None
    if settings_attr:
        from collections import namedtuple
        from gps_gaussian_amd import rasterizer as RZ
        S = namedtuple("NewerSettings", RZ.GaussianRasterizationSettings._fields + ("antialiasing",))
        make = lambda *args: S(*args, bool(aa))  # noqa: E731
    return run_view(g, dict(img=dpix), aa=aa if keyword and not settings_attr else None, keep_ws=True, make_settings=make, **kw)


def _op_eff(r):
    return r["st"]["conic_opacity"][:, 3].cpu().numpy()


# ---- known answers -----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(params=["valu", "tiles"])
def family(request, monkeypatch):
    monkeypatch.setenv("GPSGS_COMPOSITE", request.param)
    return request.param


def _axis_splat(z, s, o, W=65, fx=100.0, rgb=(0.9, 0.4, 0.2), bg=(0.1, 0.2, 0.3)):
    cam = simple_scene(W, W, fx, bg=bg)
    return dict(cam, **gaussians([[0.0, 0.0, z]], rgb, o, [s, s, s]))


def test_known_answer_on_the_optical_axis(family):
    """An isotropic splat on the optical axis (odd W: the mean lands on a pixel centre): the centre pixel is min(0.99, o sigma^2 / (sigma^2 + 0.3)) rgb
    + T bg, sigma = fx s / z."""
    fx, s, o = 100.0, 0.02, 0.8
    for z in (0.5, 1.0, 2.0, 4.0, 8.0):
        g = _axis_splat(z, s, o, fx=fx)
        r = _render(g)
        sig2 = (fx * s / z) ** 2
        a = min(0.99, o * sig2 / (sig2 + 0.3))
        c = 32
        want = a * np.array(g["colors"][0], np.float64) + (1 - a) * g["bg"].astype(np.float64)
        np.testing.assert_allclose(r["img"][:, c, c], want, rtol=1e-5, err_msg="z=%g" % z)
        plain = _render(g, aa=False)
        ap = min(0.99, o)
        np.testing.assert_allclose(plain["img"][:, c, c], ap * g["colors"][0] + (1 - ap) * g["bg"], rtol=1e-5)
        np.testing.assert_array_equal(r["radii"], plain["radii"])


def test_floor_case_is_visible_and_has_no_covariance_gradient(family):
    """sigma = 0.01 px: rho is below 2.5e-5, k = 0.005 > 1/255 (o = 1): the splat is drawn with alpha 0.005 at its centre pixel only, and
    nothing reaches its covariance: dL/dscales = dL/drotations = 0 exactly, dL/dopacity = 0.005 dL/dopacity_eff."""
    fx, z = 100.0, 2.0
    s = 0.01 * z / fx
    g = _axis_splat(z, s, 1.0, fx=fx)
    rng = np.random.default_rng(1)
    dpix = rng.standard_normal((3, 65, 65)).astype(np.float32)
    r = _render(g, dpix=dpix)
    assert r["radii"][0] > 0
    c = 32
    a = 0.005
    np.testing.assert_allclose(r["img"][:, c, c], a * g["colors"][0] + (1 - a) * g["bg"], rtol=1e-5)
    drawn = np.abs(r["img"] - g["bg"][:, None, None]).max(0) > 0
    assert drawn.sum() == 1 and drawn[c, c]
    np.testing.assert_allclose(_op_eff(r)[0], 0.005, rtol=1e-6)
    gr = r["grads"]
    assert (gr["scales"] == 0).all() and (gr["rotations"] == 0).all()
    g_eff = float(np.dot(dpix[:, c, c], np.asarray(g["colors"][0]) - g["bg"]))  # dL/dalpha at the one pixel (T = 1, nothing behind)
    np.testing.assert_allclose(gr["opacities"][0, 0], 0.005 * g_eff, rtol=1e-5)


def test_alpha_mass_follows_the_undilated_footprint(monkeypatch):
    """One receding splat, sigma from ~2.9 down to 0.8 px, o = 0.5: the summed alpha map is its fp64 per-pixel sum (1e-5), and it follows the
    undilated footprint 2 pi o sigma^2 with AA, the dilated one 2 pi o (sigma^2 + 0.3) without (5 %), each times the kept fraction 1 - 1/(255 o_eff)
    of the alpha >= 1/255 cut."""
    monkeypatch.setenv("GPSGS_COMPOSITE", "valu")
    fx, s, o, W = 100.0, 0.04, 0.5, 65
    ys, xs = np.meshgrid(np.arange(W), np.arange(W), indexing="ij")
    d2 = (xs - 32.0) ** 2 + (ys - 32.0) ** 2
    for z in (1.4, 2.0, 3.0, 5.0):
        g = _axis_splat(z, s, o, W=W, fx=fx, bg=(0.0, 0.0, 0.0))
        sig2 = (fx * s / z) ** 2
        S2 = sig2 + 0.3
        masses = {}
        for aa in (True, False):
            r = _render(g, aa=aa, extras=True)
            oe = o * sig2 / S2 if aa else o
            a = oe * np.exp(-0.5 * d2 / S2)
            a = np.where(a >= 1 / 255, np.minimum(a, 0.99), 0.0)
            mass = float(r["alpha"].astype(np.float64).sum())
            assert abs(mass - a.sum()) <= 1e-5 * a.sum(), (z, aa, mass, a.sum())
            kept = 1.0 - 1.0 / (255.0 * oe)
            foot = 2 * math.pi * o * (sig2 if aa else S2) * kept
            assert abs(mass - foot) <= 0.05 * foot, (z, aa, mass, foot)
            masses[aa] = mass
        if sig2 < 2.0:  # the property: here the two modes differ by far more than the tolerance
            assert masses[False] > 1.1 * masses[True]


# ---- references -----------------------------------------------------------------------------------------------------------------------------------

def _small_scene(seed, n=40, side=48):
    rng = np.random.default_rng(seed)
    cam = simple_scene(side, side, 40.0, bg=(0.2, 0.1, 0.3))
    xyz = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n), rng.uniform(1.5, 3.0, n)], 1)
    scale = np.exp(rng.uniform(np.log(0.002), np.log(0.06), (n, 3)))
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return dict(cam, **gaussians(xyz, rng.uniform(0, 1, (n, 3)), rng.uniform(0.1, 0.95, n), scale, q)), rng


@pytest.mark.parametrize("inputs", ["plain", "shs", "cov3D_precomp"])
def test_against_the_dense_fp64_reference(inputs, family):
    from gps_gaussian_amd import synthetic as S
    g, rng = _small_scene(21)
    P = g["means3D"].shape[0]
    dpix = rng.standard_normal((3, g["H"], g["W"])).astype(np.float32)
    shs = S.random_shs(P, 16) if inputs == "shs" else None
    cov = S.covariances_from(g["scales"], g["rotations"]).astype(np.float32) if inputs == "cov3D_precomp" else None
    r = _render(g, dpix=dpix, shs=shs, cov=cov)
    rimg, rradii, rg = aa_grads_dense(g, dpix, cov3D_precomp=cov, shs=shs, sh_degree=3 if shs is not None else None)
    vis = r["radii"] > 0
    np.testing.assert_array_equal(vis, rradii > 0)
    assert vis.sum() >= P // 2
    # fragile pixels (a branch threshold within 1e-5) from the fp32 oracle run with the kernel's opacity_eff: the only places a decision may differ
    from oracle.gsr_oracle import OracleRasterizer
    o = OracleRasterizer("f32")
    o.forward(g["means3D"], None if shs is not None else g["colors"], _op_eff(r), None if cov is not None else g["scales"],
              None if cov is not None else g["rotations"], g["view"], g["proj"], g["W"], g["H"], g["tanfovx"], g["tanfovy"], g["bg"],
              shs=shs, sh_degree=3, campos=g["campos"], cov3D_precomp=cov)
    solid, touched, _ = fragile_bounds(o, dpix)
    assert np.abs(r["img"] - rimg).max(0)[solid].max() <= RGB_TOL
    assert_grad_parity(r["grads"], {k: rg[k] for k in r["grads"]}, touched, vis)
    if cov is not None:  # dL/dcov3D carries the k term: the same render with opacity_eff held constant is far outside the tolerance
        from oracle.gsr_torch_ref import grads_ref
        held = dict(g, opacities=opacity_eff(g, cov).reshape(-1, 1), cov3D_precomp=cov, scales=None, rotations=None)
        _, _, hg = grads_ref(held, g["W"], g["H"], g["tanfovx"], g["tanfovy"], dpix)
        s = np.abs(rg["cov3D_precomp"]).max()
        assert np.abs(hg["cov3D_precomp"] - rg["cov3D_precomp"]).max() > 10 * GRAD_TOL * s
        assert np.abs(r["grads"]["cov3D_precomp"] - hg["cov3D_precomp"]).max() > 10 * GRAD_TOL * s


def _scene(name):
    from gps_gaussian_amd import synthetic as S
    if name == "config2_at_512":
        return S.make_scene(1024, 600000, render_res=512)
    return scene({"c1_256_30k": "256", "config2_1024_600k": "config2", "hr_2048_600k": "2048"}[name])


@pytest.mark.parametrize("name", ["c1_256_30k", "config2_1024_600k", "config2_at_512", "hr_2048_600k"])
def test_parity_with_the_oracles(name, monkeypatch):
    """Image against the fp32 oracle run with the kernel's opacity_eff (the suite's RGB tolerance away from branch thresholds); every gradient
    against the oracles' chained through the fp64 product of k (the suite's criterion against fp32, quantiles against fp64); opacity_eff itself
    against fp64 opacity * k."""
    monkeypatch.setenv("GPSGS_COMPOSITE", "valu")
    g = _scene(name)
    H, W = g["H"], g["W"]
    rng = np.random.default_rng(31)
    dpix = rng.standard_normal((3, H, W)).astype(np.float32)
    r = _render(g, dpix=dpix)
    vis = r["radii"] > 0
    oe = _op_eff(r)
    oe64 = opacity_eff(dict(g, means3D=g["means3D"][vis], scales=g["scales"][vis], rotations=g["rotations"][vis], opacities=g["opacities"][vis]))
    rel = np.abs(oe[vis] - oe64) / oe64
    assert np.quantile(rel, 0.99) <= 1e-5 and np.abs(oe[vis] - oe64).max() <= 1e-3, (np.quantile(rel, 0.99), np.abs(oe[vis] - oe64).max())
    assert (oe[vis] <= g["opacities"].reshape(-1)[vis]).all()
    sc = dict(g, opacities=oe.reshape(-1, 1).astype(np.float32))
    o, oimg, oradii = oracle_render(sc, "f32")
    np.testing.assert_array_equal(r["radii"], oradii)
    solid, touched, bounds = fragile_bounds(o, dpix)
    err = np.abs(r["img"] - oimg).max(0)
    assert err[solid].max() <= RGB_TOL, err[solid].max()
    og32 = o.backward(dpix)
    vj = aa_vjp(g, og32["opacities"])
    c32 = chain_oracle(og32, vj)
    mine = {k: r["grads"][k] for k in ("means3D", "opacities", "colors", "scales", "rotations", "means2D")}
    # flip bounds: those of dL/dopacity_eff, times k for dL/dopacity, and through |d(op k)/dx| for the shape gradients (one scalar per Gaussian)
    bounds = dict(bounds)
    bvj = aa_vjp(g, bounds["opacities"])
    for k in ("means3D", "scales", "rotations"):
        bounds[k] = bounds[k] + np.abs(bvj[k])
    bounds["opacities"] = np.abs(bvj["opacities"])
    assert_grad_parity(mine, {k: c32[k] for k in mine}, touched, vis, bounds=bounds)
    o64, _, _ = oracle_render(sc, "f64", decisions=o.geom())
    og64 = o64.backward(dpix)
    c64 = chain_oracle(og64, aa_vjp(g, og64["opacities"]))
    for k in mine:
        s = np.abs(c64[k]).max() + 1e-30
        e = np.abs(mine[k] - c64[k]) / (np.abs(c64[k]) + GRAD_TOL * s)
        assert np.quantile(e, 0.99) <= GRAD_TOL, "%s q99 %.3e" % (k, np.quantile(e, 0.99))


# ---- the matrix -----------------------------------------------------------------------------------------------------------------------------------

def test_families_and_list_forms(monkeypatch):
    """Scanned and direct lists give the same bits within a family; the VALU and tile families agree within the suite's tolerance; each is
    antialiased (the records carry opacity_eff)."""
    from gps_gaussian_amd import synthetic as S
    g = S.make_scene(256, 30000)
    rng = np.random.default_rng(41)
    dpix = rng.standard_normal((3, g["H"], g["W"])).astype(np.float32)
    runs = {}
    for fam in ("valu", "tiles"):
        monkeypatch.setenv("GPSGS_COMPOSITE", fam)
        for lists in ("scanned", "direct"):
            monkeypatch.setenv("GPSGS_LISTS", lists)
            runs[fam, lists] = _render(g, dpix=dpix)
            assert bool(runs[fam, lists]["st"]["num_rendered"] > 0)
        a, b = runs[fam, "scanned"], runs[fam, "direct"]
        np.testing.assert_array_equal(a["img"], b["img"])
        for k in a["grads"]:
            np.testing.assert_array_equal(a["grads"][k], b["grads"][k], err_msg="%s %s" % (fam, k))
    v, t = runs["valu", "scanned"], runs["tiles", "scanned"]
    np.testing.assert_array_equal(_op_eff(v), _op_eff(t))
    assert np.abs(v["img"] - t["img"]).max() <= RGB_TOL
    for k in v["grads"]:
        s = np.abs(v["grads"][k]).max() + 1e-30
        e = np.abs(t["grads"][k] - v["grads"][k]) / (np.abs(v["grads"][k]) + GRAD_TOL * s)
        assert np.quantile(e, 0.999) <= GRAD_TOL, k


def test_stage2_gradient_set_is_bit_equal(monkeypatch):
    """Colours without a gradient (GSR_FLAG_NO_COLOR_GRAD, the tile family drops the colour sums): every other gradient equals the full set's bits."""
    from gps_gaussian_amd import synthetic as S
    monkeypatch.setenv("GPSGS_COMPOSITE", "tiles")
    g = S.make_scene(256, 30000)
    dpix = to_dev(np.random.default_rng(42).standard_normal((3, g["H"], g["W"])))
    rs = settings(g)
    out = []
    for col_grad in (True, False):
        t = leaves(g, grad=lambda k: k != "colors" or col_grad)
        img, _ = rasterize(rs, t, antialiasing=True)
        img.backward(dpix)
        out.append({k: t[k].grad.cpu().numpy() for k in ("means3D", "opacities", "scales", "rotations")})
    for k in out[0]:
        np.testing.assert_array_equal(out[0][k], out[1][k], err_msg=k)
    assert np.abs(out[0]["opacities"]).max() > 0


def test_depth_alpha_maps_with_antialiasing(monkeypatch):
    """The maps of an antialiased view are the R and G channels of an antialiased plain run with colours (z, 1, 0) and background 0; the image
    equals the antialiased image without the maps (same VALU family)."""
    from gps_gaussian_amd import synthetic as S
    monkeypatch.setenv("GPSGS_COMPOSITE", "valu")
    g = S.make_scene(256, 30000)
    r = _render(g, extras=True, bg=(0.3, 0.2, 0.1))
    z = r["st"]["depth"].cpu().numpy()
    zc = np.stack([z, np.ones_like(z), np.zeros_like(z)], 1).astype(np.float32)
    p = _render(g, colors=zc, bg=(0.0, 0.0, 0.0))
    np.testing.assert_array_equal(r["depth"][0], p["img"][0])
    np.testing.assert_array_equal(r["alpha"][0], p["img"][1])
    np.testing.assert_array_equal(r["img"], _render(g, bg=(0.3, 0.2, 0.1))["img"])
    plain = _render(g, aa=False, extras=True, bg=(0.3, 0.2, 0.1))
    assert r["alpha"].sum() < plain["alpha"].sum()  # thinner splats: less coverage


def test_invariants(family):
    """radii bit-equal with AA on and off; R with AA <= R without (tau from opacity_eff: lists only get shorter); antialiasing=False and a settings
    object with antialiasing=False are bit-identical to the call without the keyword; a truthy settings attribute is the keyword."""
    from gps_gaussian_amd import synthetic as S
    g = S.make_scene(256, 30000)
    dpix = np.random.default_rng(51).standard_normal((3, g["H"], g["W"])).astype(np.float32)
    on = _render(g, dpix=dpix)
    off = _render(g, aa=False, dpix=dpix)
    base = _render(g, dpix=dpix, keyword=False)
    attr_off = _render(g, aa=False, dpix=dpix, settings_attr=True)
    attr_on = _render(g, aa=True, dpix=dpix, settings_attr=True)
    np.testing.assert_array_equal(on["radii"], off["radii"])
    assert on["st"]["num_rendered"] <= off["st"]["num_rendered"]
    assert on["st"]["num_rendered"] < off["st"]["num_rendered"]  # this cloud has splats whose opacity_eff drops below what their box was
    for other in (base, attr_off):
        np.testing.assert_array_equal(off["img"], other["img"])
        for k in off["grads"]:
            np.testing.assert_array_equal(off["grads"][k], other["grads"][k], err_msg=k)
    np.testing.assert_array_equal(on["img"], attr_on["img"])
    for k in on["grads"]:
        np.testing.assert_array_equal(on["grads"][k], attr_on["grads"][k], err_msg=k)
    assert np.abs(on["img"] - off["img"]).max() > 1e-2


def test_no_gaussians(family):
    cam = simple_scene(64, 48, 40.0)
    g = dict(cam, **gaussians(np.zeros((0, 3)), [1, 1, 1], 0.5, 0.1))
    r = _render(g, bg=(0.5, 0.5, 0.5))
    assert (r["img"] == 0).all() and r["img"].shape == (3, 48, 64)


def test_capacity_repair_keeps_the_flag(monkeypatch):
    from gps_gaussian_amd import rasterizer as RZ
    from gps_gaussian_amd import synthetic as S
    monkeypatch.setenv("GPSGS_LISTS", "scanned")
    g = S.make_uniform_cloud(5000, 128, 96, seed=9, scale_med=0.05)
    dpix = np.random.default_rng(61).standard_normal((3, g["H"], g["W"])).astype(np.float32)
    ref = _render(g, dpix=dpix)
    calls = []
    real = RZ._capacity_for

    def tiny_first(st, P):
        calls.append(1)
        return 1024 if len(calls) == 1 else real(st, P)

    monkeypatch.setattr(RZ, "_capacity_for", tiny_first)
    r = _render(g, dpix=dpix)
    assert len(calls) >= 2
    np.testing.assert_array_equal(r["img"], ref["img"])
    for k in r["grads"]:
        np.testing.assert_array_equal(r["grads"][k], ref["grads"][k], err_msg=k)
    monkeypatch.setattr(RZ, "_capacity_for", real)
    assert np.abs(r["img"] - _render(g, aa=False)["img"]).max() > 1e-3


@pytest.mark.parametrize("form", ["batch", "loop"])
def test_pts2render_batch_of_4_against_four_render_ex_calls(form, monkeypatch):
    import torch
    from gps_gaussian_amd import render_api
    from gps_gaussian_amd.pack import pack_views
    monkeypatch.setenv("GPSGS_PTS2RENDER", form)
    monkeypatch.setenv("GPSGS_COMPOSITE", "valu")
    B = 4
    data = batch_with_xyz_grad(B)
    bg = [0.2, 0.3, 0.4]
    nv = render_api.pts2render(data, bg, antialiasing=True)["novel_view"]
    rng = np.random.default_rng(71)
    gi = torch.from_numpy(rng.standard_normal((B, 3, 64, 64)).astype(np.float32)).cuda()
    (nv["img_pred"] * gi).sum().backward()
    g_batch = [data[v]["xyz"].grad.clone() for v in ("lmain", "rmain")]
    data2 = batch_with_xyz_grad(B)
    *packed, offsets = pack_views(data2)
    loss = 0
    for i, sl, r in render_ex_rows(data2, packed, offsets, bg, antialiasing=True):
        np.testing.assert_array_equal(nv["img_pred"][i].detach().cpu().numpy(), r["img"].detach().cpu().numpy())
        loss = loss + (r["img"] * gi[i]).sum()
    loss.backward()
    for v, gbat in zip(("lmain", "rmain"), g_batch):
        gref = data2[v]["xyz"].grad
        s = float(gref.abs().max())
        assert s > 0
        assert float((gbat - gref).abs().max()) <= 1e-6 * s, v
    plain = render_api.pts2render(batch_data(B), bg)["novel_view"]["img_pred"]
    assert float((plain.detach() - nv["img_pred"].detach()).abs().max()) > 1e-3


def test_raster_session_equals_the_dropin(family):
    import torch
    from gps_gaussian_amd.session import RasterSession
    from gps_gaussian_amd import synthetic as S
    g = S.make_scene(256, 30000)
    P = g["means3D"].shape[0]
    dev = torch.device("cuda:0")
    dpix = np.random.default_rng(81).standard_normal((3, g["H"], g["W"])).astype(np.float32)
    ref = _render(g, dpix=dpix)
    t = {k: torch.from_numpy(np.ascontiguousarray(g[k], dtype=np.float32)).to(dev) for k in ("means3D", "colors", "opacities", "scales", "rotations",
                                                                                             "view", "proj", "bg")}
    s = RasterSession(P, g["W"], g["H"], dev, antialiasing=True)
    color, radii = s.forward(t["means3D"], t["colors"], t["opacities"], t["scales"], t["rotations"], t["view"], t["proj"], t["bg"], g["tanfovx"],
                             g["tanfovy"])
    G = s.backward(torch.from_numpy(dpix).to(dev))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(color.cpu().numpy(), ref["img"])
    np.testing.assert_array_equal(radii.cpu().numpy(), ref["radii"])
    for k in ("means3D", "colors", "opacities", "scales", "rotations", "means2D"):
        np.testing.assert_array_equal(G[k].cpu().numpy().reshape(ref["grads"][k].shape), ref["grads"][k], err_msg=k)
