"""GPU (-m gpu): the opt-in per-Gaussian contribution statistics of the rasteriser (include/gpsgs.h GsrContrib;
rasterizer.rasterize_gaussians(return_contrib=True); render_api.render_ex(contrib=True); render_api.pts2render(with_contrib=True)).

The spec: a (pixel, Gaussian) pair is blended when the forward adds the Gaussian's colour to the pixel; its weight is w = alpha T, the weight of the
image, the alpha map and the feature maps.  contrib_weight = sum_p w, contrib_max = max_p w, contrib_pixels = #blended pixels.  Checked against a
replay of the fp32 oracle's blend (tests/contrib_ref.py) and against identities the renderer's other outputs must satisfy.
"""
import numpy as np
import pytest

from conftest import fragile_bounds
from raster_run import RGB_TOL, batch as _batch, check_contrib_structure as _check_structure, close_each as _close, decode, leaves, rasterize
from raster_run import render_ex_rows, run_view, scene as _scene, settings, small as _small, valu_fixture

pytestmark = pytest.mark.gpu

_valu = valu_fixture()  # the plain runs the statistics runs are compared with use the VALU family too (the statistics runs always do)


def _run(g, contrib=True, dpix=None, gfeat=None, **kw):
    """run_view with the statistics on by default (+ backward of sum(img * dpix) + sum(feat * gfeat) when given)."""
    return run_view(g, dict(img=dpix, feat=gfeat), contrib=contrib, **kw)


# ---- against the oracle's blend -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("aa", [False, True], ids=["plain", "aa"])
@pytest.mark.parametrize("name", ["96x64", "256"])
def test_against_the_oracle_blend(name, aa):
    """Untouched Gaussians (no fragile pixel takes them in): pixel counts equal, sum and max within the suite's RGB tolerance.  A Gaussian a fragile
    pixel takes in may differ by one pixel and up to 0.99 of weight per fragile pixel inside its rect."""
    from contrib_ref import contrib_stats, fragile_in_rect
    from oracle.gsr_oracle import OracleRasterizer
    g = _scene(name)
    r = _run(g, aa=aa, keep_ws=aa)
    _check_structure(r)
    op = r["st"]["conic_opacity"][:, 3].cpu().numpy() if aa else g["opacities"]  # antialiasing: the kernel's compensated opacity, as the image sees it
    o = OracleRasterizer("f32")
    _, oradii = o.forward(g["means3D"], g["colors"], op, g["scales"], g["rotations"], g["view"], g["proj"], g["W"], g["H"], g["tanfovx"],
                          g["tanfovy"], g["bg"])
    np.testing.assert_array_equal(r["radii"] > 0, oradii > 0)
    rw, rm, rn = contrib_stats(o)
    solid, touched, _ = fragile_bounds(o)
    nf = fragile_in_rect(o, solid)
    assert (rn > 0).sum() > 100 and (~touched & (rn > 0)).sum() > 100
    ok = ~touched
    np.testing.assert_array_equal(r["n"][ok], rn[ok])
    assert _close(r["w"][ok], rw[ok]).all(), np.abs(r["w"][ok] - rw[ok]).max()
    assert _close(r["m"][ok], rm[ok]).all(), np.abs(r["m"][ok] - rm[ok]).max()
    t = touched
    assert (np.abs(r["n"][t] - rn[t]) <= nf[t]).all()
    assert (np.abs(r["w"][t] - rw[t]) <= 0.99 * nf[t] + RGB_TOL * np.abs(rw[t]) + 1e-7).all()


# ---- identities at the benchmark's sizes ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["config2", "2048"])
def test_identities(name):
    """The image has the bits of a plain VALU render; contrib_weight is the feature gradient for features = ones with dL/dfeat = 1; the weights add up
    to the alpha map; max <= min(0.99, sum); the three agree on who contributes; culled Gaussians get zeros."""
    g = _scene(name)
    P = g["means3D"].shape[0]
    plain = _run(g, contrib=False)
    r = _run(g, extras=True)
    np.testing.assert_array_equal(r["img"], plain["img"])
    np.testing.assert_array_equal(r["radii"], plain["radii"])
    _check_structure(r)
    assert (r["n"] > 0).sum() > P // 10
    s_w, s_a = float(r["w"].astype(np.float64).sum()), float(r["alpha"].astype(np.float64).sum())
    assert abs(s_w - s_a) <= 1e-5 * s_a
    H, W = g["H"], g["W"]
    f = _run(g, contrib=False, feats=np.ones((P, 1), np.float32), gfeat=np.ones((1, H, W), np.float32))
    gfe = f["grads"]["features"][:, 0]
    assert _close(r["w"], gfe, 1e-4, 1e-7).all(), np.abs(r["w"] - gfe).max()


# ---- no side effects ------------------------------------------------------------------------------------------------------------------------------

def test_gradients_and_outputs_unchanged_and_reproducible():
    """Gradients with the statistics on are bit-identical to those without (depth / alpha maps too); the statistics have the same bits run to run."""
    g = _scene("256")
    rng = np.random.default_rng(3)
    dpix = rng.standard_normal((3, g["H"], g["W"])).astype(np.float32)
    a = _run(g, contrib=False, dpix=dpix, extras=True)
    b = _run(g, contrib=True, dpix=dpix, extras=True)
    c = _run(g, contrib=True, dpix=dpix, extras=True)
    for k in ("img", "radii", "depth", "alpha"):
        np.testing.assert_array_equal(a[k], b[k])
    for k in a["grads"]:
        np.testing.assert_array_equal(a["grads"][k], b["grads"][k])
    for k in ("w", "m", "n"):
        np.testing.assert_array_equal(b[k], c[k])
    _check_structure(b)


def test_option_off_call_unchanged():
    """return_contrib=False is the call without the keyword: same outputs, same count."""
    g = _scene("96x64")
    rs, t = settings(g), leaves(g)
    x = decode(rasterize(rs, t), g, False)
    y = decode(rasterize(rs, t, return_contrib=False), g, False)
    assert len(x) == len(y) == 2
    np.testing.assert_array_equal(x["color"].cpu().numpy(), y["color"].cpu().numpy())


# ---- combinations ---------------------------------------------------------------------------------------------------------------------------------

def test_combinations():
    """shs and pinned-CPU cameras with camera gradients leave the blend as it is: the statistics keep the plain call's bits; cov3D_precomp and
    antialiasing keep the identities; features are refused before anything is launched."""
    import torch
    from gps_gaussian_amd import synthetic as S
    g = _scene("256")
    P = g["means3D"].shape[0]
    base = _run(g)
    shs = S.random_shs(P, 16)
    rng = np.random.default_rng(4)
    dpix = rng.standard_normal((3, g["H"], g["W"])).astype(np.float32)
    r = _run(g, shs=shs, cam=True, pinned=True, dpix=dpix)
    for k in ("w", "m", "n"):
        np.testing.assert_array_equal(r[k], base[k])
    assert np.isfinite(r["grads"]["view"]).all() and np.abs(r["grads"]["view"]).max() > 0
    cov = S.covariances_from(g["scales"], g["rotations"]).astype(np.float32)
    for kw in (dict(cov=cov), dict(aa=True), dict(cov=cov, aa=True)):
        c = _run(g, extras=True, **kw)
        _check_structure(c)
        s_w, s_a = float(c["w"].astype(np.float64).sum()), float(c["alpha"].astype(np.float64).sum())
        assert abs(s_w - s_a) <= 1e-5 * s_a
    with pytest.raises(RuntimeError, match="features"):
        _run(g, feats=np.ones((P, 2), np.float32))
    torch.cuda.synchronize()


# ---- edge cases -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lists", ["direct", "scanned"])
def test_list_forms(lists, monkeypatch):
    """Both list forms give the same statistics (same blend, same slots)."""
    g = _scene("256")
    ref = _run(g)
    monkeypatch.setenv("GPSGS_LISTS", lists)
    r = _run(g)
    np.testing.assert_array_equal(r["img"], ref["img"])
    np.testing.assert_array_equal(r["n"], ref["n"])
    assert _close(r["w"], ref["w"], 1e-6, 0).all() and _close(r["m"], ref["m"], 1e-6, 0).all()
    _check_structure(r)


def test_capacity_repair_fills_the_statistics(monkeypatch):
    """A forward whose first attempt overflows (capacity forced tiny) is repaired in sync mode: the statistics of the repair run are written."""
    from gps_gaussian_amd import rasterizer as RZ
    g = _scene("256")
    ref = _run(g)
    real = RZ._capacity_for
    calls = []
    monkeypatch.setattr(RZ, "_capacity_for", lambda st, P: (calls.append(1), 1500 if len(calls) == 1 else real(st, P))[1])
    r = _run(g)
    assert len(calls) >= 2  # the first attempt overflowed and was re-run
    for k in ("img", "w", "m", "n"):
        np.testing.assert_array_equal(r[k], ref[k])


def test_unrepaired_overflow_gives_zeros(monkeypatch):
    """GPSGS_CHECK=none with a capacity far too small: the zero image, and zero statistics."""
    from gps_gaussian_amd import rasterizer as RZ
    g = _scene("256")
    monkeypatch.setenv("GPSGS_CHECK", "none")
    monkeypatch.setattr(RZ, "_capacity_for", lambda st, P: 1500)
    r = _run(g)
    assert (r["img"] == 0).all()
    assert (r["w"] == 0).all() and (r["m"] == 0).all() and (r["n"] == 0).all()


def test_empty_and_all_culled_views():
    """P = 0 gives empty statistics; a view whose Gaussians are all behind the camera gives zeros."""
    g = _small(n=200)
    e = dict(g, **{k: g[k][:0] for k in ("means3D", "colors", "opacities", "scales", "rotations")})
    r = _run(e)
    assert r["w"].shape == (0,) and r["n"].shape == (0,)
    behind = dict(g, means3D=g["means3D"] * np.array([1.0, 1.0, -1.0], np.float32))
    r = _run(behind)
    assert (r["radii"] == 0).all()
    assert (r["w"] == 0).all() and (r["m"] == 0).all() and (r["n"] == 0).all()


# ---- pts2render -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["batch", "loop"])
def test_pts2render_against_four_render_ex_calls(form, monkeypatch):
    """pts2render(with_contrib=True) at B = 4: the statistics have the bits of four render_ex(contrib=True) calls on the same packed rows; every valid
    source pixel holds its own Gaussian's statistics, every invalid one 0; the image is unchanged and the backward still runs."""
    import torch
    from gps_gaussian_amd import render_api
    from gps_gaussian_amd.pack import pack_views
    monkeypatch.setenv("GPSGS_PTS2RENDER", form)
    B = 4
    bg = [0.2, 0.3, 0.4]
    data = _batch(B)
    out = render_api.pts2render(data, bg, with_contrib=True)
    img = out["novel_view"]["img_pred"]
    plain = render_api.pts2render(_batch(B), bg)["novel_view"]["img_pred"]
    np.testing.assert_array_equal(img.detach().cpu().numpy(), plain.detach().cpu().numpy())
    img.sum().backward()
    assert data["lmain"]["xyz"].grad is not None

    data2 = _batch(B)
    xyz, rgb, rot, scale, opacity, offsets, rows = pack_views(data2, return_rows=True)
    keys = ("contrib_weight", "contrib_max", "contrib_pixels")
    stats = {k: [] for k in keys}
    for i, sl, r in render_ex_rows(data2, (xyz, rgb, rot, scale, opacity), offsets, bg, contrib=True):
        for k in keys:
            assert tuple(r[k].shape) == (sl.stop - sl.start,)
            stats[k].append(r[k])
    rows = rows.cpu().numpy()
    for k in keys:
        packed = torch.cat(stats[k]).cpu().numpy()
        assert (packed > 0).sum() > 100
        for v, view in enumerate(("lmain", "rmain")):
            m = out[view][k]
            assert tuple(m.shape) == (B, 1) + tuple(data2[view]["img"].shape[2:]) and not m.requires_grad
            m = m.cpu().numpy().reshape(B, -1)
            valid = data2[view]["pts_valid"].cpu().numpy().reshape(B, -1)
            rv = rows[:, v]
            np.testing.assert_array_equal(rv >= 0, valid)
            np.testing.assert_array_equal(m[valid], packed[rv[valid]])
            assert (m[~valid] == 0).all()


def test_pts2render_with_contrib_reads_nothing_back():
    """The batch form with with_contrib adds no host synchronisation: the maps come from device index ops."""
    import torch
    from gps_gaussian_amd import render_api
    render_api.pts2render(_batch(2), [0, 0, 0], with_contrib=True)  # warm-up: capacities learnt
    data = _batch(2)
    with torch.cuda.stream(torch.cuda.Stream()):  # set_sync_debug_mode does not police the legacy default stream
        torch.cuda.set_sync_debug_mode("error")
        try:
            w = render_api.pts2render(data, [0, 0, 0], with_contrib=True)["lmain"]["contrib_weight"]
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert float(w.max()) > 0
