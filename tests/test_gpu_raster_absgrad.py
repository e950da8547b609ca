"""GPU (-m gpu): the opt-in absolute screen-space gradient of the rasteriser (include/gpsgs.h GsrAbsGrad;
rasterizer.rasterize_gaussians(return_absgrad=True); render_api.render_ex(absgrad=True); render_api.pts2render(with_absgrad=True)).

The spec: absgrad[i] = sum over pixels p of (|t_x(p, i)|, |t_y(p, i)|), where the signed sums of the same terms are means2D.grad[i, :2].  Checked
against two references that do not reuse the kernel's formula (tests/absgrad_ref.py: a replay of the fp32 oracle's blend, and the per-pixel Jacobian
of the fp64 torch renderer) and against identities the renderer's other outputs must satisfy.
"""
import numpy as np
import pytest

from conftest import assert_grad_parity, fragile_bounds
from raster_run import batch as _batch, check_absgrad_structure as _check_structure, decode, leaves, pad as _pad, rasterize, render_ex_rows, run_view
from raster_run import scene as _scene, settings, small as _small, valu_fixture

pytestmark = pytest.mark.gpu

_valu = valu_fixture()  # the plain runs the absgrad runs are compared with use the VALU family too (the absgrad runs always do)


def _run(g, absgrad=True, dpix=None, gdepth=None, galpha=None, dpix2=None, **kw):
    """run_view with absgrad on by default and features that need no gradient; the backward of sum(img * dpix) (+ sum(depth * gdepth) +
    sum(alpha * galpha)); dpix2: a second backward over the retained graph."""
    cot = dict(img=dpix, depth=gdepth, alpha=galpha)
    return run_view(g, cot, dict(cot, img=dpix2) if dpix2 is not None else None, absgrad=absgrad, feat_grad=False, **kw)


def _dpix(g, seed):
    return np.random.default_rng(seed).standard_normal((3, g["H"], g["W"])).astype(np.float32)


# ---- against the two references -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("aa", [False, True], ids=["plain", "aa"])
@pytest.mark.parametrize("name", ["96x64", "256"])
def test_against_the_oracle_replay(name, aa):
    """The suite's gradient criterion (conftest.assert_grad_parity, unchanged), absgrad in place of the screen-space gradient and the replay of the fp32
    oracle's blend in place of the oracle's backward.  The flip budget of means2D is a valid budget for the absolute sum too: flip_bound adds the
    magnitudes of the per-pixel terms, and ||a| - |b|| <= |a - b|."""
    from absgrad_ref import absgrad_replay
    from oracle.gsr_oracle import OracleRasterizer
    g = _scene(name)
    dpix = _dpix(g, 11)
    r = _run(g, dpix=dpix, aa=aa, keep_ws=aa)
    _check_structure(r)
    op = r["st"]["conic_opacity"][:, 3].cpu().numpy() if aa else g["opacities"]  # antialiasing: the kernel's compensated opacity, as the image sees it
    o = OracleRasterizer("f32")
    _, oradii = o.forward(g["means3D"], g["colors"], op, g["scales"], g["rotations"], g["view"], g["proj"], g["W"], g["H"], g["tanfovx"],
                          g["tanfovy"], g["bg"])
    np.testing.assert_array_equal(r["radii"] > 0, oradii > 0)
    ref, _ = absgrad_replay(o, dpix)
    _, touched, bounds = fragile_bounds(o, dpix)
    visible = oradii > 0
    strict = visible & ~touched
    e = np.abs(r["abs"] - ref) / (np.abs(ref) + 1e-3 * np.abs(ref).max())
    print("%s %s: strict set %.4f of the visible cloud, max normalised error on it %.3e, over all %.3e" % (
        name, "aa" if aa else "plain", strict.sum() / max(1, visible.sum()), e[strict].max(), e.max()))
    assert (strict & (ref > 0).any(axis=1)).sum() > 100
    assert_grad_parity({"means2D": _pad(r["abs"])}, {"means2D": _pad(ref)}, touched, visible, bounds=bounds)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_against_the_per_pixel_jacobian(seed):
    """24 x 16 pixels, 40 Gaussians: autograd through the fp64 renderer, one backward per pixel.  These scenes have no fragile pixel
    (tests/test_absgrad_ref.py asserts it), so every Gaussian is held to the suite's tolerance."""
    from absgrad_ref import absgrad_jacobian, norm_err, tiny_scene
    g = tiny_scene(seed)
    dpix = _dpix(g, 100 + seed)
    r = _run(g, dpix=dpix)
    ref, sg = absgrad_jacobian(g, dpix)
    e = norm_err(r["abs"], ref)
    print("seed %d: absgrad vs Jacobian, max normalised error %.3e; signed %.3e" % (seed, e.max(), norm_err(r["grads"]["means2D"][:, :2], sg).max()))
    assert (ref > 0).any(axis=1).sum() >= 10
    assert (e <= 1e-3).all()
    assert (r["abs"][r["radii"] == 0] == 0).all()


# ---- identities at the benchmark's sizes ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["config2", "2048"])
def test_identities(name):
    g = _scene(name)
    P, H, W = g["means3D"].shape[0], g["H"], g["W"]
    dpix = _dpix(g, 21)
    r = _run(g, dpix=dpix)
    a, gm = r["abs"], r["grads"]["means2D"][:, :2]
    _check_structure(r)  # finite, non-negative, zero where culled, |grad| <= absgrad at the suite's gradient tolerance
    big = np.abs(gm) > 1e-6 * np.abs(gm).max()  # (the floor keeps flushed denormals out)
    assert (a[big] > 0).all()
    assert (a > 0).any(axis=1).sum() > P // 10
    # every operation is sign-symmetric, and scales with dpix (equal bits expected except where denormals flush)
    np.testing.assert_array_equal(_run(g, dpix=-dpix)["abs"], a)
    a2 = _run(g, dpix=2 * dpix)["abs"]
    assert (np.abs(a2 - 2 * a) <= 1e-6 * 2 * a).all()
    # one pixel: one term per Gaussian, so the absolute sum IS the magnitude of the signed one (the two factor the same products differently)
    one = np.zeros_like(dpix)
    one[:, H // 2, W // 2] = (0.7, -1.3, 0.4)
    s = _run(g, dpix=one)
    ref = np.abs(s["grads"]["means2D"][:, :2])
    assert (ref > 0).any()
    assert (np.abs(s["abs"] - ref) <= 1e-4 * ref + 1e-6 * ref.max()).all(), np.abs(s["abs"] - ref).max()
    # ... and with the depth / alpha maps' gradients in that pixel (the EXTRA + ABSGRAD instantiation, which the references do not reach)
    gd, ga = np.zeros((1, H, W), np.float32), np.zeros((1, H, W), np.float32)
    gd[0, H // 2, W // 2], ga[0, H // 2, W // 2] = 0.3, -0.8
    s = _run(g, dpix=one, extras=True, gdepth=gd, galpha=ga)
    ref = np.abs(s["grads"]["means2D"][:, :2])
    assert (ref > 0).any()
    assert (np.abs(s["abs"] - ref) <= 1e-4 * ref + 1e-6 * ref.max()).all(), np.abs(s["abs"] - ref).max()
    plain = _run(g, dpix=one)["grads"]["means2D"][:, :2]
    assert not np.array_equal(np.abs(plain), ref)  # (the maps' gradients did enter dL/dalpha)


# ---- no side effects ------------------------------------------------------------------------------------------------------------------------------

def test_outputs_and_gradients_unchanged_and_reproducible():
    """With return_absgrad the image, radii, maps and EVERY gradient are bit-identical to the same call without it; absgrad has the same bits run to
    run; it is all zeros before any backward."""
    g = _scene("256")
    dpix = _dpix(g, 3)
    rng = np.random.default_rng(31)
    gd, ga = (rng.standard_normal((1, g["H"], g["W"])).astype(np.float32) for _ in range(2))
    for kw in (dict(), dict(extras=True, gdepth=gd, galpha=ga)):
        a = _run(g, absgrad=False, dpix=dpix, **kw)
        b = _run(g, dpix=dpix, **kw)
        c = _run(g, dpix=dpix, **kw)
        for k in ("img", "radii") + (("depth", "alpha") if kw else ()):
            np.testing.assert_array_equal(a[k], b[k])
        assert set(a["grads"]) == set(b["grads"])
        for k in a["grads"]:
            np.testing.assert_array_equal(a["grads"][k], b["grads"][k])
        assert (b["abs0"] == 0).all()
        assert (b["abs"] > 0).any()
        np.testing.assert_array_equal(b["abs"], c["abs"])
        _check_structure(b)


def test_backward_overwrites_in_place():
    """Two backwards over a retained graph with different dL/dpixel leave exactly what a fresh run with the second one gives (no accumulation)."""
    g = _scene("256")
    d1, d2 = _dpix(g, 5), _dpix(g, 6)
    twice = _run(g, dpix=d1, dpix2=d2)
    fresh = _run(g, dpix=d2)
    first = _run(g, dpix=d1)
    np.testing.assert_array_equal(twice["abs"], fresh["abs"])
    np.testing.assert_array_equal(twice["grads"]["means2D"], fresh["grads"]["means2D"])
    assert not np.array_equal(first["abs"], fresh["abs"])


def test_option_off_call_unchanged():
    """return_absgrad=False is the call without the keyword: same outputs, same count."""
    g = _scene("96x64")
    rs, t = settings(g), leaves(g)
    x = decode(rasterize(rs, t), g, False)
    y = decode(rasterize(rs, t, return_absgrad=False), g, False)
    assert len(x) == len(y) == 2
    np.testing.assert_array_equal(x["color"].cpu().numpy(), y["color"].cpu().numpy())


# ---- combinations ---------------------------------------------------------------------------------------------------------------------------------

def test_combinations():
    """Every combination leaves the other gradients their bits and keeps the identities; what does not change the blend keeps absgrad's bits;
    features are refused before anything is launched."""
    import torch
    from gps_gaussian_amd import synthetic as S
    g = _scene("256")
    P = g["means3D"].shape[0]
    dpix = _dpix(g, 4)
    base = _run(g, dpix=dpix)
    _check_structure(base)
    # SH colours, pinned-CPU cameras, camera gradients
    shs = S.random_shs(P, 16)
    kw = dict(shs=shs, cam=True, pinned=True)
    r, p = _run(g, dpix=dpix, **kw), _run(g, absgrad=False, dpix=dpix, **kw)
    for k in p["grads"]:
        np.testing.assert_array_equal(r["grads"][k], p["grads"][k])
    assert np.isfinite(r["grads"]["view"]).all() and np.abs(r["grads"]["view"]).max() > 0
    _check_structure(r)
    assert (r["abs"] > 0).any()
    # precomputed covariances (with and without antialiasing)
    cov = S.covariances_from(g["scales"], g["rotations"]).astype(np.float32)
    for kw in (dict(cov=cov), dict(cov=cov, aa=True)):
        r, p = _run(g, dpix=dpix, **kw), _run(g, absgrad=False, dpix=dpix, **kw)
        for k in p["grads"]:
            np.testing.assert_array_equal(r["grads"][k], p["grads"][k])
        _check_structure(r)
        assert (r["abs"] > 0).any()
    # colours that need no gradient: the blend and dL/dalpha are the same
    r = _run(g, dpix=dpix, color_grad=False)
    assert "colors" not in r["grads"]
    np.testing.assert_array_equal(r["abs"], base["abs"])
    np.testing.assert_array_equal(r["grads"]["means2D"], base["grads"]["means2D"])
    # depth / alpha gradients present: they enter dL/dalpha
    rng = np.random.default_rng(41)
    gd, ga = (rng.standard_normal((1, g["H"], g["W"])).astype(np.float32) for _ in range(2))
    r = _run(g, dpix=dpix, extras=True, gdepth=gd, galpha=ga)
    _check_structure(r)
    assert not np.array_equal(r["abs"], base["abs"])
    # with the contribution statistics: both keep the bits they have alone (the absgrad tail reuses the dead contribution tail)
    both = _run(g, dpix=dpix, contrib=True)
    only = _run(g, absgrad=False, dpix=dpix, contrib=True)
    for k in ("w", "m", "n", "img"):
        np.testing.assert_array_equal(both[k], only[k])
    for k in only["grads"]:
        np.testing.assert_array_equal(both["grads"][k], only["grads"][k])
    np.testing.assert_array_equal(both["abs"], base["abs"])
    with pytest.raises(RuntimeError, match="features"):
        _run(g, dpix=dpix, feats=np.ones((P, 2), np.float32))
    torch.cuda.synchronize()


# ---- edge cases -----------------------------------------------------------------------------------------------------------------------------------

def test_list_forms(monkeypatch):
    """Both list forms agree (same blend, same slots; rtol as for the contribution statistics)."""
    g = _scene("256")
    dpix = _dpix(g, 8)
    res = {}
    for lists in ("direct", "scanned"):
        monkeypatch.setenv("GPSGS_LISTS", lists)
        res[lists] = _run(g, dpix=dpix)
        _check_structure(res[lists])
    np.testing.assert_array_equal(res["direct"]["img"], res["scanned"]["img"])
    np.testing.assert_allclose(res["direct"]["abs"], res["scanned"]["abs"], rtol=1e-6, atol=0)
    assert (res["direct"]["abs"] > 0).any()


def test_capacity_repair_gives_the_unforced_bits(monkeypatch):
    """A forward whose first attempt overflows (capacity forced tiny) is repaired in sync mode: the backward of the repaired view gives the bits of an
    unforced run."""
    from gps_gaussian_amd import rasterizer as RZ
    g = _scene("256")
    dpix = _dpix(g, 9)
    ref = _run(g, dpix=dpix)
    real = RZ._capacity_for
    calls = []
    monkeypatch.setattr(RZ, "_capacity_for", lambda st, P: (calls.append(1), 1500 if len(calls) == 1 else real(st, P))[1])
    r = _run(g, dpix=dpix)
    assert len(calls) >= 2  # the first attempt overflowed and was re-run
    for k in ("img", "abs"):
        np.testing.assert_array_equal(r[k], ref[k])
    assert (r["abs"] > 0).any()


def test_unrepaired_overflow_gives_zeros(monkeypatch):
    """GPSGS_CHECK=none with a capacity far too small: the zero image, and after the backward a zero absgrad."""
    from gps_gaussian_amd import rasterizer as RZ
    g = _scene("256")
    monkeypatch.setenv("GPSGS_CHECK", "none")
    monkeypatch.setattr(RZ, "_capacity_for", lambda st, P: 1500)
    r = _run(g, dpix=_dpix(g, 10))
    assert (r["img"] == 0).all()
    assert (r["abs"] == 0).all()


def test_empty_and_all_culled_views():
    """P = 0 gives shape (0, 2); a view whose Gaussians are all behind the camera gives zeros after its backward."""
    g = _small(n=200)
    e = dict(g, **{k: g[k][:0] for k in ("means3D", "colors", "opacities", "scales", "rotations")})
    r = _run(e)
    assert r["abs"].shape == (0, 2)
    behind = dict(g, means3D=g["means3D"] * np.array([1.0, 1.0, -1.0], np.float32))
    r = _run(behind, dpix=_dpix(g, 12))
    assert (r["radii"] == 0).all()
    assert (r["abs"] == 0).all()


# ---- pts2render -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["batch", "loop"])
def test_pts2render_against_four_render_ex_calls(form, monkeypatch):
    """pts2render(with_absgrad=True) at B = 4: zeros before the backward; after img.sum().backward() the two maps have the bits of four
    render_ex(absgrad=True) calls on the same packed rows, scattered to their source pixels; invalid pixels hold 0; the image is the plain call's."""
    import torch
    from gps_gaussian_amd import render_api
    from gps_gaussian_amd.pack import pack_views
    monkeypatch.setenv("GPSGS_PTS2RENDER", form)
    B = 4
    bg = [0.2, 0.3, 0.4]
    data = _batch(B)
    out = render_api.pts2render(data, bg, with_absgrad=True)
    img = out["novel_view"]["img_pred"]
    plain = render_api.pts2render(_batch(B), bg)["novel_view"]["img_pred"]
    np.testing.assert_array_equal(img.detach().cpu().numpy(), plain.detach().cpu().numpy())
    for view in ("lmain", "rmain"):
        m = out[view]["absgrad"]
        assert tuple(m.shape) == (B, 2) + tuple(data[view]["img"].shape[2:]) and m.dtype == torch.float32 and not m.requires_grad
        assert float(m.abs().max()) == 0.0
    img.sum().backward()
    assert data["lmain"]["xyz"].grad is not None

    data2 = _batch(B)
    xyz, rgb, rot, scale, opacity, offsets, rows = pack_views(data2, return_rows=True)
    xyz, rgb, rot, scale, opacity = (t.detach() for t in (xyz, rgb, rot, scale, opacity))  # (four separate backwards: not through the one pack node)
    parts = []
    for i, sl, r in render_ex_rows(data2, (xyz, rgb, rot, scale, opacity), offsets, bg, absgrad=True):
        assert tuple(r["absgrad"].shape) == (sl.stop - sl.start, 2) and float(r["absgrad"].abs().max()) == 0.0
        r["img"].sum().backward()
        parts.append(r["absgrad"])
    packed = torch.cat(parts).cpu().numpy()
    assert (packed > 0).any(axis=1).sum() > 100
    rows = rows.cpu().numpy()
    for v, view in enumerate(("lmain", "rmain")):
        m = out[view]["absgrad"].cpu().numpy().reshape(B, 2, -1)
        valid = data2[view]["pts_valid"].cpu().numpy().reshape(B, -1)
        rv = rows[:, v]
        np.testing.assert_array_equal(rv >= 0, valid)
        for c in range(2):
            np.testing.assert_array_equal(m[:, c][valid], packed[rv[valid], c])
            assert (m[:, c][~valid] == 0).all()


def test_pts2render_with_absgrad_reads_nothing_back():
    """The batch form with with_absgrad adds no host synchronisation, forward and backward: the maps are filled with device index ops."""
    import torch
    from gps_gaussian_amd import render_api
    render_api.pts2render(_batch(2), [0, 0, 0], with_absgrad=True)["novel_view"]["img_pred"].sum().backward()  # warm-up: capacities learnt
    data = _batch(2)
    with torch.cuda.stream(torch.cuda.Stream()):  # set_sync_debug_mode does not police the legacy default stream
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = render_api.pts2render(data, [0, 0, 0], with_absgrad=True)
            out["novel_view"]["img_pred"].sum().backward()
            m = out["lmain"]["absgrad"]
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert float(m.max()) > 0
