"""GPU (-m gpu): every valid combination of the rasteriser's six opt-ins -- depth / alpha maps, antialiasing, camera gradients, feature maps,
contribution statistics, absgrad: 40 combinations, features exclude the last two -- through the three host paths that assemble and decode the output
tuple: rasterizer.rasterize_gaussians, render_api.pts2render in its batch form (B = 2) and with GPSGS_PTS2RENDER=loop.

What the headers promise and this file holds every combination to (include/gpsgs.h; the docstrings of rasterize_gaussians and pts2render):
the outputs come in the documented order with the documented shapes and dtypes; an opt-in changes no bit of the colour, the radii or any per-Gaussian
gradient (only antialiasing changes the arithmetic, so the call with only `antialiasing` set the same way is the reference); the camera gradients
keep their bits whatever else is on; the statistics and absgrad are what they are when requested alone; features with the statistics or absgrad
are refused before a view is planned.  GPSGS_COMPOSITE=valu throughout: the opt-in maps come from the VALU kernels, so the all-off call must use
them too to be comparable bit for bit.  The loss is on the colour image only.
"""
import itertools
import os

import numpy as np
import pytest

from conftest import GOLDEN, simple_scene
from raster_run import output_table

pytestmark = pytest.mark.gpu

OPTIONS = ("depth_alpha", "antialiasing", "camera_grad", "features", "contrib", "absgrad")
COMBOS = [frozenset(o for o, on in zip(OPTIONS, bits) if on) for bits in itertools.product((False, True), repeat=len(OPTIONS))]
COMBOS = [c for c in COMBOS if not ("features" in c and ("contrib" in c or "absgrad" in c))]
F = 3
VIEWS = ("lmain", "rmain")
STATS = (("contrib_weight", np.float32), ("contrib_max", np.float32), ("contrib_pixels", np.int32))


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        np.testing.assert_array_equal(a, b, err_msg=what)


# ---- one view: rasterize_gaussians ------------------------------------------------------------------------------------------------------------------

def _run_view(c):
    """-> dict(out: named outputs, grads: per-Gaussian gradients, cam: camera gradients, feat_grad) as numpy, after the backward of sum(colour * dpix)."""
    import torch
    from gps_gaussian_amd import rasterizer as RZ
    from gps_gaussian_amd import synthetic as S
    dev = torch.device("cuda:0")
    g = S.make_uniform_cloud(200, 44, 28, scale_med=0.05)
    P, H, W = g["means3D"].shape[0], g["H"], g["W"]
    rng = np.random.default_rng(7)
    names = ("means3D", "colors", "opacities", "scales", "rotations")
    t = {k: torch.from_numpy(np.ascontiguousarray(g[k], dtype=np.float32)).to(dev).requires_grad_(True) for k in names}
    t["means2D"] = torch.zeros_like(t["means3D"], requires_grad=True)
    cam = {k: torch.from_numpy(np.ascontiguousarray(g[k], dtype=np.float32)).to(dev).requires_grad_("camera_grad" in c) for k in ("view", "proj", "campos")}
    dpix = torch.from_numpy(rng.standard_normal((3, H, W)).astype(np.float32)).to(dev)
    feats = torch.from_numpy(rng.uniform(-1, 1, (P, F)).astype(np.float32)).to(dev).requires_grad_(True) if "features" in c else None
    rs = RZ.GaussianRasterizationSettings(H, W, g["tanfovx"], g["tanfovy"], torch.from_numpy(g["bg"]).to(dev), 1.0, cam["view"], cam["proj"], 3,
                                          cam["campos"], False, False)
    out = RZ.rasterize_gaussians(t["means3D"], t["means2D"], None, t["colors"], t["opacities"], t["scales"], t["rotations"], None, rs,
                                 return_depth_alpha="depth_alpha" in c, antialiasing="antialiasing" in c, camera_grad="camera_grad" in c,
                                 features=feats, return_contrib="contrib" in c, return_absgrad="absgrad" in c)
    # the documented order, shapes and dtypes
    want = output_table(P, H, W, extras="depth_alpha" in c, F=F if "features" in c else 0, contrib="contrib" in c, absgrad="absgrad" in c)
    assert isinstance(out, tuple) and len(out) == len(want), (sorted(c), len(out))
    for x, (name, shape, dtype, diff) in zip(out, want):
        assert tuple(x.shape) == shape and x.dtype == getattr(torch, dtype) and x.requires_grad == diff and x.device == dev, (sorted(c), name)
    named = dict(zip((w[0] for w in want), out))
    if "absgrad" in c:
        assert float(named["absgrad"].abs().max()) == 0.0  # zeros until a backward has run
    (out[0] * dpix).sum().backward()
    torch.cuda.synchronize()
    return dict(out={k: _np(v) for k, v in named.items()}, grads={k: _np(v.grad) for k, v in t.items()}, cam={k: _np(v.grad) for k, v in cam.items()},
                feat_grad=_np(feats.grad) if feats is not None else None)


# ---- a batch of two: pts2render ---------------------------------------------------------------------------------------------------------------------

GRAD_KEYS = ("img", "xyz", "rot_maps", "scale_maps", "opacity_maps")
CAM_KEYS = ("world_view_transform", "full_proj_transform", "camera_center")


def _batch_data(c):
    """The two 12 x 12 samples of the golden fixture in front of a 24 x 20 novel camera; every per-pixel input is a leaf that wants a gradient."""
    import torch
    gold = np.load(os.path.join(GOLDEN, "pts2render_golden.npz"))
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(17)
    data = {}
    for v in VIEWS:
        d = {k: torch.from_numpy(gold["%s_%s" % (v, k)]).to(dev) for k in GRAD_KEYS + ("pts_valid",)}
        d["xyz"] = d["xyz"] * torch.tensor([0.3, 0.25, 0.1], device=dev) + torch.tensor([0.0, 0.0, 2.0], device=dev)
        d["scale_maps"] = d["scale_maps"] * 5
        for k in GRAD_KEYS:
            d[k] = d[k].detach().contiguous().requires_grad_(True)
        if "features" in c:
            d["sem"] = torch.from_numpy(rng.standard_normal((2, F, 12, 12)).astype(np.float32)).to(dev).requires_grad_(True)
        data[v] = d
    W, H = 24, 20
    cam = simple_scene(W, H, 18.0)
    nv = dict(FovX=torch.tensor([2 * np.arctan(cam["tanfovx"])] * 2), FovY=torch.tensor([2 * np.arctan(cam["tanfovy"])] * 2),
              width=torch.tensor([W] * 2), height=torch.tensor([H] * 2),
              world_view_transform=torch.from_numpy(cam["view"])[None].repeat(2, 1, 1), full_proj_transform=torch.from_numpy(cam["proj"])[None].repeat(2, 1, 1),
              camera_center=torch.zeros(2, 3))
    nv["world_view_transform"][1, 3, :3] += torch.tensor([0.02, -0.01, 0.03])  # the second sample's camera differs from the first's
    nv["full_proj_transform"][1] = nv["world_view_transform"][1] @ torch.from_numpy(np.linalg.inv(cam["view"]) @ cam["proj"])
    for k in CAM_KEYS:
        nv[k] = nv[k].float().contiguous().requires_grad_("camera_grad" in c)
    data["novel_view"] = nv
    return data


def _run_batch(c):
    import torch
    from gps_gaussian_amd import render_api
    data = _batch_data(c)
    nv = data["novel_view"]
    before = dict({v: set(data[v]) for v in VIEWS}, novel_view=set(nv))
    render_api.pts2render(data, [0.2, 0.3, 0.4], with_depth_alpha="depth_alpha" in c, antialiasing="antialiasing" in c, camera_grad="camera_grad" in c,
                          feature_key="sem" if "features" in c else None, with_contrib="contrib" in c, with_absgrad="absgrad" in c)
    B, H, W, dev = 2, 20, 24, data["lmain"]["img"].device
    # exactly the documented keys, with the documented shapes and dtypes
    want_nv = {"img_pred": (B, 3, H, W)}
    if "depth_alpha" in c:
        want_nv.update(depth_pred=(B, 1, H, W), alpha_pred=(B, 1, H, W))
    if "features" in c:
        want_nv["feat_pred"] = (B, F, H, W)
    assert set(nv) - before["novel_view"] == set(want_nv), sorted(c)
    for k, shape in want_nv.items():
        assert tuple(nv[k].shape) == shape and nv[k].dtype == torch.float32 and nv[k].requires_grad and nv[k].device == dev, (sorted(c), k)
    want_src = {}
    if "contrib" in c:
        want_src.update({k: ((B, 1, 12, 12), torch.int32 if dt is np.int32 else torch.float32) for k, dt in STATS})
    if "absgrad" in c:
        want_src["absgrad"] = ((B, 2, 12, 12), torch.float32)
    for v in VIEWS:
        assert set(data[v]) - before[v] == set(want_src), (sorted(c), v)
        for k, (shape, dtype) in want_src.items():
            assert tuple(data[v][k].shape) == shape and data[v][k].dtype == dtype and not data[v][k].requires_grad, (sorted(c), v, k)
        if "absgrad" in c:
            assert float(data[v]["absgrad"].abs().max()) == 0.0  # zeros until the backward has run
    rng = np.random.default_rng(27)
    gi = torch.from_numpy(rng.standard_normal((B, 3, H, W)).astype(np.float32)).to(dev)
    (nv["img_pred"] * gi).sum().backward()
    torch.cuda.synchronize()
    out = {k: _np(nv[k]) for k in want_nv}
    out.update({"%s_%s" % (v, k): _np(data[v][k]) for v in VIEWS for k in want_src})
    return dict(out=out, grads={"%s_%s" % (v, k): _np(data[v][k].grad) for v in VIEWS for k in GRAD_KEYS}, cam={k: _np(nv[k].grad) for k in CAM_KEYS},
                feat_grad=np.stack([_np(data[v]["sem"].grad) for v in VIEWS]) if "features" in c else None)


# ---- the matrix -------------------------------------------------------------------------------------------------------------------------------------

def _aa(c, *more):
    """The combination with only `antialiasing` set as in c, plus `more`."""
    return frozenset(more) | (c & {"antialiasing"})


@pytest.mark.parametrize("path", ["rasterize_gaussians", "pts2render_batch", "pts2render_loop"])
def test_every_valid_combination(path, monkeypatch):
    monkeypatch.setenv("GPSGS_COMPOSITE", "valu")
    monkeypatch.setenv("GPSGS_PTS2RENDER", "loop" if path == "pts2render_loop" else "batch")
    assert len(COMBOS) == 40
    run = _run_view if path == "rasterize_gaussians" else _run_batch
    res = {c: run(c) for c in COMBOS}
    colour = "color" if path == "rasterize_gaussians" else "img_pred"
    for c, r in res.items():
        tag = "%s %s" % (path, sorted(c))
        # colour, radii and every per-Gaussian gradient: the bits of the call with only antialiasing set the same way
        base = res[_aa(c)]
        _same(r["out"][colour], base["out"][colour], tag + " colour")
        if "radii" in r["out"]:
            _same(r["out"]["radii"], base["out"]["radii"], tag + " radii")
        assert set(r["grads"]) == set(base["grads"])
        for k in base["grads"]:
            assert base["grads"][k] is not None and np.isfinite(base["grads"][k]).all(), k
            _same(r["grads"][k], base["grads"][k], tag + " dL/d" + k)
        # camera gradients: the same bits in every combination that shares antialiasing; None without the option
        for k, v in r["cam"].items():
            if "camera_grad" in c:
                _same(v, res[_aa(c, "camera_grad")]["cam"][k], tag + " dL/d" + k)
            else:
                assert v is None, tag + " " + k
        # the maps, statistics and absgrad: what they are when requested alone
        for opt, keys in (("depth_alpha", ("depth", "alpha")), ("features", ("feat",)), ("contrib", ("contrib_",)), ("absgrad", ("absgrad",))):
            if opt in c:
                alone = res[_aa(c, opt)]
                mine = [k for k in r["out"] if any(s in k for s in keys)]
                assert mine and set(mine) == {k for k in alone["out"] if any(s in k for s in keys)}
                for k in mine:
                    _same(r["out"][k], alone["out"][k], tag + " " + k)
        if "features" in c:
            _same(r["feat_grad"], res[_aa(c, "features")]["feat_grad"], tag + " dL/dfeatures")
    # the comparisons above are not vacuous: something was rendered, antialiasing changes it, the gradients and the opt-in outputs are not all zero
    off, aa = res[frozenset()], res[frozenset({"antialiasing"})]
    assert np.abs(off["out"][colour] - aa["out"][colour]).max() > 0
    assert all(np.abs(v).max() > 0 for v in off["grads"].values())
    cg = res[frozenset({"camera_grad"})]["cam"]
    assert all(np.abs(cg[k]).max() > 0 for k in list(cg)[:2])
    everything = res[frozenset(OPTIONS) - {"features"}]["out"]
    for k, v in everything.items():
        assert np.isfinite(v).all() and np.abs(v).max() > 0, k
    assert np.abs(res[frozenset({"features"})]["out"]["feat" if path == "rasterize_gaussians" else "feat_pred"]).max() > 0


@pytest.mark.parametrize("path", ["rasterize_gaussians", "pts2render_batch", "pts2render_loop"])
@pytest.mark.parametrize("other", ["contrib", "absgrad"])
def test_features_are_refused_with_statistics_or_absgrad(path, other, monkeypatch):
    """A RuntimeError that mentions `features` -- pts2render's own check of with_contrib names its keyword, `feature_key` -- raised before a single
    view is planned (every launch attempt goes through rasterizer._plan)."""
    from gps_gaussian_amd import rasterizer as RZ
    monkeypatch.setenv("GPSGS_COMPOSITE", "valu")
    monkeypatch.setenv("GPSGS_PTS2RENDER", "loop" if path == "pts2render_loop" else "batch")
    planned = []
    real = RZ._plan
    monkeypatch.setattr(RZ, "_plan", lambda *a, **k: (planned.append(1), real(*a, **k))[1])
    run = _run_view if path == "rasterize_gaussians" else _run_batch
    for extra in ((), ("depth_alpha", "antialiasing", "camera_grad")):
        with pytest.raises(RuntimeError, match="features" if path == "rasterize_gaussians" or other == "absgrad" else "feature_key"):
            run(frozenset(("features", other) + extra))
    assert not planned
