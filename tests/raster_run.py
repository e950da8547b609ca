"""What the GPU tests of the rasteriser's opt-ins share (tests/test_gpu_raster_*.py): the table of what a call returns, one view runner that
decodes and checks the outputs with it, the small scenes, and the stage-2 batch fixture of the pts2render tests.

The output table is written out here from rasterize_gaussians' docstring.  It is NOT derived from rasterizer._unpack_outputs: the product has its
decoder and the tests have theirs, so a mis-ordered output tuple fails (tests/test_raster_run.py holds the two to each other).
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, gaussians, simple_scene

GAUSSIANS = ("means3D", "colors", "opacities", "scales", "rotations")
GEOM = ("means3D", "means2D", "opacities", "scales", "rotations")
RGB_TOL = 1e-4  # the suite's RGB tolerance
# the documented output names -> the keys of run_view's result
KEYS = dict(color="img", radii="radii", depth="depth", alpha="alpha", feat="feat", contrib_weight="w", contrib_max="m", contrib_pixels="n",
            absgrad="abs", distortion="dist")


# ---- the output table -----------------------------------------------------------------------------------------------------------------------------

def output_table(P, H, W, extras=False, F=0, contrib=False, absgrad=False, distortion=False):
    """-> [(name, shape, dtype name, differentiable)], in the order a call with these options returns its outputs.  extras: the depth and alpha maps;
    F: the number of feature channels (0 = no features given).  Antialiasing and camera gradients add no output."""
    t = [("color", (3, H, W), "float32", True), ("radii", (P,), "int32", False)]
    if extras:
        t += [("depth", (1, H, W), "float32", True), ("alpha", (1, H, W), "float32", True)]
    if F:
        t += [("feat", (F, H, W), "float32", True)]
    if contrib:
        t += [("contrib_weight", (P,), "float32", False), ("contrib_max", (P,), "float32", False), ("contrib_pixels", (P,), "int32", False)]
    if absgrad:
        t += [("absgrad", (P, 2), "float32", False)]
    if distortion:
        t += [("distortion", (1, H, W), "float32", True)]
    return t


def decode(out, g, want, F=0, **options):
    """The tuple a call on scene g returned -> {documented name: tensor}, after holding it to output_table(**options): its length, every output's
    shape, dtype and device, requires_grad (a differentiable output exactly when some input requires a gradient, `want`; never the others), and
    absgrad all zero (this is before any backward)."""
    import torch
    table = output_table(g["means3D"].shape[0], g["H"], g["W"], F=F, **options)
    assert len(out) == len(table), (len(out), [row[0] for row in table])
    for x, (name, shape, dtype, diff) in zip(out, table):
        assert tuple(x.shape) == shape and x.dtype == getattr(torch, dtype) and x.device == device(), (name, tuple(x.shape), x.dtype, x.device)
        assert x.requires_grad == (diff and want) and (diff or x.grad_fn is None), (name, x.requires_grad)
    named = {row[0]: x for row, x in zip(table, out)}
    if "absgrad" in named:
        assert not bool(named["absgrad"].any())
    return named


# ---- one view -------------------------------------------------------------------------------------------------------------------------------------

def device():
    import torch
    return torch.device("cuda:0")


def to_dev(x, dev=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device() if dev is None else dev)


def leaves(g, names=GAUSSIANS, grad=False):
    """The arrays `names` of the scene as fp32 device tensors; grad: whether they require a gradient, a bool or a function of the name."""
    return {k: to_dev(g[k]).requires_grad_(grad(k) if callable(grad) else grad) for k in names}


def settings(g, bg=None, view=None, proj=None, campos=None, sh_degree=3, make=None):
    """GaussianRasterizationSettings of the scene's camera.  bg: another background (array); view / proj / campos: tensors to use instead of the
    scene's; make: called with the twelve fields instead of GaussianRasterizationSettings (a settings object of another type)."""
    from gps_gaussian_amd import rasterizer as RZ
    view, proj, campos = (to_dev(g[k]) if x is None else x for k, x in (("view", view), ("proj", proj), ("campos", campos)))
    return (make or RZ.GaussianRasterizationSettings)(g["H"], g["W"], g["tanfovx"], g["tanfovy"], to_dev(g["bg"] if bg is None else bg),
                                                      float(g.get("scale_modifier", 1.0)), view, proj, sh_degree, campos, False, False)


def rasterize(rs, t, m2=None, **kw):
    """GaussianRasterizer(rs) on the tensors of t (colors or shs; scales + rotations or cov3D_precomp); m2: means2D, zeros by default."""
    import torch
    from gps_gaussian_amd import rasterizer as RZ
    return RZ.GaussianRasterizer(rs)(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]) if m2 is None else m2, opacities=t["opacities"],
                                     colors_precomp=t.get("colors"), shs=t.get("shs"), scales=t.get("scales"), rotations=t.get("rotations"),
                                     cov3D_precomp=t.get("cov3D_precomp"), **kw)


def run_view(g, cot=None, cot2=None, *, colors=None, bg=None, shs=None, cov=None, sh_degree=3, extras=False, aa=False, cam=False, feats=None,
             contrib=False, absgrad=False, distortion=False, color_grad=True, feat_grad=True, cam_device=None, pinned=False, campos_leaf=False,
             raw_cam=False, keep_ws=False, make_settings=None):
    """One view of scene g through GaussianRasterizer, its outputs decoded and checked (decode), then the backward.

    cot: {img / depth / alpha / feat / dist: cotangent} (None entries count as absent; [H, W] is reshaped to the output's shape).  The outputs named
    get exactly their cotangent, the others none.  No cotangent at all: no tensor requires a gradient and no backward runs.  cot2: a second backward
    over the retained graph, from cleared gradients.
    colors / bg / shs / cov: instead of the scene's colours / background / colours / scales + rotations.  extras, aa, cam, feats [P, F], contrib,
    absgrad, distortion: the opt-ins (aa=None: the call without the antialiasing keyword).  color_grad / feat_grad: whether the colours / features
    require a gradient when anything does.  cam_device, pinned: where the camera matrices live (pinned alone: pinned CPU memory); campos_leaf: campos
    lives with them and is a leaf like them.  make_settings: see settings().  keep_ws: also `st`, export_state of the forward's workspace (None for
    an empty cloud).
    -> dict of numpy arrays: img, radii, depth, alpha, feat, w, m, n (the statistics), abs0 (absgrad before any backward), abs (after the last),
    dist [H, W], and grads: one entry per input that required a gradient -- means2D, features, view and proj included.  raw_cam: the camera
    gradients are not in grads but, as the tensors autograd left, in cam (view, proj, campos; None without cam), with the leaves in cam_tensors."""
    import torch
    from gps_gaussian_amd import rasterizer as RZ
    dev = device()
    cots = [{k: v for k, v in (c or {}).items() if v is not None} for c in (cot, cot2)]
    want = bool(cots[0])
    src = dict(g, shs=shs, cov3D_precomp=cov)
    if colors is not None:
        src["colors"] = colors
    names = ["means3D", "opacities"] + (["colors"] if shs is None else ["shs"]) + (["scales", "rotations"] if cov is None else ["cov3D_precomp"])
    t = leaves(src, names, lambda k: want and (color_grad or k != "colors"))
    m2 = torch.zeros_like(t["means3D"], requires_grad=want)
    ft = to_dev(feats).requires_grad_(want and feat_grad) if feats is not None else None
    cdev = torch.device(cam_device if cam_device is not None else "cpu" if pinned else dev)

    def camera(k):
        x = to_dev(g[k], cdev)
        return (x.pin_memory() if pinned else x).requires_grad_(cam)

    view, proj, campos = camera("view"), camera("proj"), camera("campos") if campos_leaf else to_dev(g["campos"])
    rs = settings(g, bg, view, proj, campos, sh_degree, make_settings)
    kw = dict(return_depth_alpha=extras, camera_grad=cam, features=ft, return_contrib=contrib, return_absgrad=absgrad, return_distortion=distortion)
    if aa is not None:
        kw["antialiasing"] = aa
    RZ._debug_keep_ws = keep_ws  # (records a reference to the workspace; selects no path)
    try:
        out = rasterize(rs, t, m2, **kw)
    finally:
        RZ._debug_keep_ws = False
    r = {}
    if keep_ws:
        last = RZ._tls.__dict__.pop("last_ws")
        P = g["means3D"].shape[0]
        r["st"] = RZ.export_state(last["ws"], P, g["W"], g["H"], last["cap"], last["bin_cap"]) if P else None
    named = decode(out, g, want or cam, F=0 if ft is None else ft.shape[1], extras=extras, contrib=contrib, absgrad=absgrad, distortion=distortion)
    named = {KEYS[k]: v for k, v in named.items()}
    r.update(named)
    if absgrad:
        r["abs0"] = named["abs"].clone()
    inputs = dict(t, means2D=m2)
    if ft is not None:
        inputs["features"] = ft
    if not raw_cam:
        inputs.update(view=view, proj=proj)
    for i, c in enumerate(cots):
        if c:
            for x in list(inputs.values()) + [view, proj, campos]:
                x.grad = None
            torch.autograd.backward([named[k] for k in c], [to_dev(v).reshape(named[k].shape) for k, v in c.items()], retain_graph=i == 0 and bool(cots[1]))
    if want:
        r["grads"] = {k: x.grad.cpu().numpy() for k, x in inputs.items() if x.requires_grad}
    if raw_cam:
        r["cam_tensors"] = (view, proj, campos)
        r["cam"] = dict(view=view.grad, proj=proj.grad, campos=campos.grad) if cam else None
    if distortion:
        r["dist"] = r["dist"][0]
    torch.cuda.synchronize()
    return {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else v) for k, v in r.items()}


# ---- the scenes, the VALU fixture -------------------------------------------------------------------------------------------------------------------

def small(seed=5, n=1500, W=96, H=64):
    """96 x 64 pixels, 1500 Gaussians in front of an identity-pose camera."""
    rng = np.random.default_rng(seed)
    cam = simple_scene(W, H, 70.0, bg=(0.2, 0.1, 0.3))
    xyz = np.stack([rng.uniform(-0.7, 0.7, n), rng.uniform(-0.45, 0.45, n), rng.uniform(1.5, 3.0, n)], 1)
    scale = np.exp(rng.uniform(np.log(0.003), np.log(0.05), (n, 3)))
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return dict(cam, **gaussians(xyz, rng.uniform(0, 1, (n, 3)), rng.uniform(0.05, 0.95, n), scale, q))


def scene(name):
    """"96x64": small(); "256", "config2", "2048": the benchmark's scenes (config 1, config 2, config 2 rendered at 2048 x 2048)."""
    from gps_gaussian_amd import synthetic as S
    if name == "96x64":
        return small()
    res, n, render_res = {"256": (256, 30000, None), "config2": (1024, 600000, None), "2048": (1024, 600000, 2048)}[name]
    return S.make_scene(res, n, render_res=render_res)


def valu_fixture():
    """An autouse fixture for a test module whose opt-in runs always use the VALU compositing family: the plain runs they are compared with bit for
    bit then use it too.  Install it with `_valu = valu_fixture()`."""
    @pytest.fixture(autouse=True)
    def _valu(monkeypatch):
        monkeypatch.setenv("GPSGS_COMPOSITE", "valu")
    return _valu


# ---- checks that more than one file makes ---------------------------------------------------------------------------------------------------------

def close(a, b, tol, what):
    """max |a - b| <= tol x max |b|."""
    s = max(float(np.abs(b).max()), 1e-30)
    err = float(np.abs(a - b).max())
    assert err <= tol * s, "%s: max error %.3e > %.1e x scale %.3e" % (what, err, tol, s)


def close_each(a, b, tol=RGB_TOL, floor=1e-7):
    """Element by element: |a - b| <= tol |b| + floor -> bool array."""
    return np.abs(a - b) <= tol * np.abs(b) + floor


def pad(a):
    """[P, 2] -> [P, 3], the shape of means2D's gradient."""
    return np.concatenate([a, np.zeros((a.shape[0], 1), a.dtype)], 1)


def check_absgrad_structure(r):
    """Finite, never negative, zero for culled Gaussians, and the triangle inequality against the signed gradient at the suite's tolerance."""
    a, gm = r["abs"], r["grads"]["means2D"][:, :2]
    assert np.isfinite(a).all() and (a >= 0).all()
    assert (a[r["radii"] == 0] == 0).all()
    assert (np.abs(gm) <= a + 1e-3 * (a + 1e-3 * np.abs(gm).max())).all()


def check_contrib_structure(r):
    """max <= min(0.99, sum); the three statistics agree on who contributes; culled Gaussians get zeros."""
    w, m, n, radii = r["w"], r["m"], r["n"], r["radii"]
    assert np.isfinite(w).all() and np.isfinite(m).all()
    assert (m <= np.minimum(np.float32(0.99), w)).all()
    assert ((n > 0) == (w > 0)).all() and ((w > 0) == (m > 0)).all()
    assert (n >= 0).all()
    culled = radii == 0
    assert (w[culled] == 0).all() and (m[culled] == 0).all() and (n[culled] == 0).all()


def depth_alpha_run(g, colors=None, bg=None, dpix=None, dd=None, da=None, extras=False, shs=None, cov=None, sh_degree=3):
    """run_view for the depth / alpha maps -> (img, depth | None, alpha | None, grads | None, per-Gaussian fp32 view-space depth)."""
    r = run_view(g, dict(img=dpix, depth=dd, alpha=da), colors=colors, bg=bg, shs=shs, cov=cov, sh_degree=sh_degree, extras=extras, keep_ws=True)
    z = r["st"]["depth"].cpu().numpy() if r["st"] is not None else np.zeros(0, np.float32)
    return r["img"], r.get("depth"), r.get("alpha"), r.get("grads"), z


def zcol(z):
    """The colours of the plain run that is equivalent to a depth / alpha run: (z_i, 1, 0)."""
    return np.stack([z, np.ones_like(z), np.zeros_like(z)], 1).astype(np.float32)


def zrow(g):
    v = np.asarray(g["view"], np.float32).reshape(16)
    return v[[2, 6, 10]]  # dz/dmeans3D: z = v[2] x + v[6] y + v[10] z + v[14] (column-major flat view matrix)


BITWISE = ("opacities", "scales", "rotations", "means2D", "cov3D_precomp", "shs")


def check_against_plain(g, dd, da, shs=None, cov=None):
    """Depth / alpha run (random colours, non-zero background, no image gradient) against the plain run with colours (z, 1, 0), background 0 and
    dL/dpix = (dd, da, 0)."""
    H, W = g["H"], g["W"]
    zero = np.zeros((3, H, W), np.float32)
    _, dep, alp, ga, z = depth_alpha_run(g, bg=(0.3, 0.2, 0.1), dpix=zero, dd=dd, da=da, extras=True, shs=shs, cov=cov)
    dB = np.stack([np.zeros((H, W), np.float32) if dd is None else dd, np.zeros((H, W), np.float32) if da is None else da, np.zeros((H, W), np.float32)])
    imgB, _, _, gb, zB = depth_alpha_run(g, colors=zcol(z), bg=(0.0, 0.0, 0.0), dpix=dB, cov=cov)
    np.testing.assert_array_equal(z, zB)
    np.testing.assert_array_equal(dep[0], imgB[0])
    np.testing.assert_array_equal(alp[0], imgB[1])
    for k in ga:
        if k in BITWISE:
            np.testing.assert_array_equal(ga[k], gb[k], err_msg=k)
    # dL/dmeans3D: the plain run's, plus dL/dz (= its dL/dcolour R) through the view matrix's third row
    dz = gb["colors"][:, 0]
    want = gb["means3D"].astype(np.float64) + dz[:, None].astype(np.float64) * zrow(g)[None, :].astype(np.float64)
    s = np.abs(want).max() + 1e-30
    assert np.abs(ga["means3D"] - want).max() <= 1e-5 * s, np.abs(ga["means3D"] - want).max() / s
    if dd is not None and np.abs(dd).max() > 0:
        assert np.abs(ga["means3D"] - gb["means3D"]).max() > 1e-3 * s  # the z term is really there
    return dep, alp, ga, gb, z


# ---- the stage-2 batch ------------------------------------------------------------------------------------------------------------------------------

def batch_data(B):
    """B stage-2 samples (the tests/golden pts2render fixture, repeated and shifted) in front of a 64 x 64 novel camera; the cameras on the host."""
    import torch
    gold = np.load(os.path.join(GOLDEN, "pts2render_golden.npz"))
    dev = device()
    side = 64
    data = {}
    for v in ("lmain", "rmain"):
        d = {k: torch.from_numpy(gold["%s_%s" % (v, k)]).to(dev) for k in ("img", "xyz", "pts_valid", "rot_maps", "scale_maps", "opacity_maps")}
        rep = (B + d["img"].shape[0] - 1) // d["img"].shape[0]
        d = {k: torch.cat([x] * rep)[:B].contiguous() for k, x in d.items()}
        d["xyz"] = d["xyz"] * 0.1 + torch.tensor([0.0, 0.0, 2.0], device=dev)
        d["scale_maps"] = d["scale_maps"] * 5
        d["xyz"][2:] = d["xyz"][2:] + torch.tensor([0.05, -0.03, 0.4], device=dev)  # the repeated samples differ from the first ones
        data[v] = d
    cam = simple_scene(side, side, 48.0)
    data["novel_view"] = dict(
        FovX=torch.tensor([2 * np.arctan(cam["tanfovx"])] * B), FovY=torch.tensor([2 * np.arctan(cam["tanfovy"])] * B),
        width=torch.tensor([side] * B), height=torch.tensor([side] * B),
        world_view_transform=torch.from_numpy(cam["view"])[None].repeat(B, 1, 1),
        full_proj_transform=torch.from_numpy(cam["proj"])[None].repeat(B, 1, 1), camera_center=torch.zeros(B, 3))
    return data


def batch_with_xyz_grad(B):
    """batch_data whose points require a gradient."""
    data = batch_data(B)
    for v in ("lmain", "rmain"):
        data[v]["xyz"].requires_grad_(True)
    return data


def batch(B):
    """batch_with_xyz_grad with the cameras on the device (as training hands them over): no host copy inside pts2render."""
    import torch
    data = batch_with_xyz_grad(B)
    nv = data["novel_view"]
    nv["world_view_transform"], nv["full_proj_transform"] = nv["world_view_transform"].cuda(), nv["full_proj_transform"].cuda()
    torch.cuda.synchronize()
    return data


def render_ex_rows(data, packed, offsets, bg, **kw):
    """render_api.render_ex for every sample of a packed batch (packed = pack_views' xyz, rgb, rot, scale, opacity) -> (i, row slice, result)."""
    from gps_gaussian_amd import render_api
    offs = offsets.tolist()
    for i in range(len(offs) - 1):
        sl = slice(offs[i], offs[i + 1])
        yield i, sl, render_api.render_ex(data, i, *(x[sl] for x in packed), bg, **kw)
