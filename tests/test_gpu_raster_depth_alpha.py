"""GPU (-m gpu): the opt-in depth and alpha maps of the rasteriser (include/gpsgs.h GsrViewExt.out_depth / out_alpha, dL_ddepth / dL_dalpha;
rasterizer.rasterize_gaussians(return_depth_alpha=True); render_api.render_ex / pts2render(with_depth_alpha=True)).

The spec: depth and alpha are two more colour channels of the same blend with background 0 -- depth = sum z_i alpha_i T_i, alpha = sum alpha_i T_i --
so an extras run must give what the EXISTING renderer gives for colours (z_i, 1, 0) and background 0: the maps are that run's R and G channels and
every gradient is that run's, except dL/dmeans3D, which also receives dL/dz_i * viewmatrix[:, 2] (dL/dz_i = that run's dL/dcolour R).  Both runs
use the VALU compositing family, so the maps and the per-Gaussian gradients agree bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_grad_parity, fragile_bounds, oracle_render, simple_scene, gaussians

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4
GRAD_TOL = 1e-3
BITWISE = ("opacities", "scales", "rotations", "means2D", "cov3D_precomp", "shs")


@pytest.fixture(autouse=True)
def _valu(monkeypatch):
    """The plain runs the extras are compared with use the VALU family too (the extras always do)."""
    monkeypatch.setenv("GPSGS_COMPOSITE", "valu")


def _render(g, colors=None, bg=None, dpix=None, dd=None, da=None, extras=False, shs=None, cov=None, sh_degree=3):
    """One view through GaussianRasterizer.  -> (img, depth|None, alpha|None, grads dict|None, per-Gaussian fp32 view-space depth)."""
    import torch
    from gps_gaussian_amd import rasterizer as RZ
    dev = torch.device("cuda:0")
    src = dict(g)
    src["colors"] = g["colors"] if colors is None else colors
    names = ["means3D", "opacities"] + (["colors"] if shs is None else ["shs"]) + (["scales", "rotations"] if cov is None else ["cov3D_precomp"])
    if shs is not None:
        src["shs"] = shs
    if cov is not None:
        src["cov3D_precomp"] = cov
    want_grad = dpix is not None or dd is not None or da is not None
    t = {k: torch.from_numpy(np.ascontiguousarray(src[k], dtype=np.float32)).to(dev).requires_grad_(want_grad) for k in names}
    m2 = torch.zeros_like(t["means3D"], requires_grad=want_grad)
    bg = g["bg"] if bg is None else np.asarray(bg, np.float32)
    rs = RZ.GaussianRasterizationSettings(g["H"], g["W"], g["tanfovx"], g["tanfovy"], torch.from_numpy(bg).to(dev), 1.0,
                                          torch.from_numpy(g["view"]).to(dev), torch.from_numpy(g["proj"]).to(dev), sh_degree,
                                          torch.from_numpy(g["campos"]).to(dev), False, False)
    RZ._debug_keep_ws = True
    try:
        out = RZ.GaussianRasterizer(rs)(means3D=t["means3D"], means2D=m2, opacities=t["opacities"], colors_precomp=t.get("colors"), shs=t.get("shs"),
                                        scales=t.get("scales"), rotations=t.get("rotations"), cov3D_precomp=t.get("cov3D_precomp"), return_depth_alpha=extras)
    finally:
        RZ._debug_keep_ws = False
    last = RZ._tls.__dict__.pop("last_ws")
    P = g["means3D"].shape[0]
    z = RZ.export_state(last["ws"], P, g["W"], g["H"], last["cap"], last["bin_cap"])["depth"].cpu().numpy() if P else np.zeros(0, np.float32)
    img = out[0]
    depth, alpha = (out[2], out[3]) if extras else (None, None)
    grads = None
    if want_grad:
        outs, gts = [], []
        for o, gt in ((img, dpix), (depth, dd), (alpha, da)):
            if o is not None and gt is not None:
                outs.append(o)
                gts.append(torch.from_numpy(np.ascontiguousarray(gt, dtype=np.float32)).to(dev).reshape(o.shape))
        torch.autograd.backward(outs, gts)
        grads = {k: t[k].grad.cpu().numpy() for k in names}
        grads["means2D"] = m2.grad.cpu().numpy()
    fetch = lambda x: None if x is None else x.detach().cpu().numpy()  # noqa: E731
    return fetch(img), fetch(depth), fetch(alpha), grads, z


def _zcol(z):
    """The colours of the equivalent plain run: (z_i, 1, 0)."""
    return np.stack([z, np.ones_like(z), np.zeros_like(z)], 1).astype(np.float32)


def _zrow(g):
    v = np.asarray(g["view"], np.float32).reshape(16)
    return v[[2, 6, 10]]  # dz/dmeans3D: z = v[2] x + v[6] y + v[10] z + v[14] (column-major flat view matrix)


def _check_against_plain(g, dd, da, shs=None, cov=None):
    """Extras run (random colours, non-zero background, no image gradient) against the plain run with colours (z, 1, 0), background 0 and
    dL/dpix = (dd, da, 0)."""
    H, W = g["H"], g["W"]
    zero = np.zeros((3, H, W), np.float32)
    _, dep, alp, ga, z = _render(g, bg=(0.3, 0.2, 0.1), dpix=zero, dd=dd, da=da, extras=True, shs=shs, cov=cov)
    dB = np.stack([np.zeros((H, W), np.float32) if dd is None else dd, np.zeros((H, W), np.float32) if da is None else da, np.zeros((H, W), np.float32)])
    imgB, _, _, gb, zB = _render(g, colors=_zcol(z), bg=(0.0, 0.0, 0.0), dpix=dB, cov=cov)
    np.testing.assert_array_equal(z, zB)
    np.testing.assert_array_equal(dep[0], imgB[0])
    np.testing.assert_array_equal(alp[0], imgB[1])
    for k in ga:
        if k in BITWISE:
            np.testing.assert_array_equal(ga[k], gb[k], err_msg=k)
    # dL/dmeans3D: the plain run's, plus dL/dz (= its dL/dcolour R) through the view matrix's third row
    dz = gb["colors"][:, 0]
    want = gb["means3D"].astype(np.float64) + dz[:, None].astype(np.float64) * _zrow(g)[None, :].astype(np.float64)
    s = np.abs(want).max() + 1e-30
    assert np.abs(ga["means3D"] - want).max() <= 1e-5 * s, np.abs(ga["means3D"] - want).max() / s
    if dd is not None and np.abs(dd).max() > 0:
        assert np.abs(ga["means3D"] - gb["means3D"]).max() > 1e-3 * s  # the z term is really there
    return dep, alp, ga, gb, z


def _scene(name):
    from gps_gaussian_amd import synthetic as S
    if name == "c1_256_30k":
        return S.make_scene(256, 30000)
    if name == "config2_1024_600k":
        return S.make_scene(1024, 600000)
    if name == "hr_2048_600k":
        return S.make_scene(1024, 600000, render_res=2048)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["c1_256_30k", "config2_1024_600k", "hr_2048_600k"])
def test_depth_alpha_equal_a_plain_run_with_colours_z_1_0(name):
    g = _scene(name)
    H, W = g["H"], g["W"]
    rng = np.random.default_rng(5)
    dd, da = rng.standard_normal((2, H, W)).astype(np.float32)
    dep, alp, ga, gb, z = _check_against_plain(g, dd, da)
    assert alp.max() <= 1.0 and alp.min() >= 0.0 and alp.max() > 0.5
    cover = alp[0] > 0.5
    mean_depth = dep[0][cover] / alp[0][cover]  # the normalised depth lies inside the range of the listed Gaussians' depths
    vis = z > 0
    assert mean_depth.min() >= z[vis].min() * (1 - 1e-5) and mean_depth.max() <= z[vis].max() * (1 + 1e-5)


def test_depth_only_alpha_only_and_neither():
    from gps_gaussian_amd import synthetic as S
    g = S.make_scene(256, 30000)
    H, W = g["H"], g["W"]
    rng = np.random.default_rng(6)
    dd, da = rng.standard_normal((2, H, W)).astype(np.float32)
    _check_against_plain(g, dd, None)
    _check_against_plain(g, None, da)
    # neither map in the loss: the extras run's gradients are the plain run's with the same colours (no z term, nothing added)
    dpix = rng.standard_normal((3, H, W)).astype(np.float32)
    img_a, dep, alp, ga, _ = _render(g, dpix=dpix, extras=True)
    img_b, _, _, gb, _ = _render(g, dpix=dpix)
    np.testing.assert_array_equal(img_a, img_b)
    for k in ga:
        np.testing.assert_array_equal(ga[k], gb[k], err_msg=k)


def test_extras_leave_the_image_and_its_gradients_bit_identical():
    """The colour output of an extras run, and its gradients under the same dL/dpix, equal the extras-off run's (same family)."""
    from gps_gaussian_amd import synthetic as S
    g = S.make_scene(256, 30000)
    g["bg"] = np.array([0.1, 0.5, 0.9], np.float32)
    rng = np.random.default_rng(7)
    dpix = rng.standard_normal((3, g["H"], g["W"])).astype(np.float32)
    dd, da = rng.standard_normal((2, g["H"], g["W"])).astype(np.float32)
    img_a, _, _, _, _ = _render(g, dpix=dpix, dd=dd, da=da, extras=True)
    img_b, _, _, gb, _ = _render(g, dpix=dpix)
    np.testing.assert_array_equal(img_a, img_b)
    # the colour gradients of an extras run with depth / alpha gradients too are the sum of the two problems: check dL/dcolours (linear, no z term)
    _, _, _, gc, _ = _render(g, dpix=dpix, dd=np.zeros_like(dd), da=np.zeros_like(da), extras=True)
    for k in gb:
        np.testing.assert_array_equal(gc[k], gb[k], err_msg=k)


def test_default_workspace_size_is_unchanged():
    from gps_gaussian_amd import _capi
    lib = _capi.lib()
    for P, W, H, cap, bcap in ((30000, 256, 256, 1 << 20, 0), (600000, 1024, 1024, 5 << 20, 1024), (1, 8, 8, 1, 0)):
        plain = lib.gsr_workspace_bytes_ex(P, W, H, cap, bcap, 0)
        extra = lib.gsr_workspace_bytes_depth_alpha(P, W, H, cap, bcap, 0)
        assert extra - plain == (cap * 4 + 255) // 256 * 256
        assert lib.gsr_workspace_bytes_depth_alpha(P, W, H, cap, bcap, 1) == lib.gsr_workspace_bytes_ex(P, W, H, cap, bcap, 1)


def test_against_the_fp64_oracle():
    """Depth / alpha and every gradient against the oracle evaluated as the spec composes it: colours (z, 1, 0), background 0, dL/dpix =
    (dL/ddepth, dL/dalpha, 0), plus the analytic z term dL/dcolour_R * viewmatrix[:, 2] for dL/dmeans3D."""
    from gps_gaussian_amd import synthetic as S
    g = S.make_scene(256, 30000)
    H, W = g["H"], g["W"]
    rng = np.random.default_rng(8)
    dd, da = rng.standard_normal((2, H, W)).astype(np.float32)
    _, dep, alp, ga, z = _render(g, bg=(0.3, 0.2, 0.1), dpix=np.zeros((3, H, W), np.float32), dd=dd, da=da, extras=True)
    sc = dict(g)
    sc["colors"], sc["bg"] = _zcol(z), np.zeros(3, np.float32)
    dpix = np.stack([dd, da, np.zeros_like(dd)])
    o, oimg, oradii = oracle_render(sc, "f32")
    geom = o.geom()
    np.testing.assert_array_equal(z[oradii > 0], geom["depth"][oradii > 0])
    o64, oimg64, _ = oracle_render(sc, "f64", decisions=geom)
    solid, touched, _ = fragile_bounds(o, dpix)
    assert solid.mean() > 0.995
    # values as every image of the suite is checked: against the fp32 oracle (same decisions) on the pixels that sit on no branch threshold; against
    # fp64 the pixels where its own evaluation takes the other side of a threshold (one contribution, about z / 255) are the only larger ones
    zmax = float(z.max())
    e_d, e_a = np.abs(dep[0] - oimg[0]), np.abs(alp[0] - oimg[1])
    assert e_d[solid].max() <= RGB_TOL * zmax, e_d[solid].max()
    assert e_a[solid].max() <= RGB_TOL, e_a[solid].max()
    e_d, e_a = np.abs(dep[0] - oimg64[0]), np.abs(alp[0] - oimg64[1])
    assert (e_d > RGB_TOL * zmax).mean() <= 1e-3 and (e_a > RGB_TOL).mean() <= 1e-3
    assert e_d.max() <= 2.0 / 255 * zmax and e_a.max() <= 2.0 / 255

    def compose(og):
        out = {k: og[k] for k in ("opacities", "scales", "rotations", "means2D")}
        out["means3D"] = og["means3D"] + og["colors"][:, :1].astype(np.float64) * _zrow(g)[None, :]
        return out

    og32, og64 = compose(o.backward(dpix)), compose(o64.backward(dpix))
    mine = {k: ga[k] for k in og32}
    assert_grad_parity(mine, og32, touched, oradii > 0)
    for k in mine:
        s = np.abs(og64[k]).max() + 1e-30
        e = np.abs(mine[k] - og64[k]) / (np.abs(og64[k]) + GRAD_TOL * s)
        assert np.quantile(e, 0.99) <= GRAD_TOL, "%s q99 %.3e" % (k, np.quantile(e, 0.99))
        assert np.abs(mine[k] - og64[k]).max() <= 0.05 * s, k


def test_no_gaussians():
    import torch
    cam = simple_scene(64, 48, 40.0)
    g = dict(cam, **gaussians(np.zeros((0, 3)), [1, 1, 1], 0.5, 0.1))
    img, dep, alp, _, _ = _render(g, bg=(0.5, 0.5, 0.5), extras=True)
    assert (img == 0).all() and (dep == 0).all() and (alp == 0).all()
    assert dep.shape == (1, 48, 64) and alp.shape == (1, 48, 64)
    torch.cuda.synchronize()


def test_capacity_repair_fills_depth_and_alpha(monkeypatch):
    """A view whose first attempt overflows its instance capacity is re-run by the repair loop: the re-run must write the maps too."""
    from gps_gaussian_amd import rasterizer as RZ
    from gps_gaussian_amd import synthetic as S
    monkeypatch.setenv("GPSGS_LISTS", "scanned")
    g = S.make_uniform_cloud(5000, 128, 96, seed=9, scale_med=0.05)
    ref = _render(g, extras=True)
    calls = []
    real = RZ._capacity_for

    def tiny_first(st, P):
        calls.append(1)
        return 1024 if len(calls) == 1 else real(st, P)

    monkeypatch.setattr(RZ, "_capacity_for", tiny_first)
    rng = np.random.default_rng(10)
    dd, da = rng.standard_normal((2, g["H"], g["W"])).astype(np.float32)
    img, dep, alp, ga, _ = _render(g, dpix=np.zeros((3, g["H"], g["W"]), np.float32), dd=dd, da=da, extras=True)
    assert len(calls) >= 2
    np.testing.assert_array_equal(img, ref[0])
    np.testing.assert_array_equal(dep, ref[1])
    np.testing.assert_array_equal(alp, ref[2])
    assert alp.max() > 0.5
    monkeypatch.setattr(RZ, "_capacity_for", real)
    _, _, _, gref, _ = _render(g, dpix=np.zeros((3, g["H"], g["W"]), np.float32), dd=dd, da=da, extras=True)
    for k in ga:
        np.testing.assert_array_equal(ga[k], gref[k], err_msg=k)


def test_shs_and_cov3D_precomp_inputs():
    from gps_gaussian_amd import synthetic as S
    g = S.make_scene(256, 30000)
    P, H, W = g["means3D"].shape[0], g["H"], g["W"]
    rng = np.random.default_rng(11)
    dd, da = rng.standard_normal((2, H, W)).astype(np.float32)
    cov = S.covariances_from(g["scales"], g["rotations"]).astype(np.float32)
    _check_against_plain(g, dd, da, cov=cov)
    # SH colours: the maps and the shape gradients do not depend on how the colours were made
    shs = S.random_shs(P, 16)
    zero = np.zeros((3, H, W), np.float32)
    _, dep_s, alp_s, gs, _ = _render(g, dpix=zero, dd=dd, da=da, extras=True, shs=shs)
    _, dep_c, alp_c, gc, _ = _render(g, dpix=zero, dd=dd, da=da, extras=True)
    np.testing.assert_array_equal(dep_s, dep_c)
    np.testing.assert_array_equal(alp_s, alp_c)
    for k in ("means3D", "opacities", "scales", "rotations", "means2D"):
        np.testing.assert_array_equal(gs[k], gc[k], err_msg=k)
    assert (gs["shs"] == 0).all()  # no image gradient: nothing reaches the SH coefficients


def test_misaligned_output_pointers():
    """The C-ABI rejects depth / alpha pointers that are not 4-byte aligned (like every fp32 array it is handed); torch views at any element
    offset are fp32-aligned and are written like any other output."""
    import torch
    from gps_gaussian_amd import _capi
    from gps_gaussian_amd import rasterizer as RZ
    from gps_gaussian_amd import synthetic as S
    g = S.make_scene(256, 30000)
    P, H, W = g["means3D"].shape[0], g["H"], g["W"]
    dev = torch.device("cuda:0")
    lib = _capi.lib()
    t = {k: torch.from_numpy(g[k]).to(dev) for k in ("means3D", "colors", "opacities", "scales", "rotations", "view", "proj", "bg")}
    color = torch.empty((3, H, W), device=dev)
    radii = torch.empty((P,), dtype=torch.int32, device=dev)
    cap = 1 << 22
    nbytes = lib.gsr_workspace_bytes_depth_alpha(P, W, H, cap, 0, 0)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    buf = torch.zeros((2 * H * W + 4,), device=dev)
    for bad in ((buf.data_ptr() + 2, None), (None, buf.data_ptr() + 1)):
        e = _capi.GsrViewExt()
        e.out_depth, e.out_alpha = bad
        rc = lib.gsr_forward_ex(P, W, H, t["means3D"].data_ptr(), t["colors"].data_ptr(), t["opacities"].data_ptr(), t["scales"].data_ptr(),
                                t["rotations"].data_ptr(), 1.0, g["tanfovx"], g["tanfovy"], t["view"].data_ptr(), t["proj"].data_ptr(), t["bg"].data_ptr(),
                                color.data_ptr(), radii.data_ptr(), ws.data_ptr(), nbytes, cap, 0, torch.cuda.current_stream().cuda_stream, None, 0,
                                C.byref(e))
        assert rc == _capi.GPSGS_E_INVALID
        e2 = _capi.GsrViewExt()
        e2.dL_ddepth, e2.dL_dalpha = bad
        d = [torch.empty((P, c), device=dev) for c in (3, 3, 3, 1, 3, 4)]
        rc = lib.gsr_backward_ex(P, W, H, t["means3D"].data_ptr(), None, None, t["scales"].data_ptr(), t["rotations"].data_ptr(), 1.0, g["tanfovx"],
                                 g["tanfovy"], t["view"].data_ptr(), t["proj"].data_ptr(), t["bg"].data_ptr(), radii.data_ptr(), color.data_ptr(),
                                 *[x.data_ptr() for x in d], ws.data_ptr(), nbytes, cap, 0, torch.cuda.current_stream().cuda_stream, C.byref(e2))
        assert rc == _capi.GPSGS_E_INVALID
    # a too-small workspace for the depth / alpha backward is refused (the forward needs nothing extra)
    e3 = _capi.GsrViewExt()
    e3.dL_ddepth = buf.data_ptr()
    small = lib.gsr_workspace_bytes_ex(P, W, H, cap, 0, 0)
    d = [torch.empty((P, c), device=dev) for c in (3, 3, 3, 1, 3, 4)]
    rc = lib.gsr_backward_ex(P, W, H, t["means3D"].data_ptr(), None, None, t["scales"].data_ptr(), t["rotations"].data_ptr(), 1.0, g["tanfovx"],
                             g["tanfovy"], t["view"].data_ptr(), t["proj"].data_ptr(), t["bg"].data_ptr(), radii.data_ptr(), color.data_ptr(),
                             *[x.data_ptr() for x in d], ws.data_ptr(), small, cap, 0, torch.cuda.current_stream().cuda_stream, C.byref(e3))
    assert rc == _capi.GPSGS_E_WORKSPACE
    torch.cuda.synchronize()
    # torch outputs at an odd element offset (4- but not 16-byte aligned): written exactly like aligned ones
    from types import SimpleNamespace
    rs = RZ.GaussianRasterizationSettings(H, W, g["tanfovx"], g["tanfovy"], t["bg"], 1.0, t["view"], t["proj"], 3, torch.zeros(3, device=dev), False, False)
    opts = RZ._view_options(rs, depth_alpha=True)
    ref = RZ._forward_impl(SimpleNamespace(), t["means3D"], t["colors"], t["opacities"], t["scales"], t["rotations"], rs, False, opts)
    big = torch.full((2 * H * W + 3,), -7.0, device=dev)
    od, oa = big[1:1 + H * W].view(H, W), big[2 + H * W:2 + 2 * H * W].view(H, W)
    out = RZ._forward_impl(SimpleNamespace(), t["means3D"], t["colors"], t["opacities"], t["scales"], t["rotations"], rs, False, opts,
                           out=dict(depth=od, alpha=oa))
    torch.cuda.synchronize()
    assert torch.equal(out[2], ref[2].reshape(H, W)) and torch.equal(out[3], ref[3].reshape(H, W))
    assert float(big[0]) == -7.0 and float(big[1 + H * W]) == -7.0 and float(big[-1]) == -7.0


def _batch_data(B):
    import os
    import torch
    from conftest import GOLDEN
    gold = np.load(os.path.join(GOLDEN, "pts2render_golden.npz"))
    dev = torch.device("cuda:0")
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


@pytest.mark.parametrize("form", ["batch", "loop"])
def test_pts2render_batch_of_4_against_four_render_ex_calls(form, monkeypatch):
    import torch
    from gps_gaussian_amd import render_api
    from gps_gaussian_amd.pack import pack_views
    monkeypatch.setenv("GPSGS_PTS2RENDER", form)
    B = 4
    data = _batch_data(B)
    for v in ("lmain", "rmain"):
        data[v]["xyz"].requires_grad_(True)
    bg = [0.2, 0.3, 0.4]
    nv = render_api.pts2render(data, bg, with_depth_alpha=True)["novel_view"]
    assert tuple(nv["depth_pred"].shape) == (B, 1, 64, 64) and tuple(nv["alpha_pred"].shape) == (B, 1, 64, 64)
    rng = np.random.default_rng(12)
    gd = torch.from_numpy(rng.standard_normal((B, 1, 64, 64)).astype(np.float32)).cuda()
    gi = torch.from_numpy(rng.standard_normal((B, 3, 64, 64)).astype(np.float32)).cuda()
    ((nv["depth_pred"] * gd).sum() + (nv["alpha_pred"] * gd.flip(2)).sum() + (nv["img_pred"] * gi).sum()).backward()
    g_batch = [data[v]["xyz"].grad.clone() for v in ("lmain", "rmain")]

    data2 = _batch_data(B)
    for v in ("lmain", "rmain"):
        data2[v]["xyz"].requires_grad_(True)
    xyz, rgb, rot, scale, opacity, offsets = pack_views(data2)
    offs = offsets.tolist()
    loss = 0
    for i in range(B):
        sl = slice(offs[i], offs[i + 1])
        r = render_api.render_ex(data2, i, xyz[sl], rgb[sl], rot[sl], scale[sl], opacity[sl], bg)
        np.testing.assert_array_equal(nv["depth_pred"][i].detach().cpu().numpy(), r["depth"].detach().cpu().numpy())
        np.testing.assert_array_equal(nv["alpha_pred"][i].detach().cpu().numpy(), r["alpha"].detach().cpu().numpy())
        np.testing.assert_array_equal(nv["img_pred"][i].detach().cpu().numpy(), r["img"].detach().cpu().numpy())
        loss = loss + (r["depth"] * gd[i]).sum() + (r["alpha"] * gd[i].flip(1)).sum() + (r["img"] * gi[i]).sum()
    loss.backward()
    for v, gbat in zip(("lmain", "rmain"), g_batch):
        gref = data2[v]["xyz"].grad
        s = float(gref.abs().max())
        assert s > 0
        assert float((gbat - gref).abs().max()) <= 1e-6 * s, v
