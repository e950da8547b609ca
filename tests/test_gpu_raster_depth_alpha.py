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
from raster_run import batch_with_xyz_grad, check_against_plain as _check_against_plain, depth_alpha_run as _render, render_ex_rows, scene, settings
from raster_run import valu_fixture, zcol as _zcol, zrow as _zrow

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4
GRAD_TOL = 1e-3

_valu = valu_fixture()  # the plain runs the extras are compared with use the VALU family too (the extras always do)


def _scene(name):
    return scene({"c1_256_30k": "256", "config2_1024_600k": "config2", "hr_2048_600k": "2048"}[name])


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
    rs = settings(g, view=t["view"], proj=t["proj"], campos=torch.zeros(3, device=dev))
    opts = RZ._view_options(rs, depth_alpha=True)
    ref = RZ._forward_impl(SimpleNamespace(), t["means3D"], t["colors"], t["opacities"], t["scales"], t["rotations"], rs, False, opts)
    big = torch.full((2 * H * W + 3,), -7.0, device=dev)
    od, oa = big[1:1 + H * W].view(H, W), big[2 + H * W:2 + 2 * H * W].view(H, W)
    out = RZ._forward_impl(SimpleNamespace(), t["means3D"], t["colors"], t["opacities"], t["scales"], t["rotations"], rs, False, opts,
                           out=dict(depth=od, alpha=oa))
    torch.cuda.synchronize()
    assert torch.equal(out.depth, ref.depth.reshape(H, W)) and torch.equal(out.alpha, ref.alpha.reshape(H, W))
    assert float(big[0]) == -7.0 and float(big[1 + H * W]) == -7.0 and float(big[-1]) == -7.0


@pytest.mark.parametrize("form", ["batch", "loop"])
def test_pts2render_batch_of_4_against_four_render_ex_calls(form, monkeypatch):
    import torch
    from gps_gaussian_amd import render_api
    from gps_gaussian_amd.pack import pack_views
    monkeypatch.setenv("GPSGS_PTS2RENDER", form)
    B = 4
    data = batch_with_xyz_grad(B)
    bg = [0.2, 0.3, 0.4]
    nv = render_api.pts2render(data, bg, with_depth_alpha=True)["novel_view"]
    assert tuple(nv["depth_pred"].shape) == (B, 1, 64, 64) and tuple(nv["alpha_pred"].shape) == (B, 1, 64, 64)
    rng = np.random.default_rng(12)
    gd = torch.from_numpy(rng.standard_normal((B, 1, 64, 64)).astype(np.float32)).cuda()
    gi = torch.from_numpy(rng.standard_normal((B, 3, 64, 64)).astype(np.float32)).cuda()
    ((nv["depth_pred"] * gd).sum() + (nv["alpha_pred"] * gd.flip(2)).sum() + (nv["img_pred"] * gi).sum()).backward()
    g_batch = [data[v]["xyz"].grad.clone() for v in ("lmain", "rmain")]

    data2 = batch_with_xyz_grad(B)
    *packed, offsets = pack_views(data2)
    loss = 0
    for i, sl, r in render_ex_rows(data2, packed, offsets, bg):
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
