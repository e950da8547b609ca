"""GPU (-m gpu): the opt-in camera gradients of the rasteriser (include/gpsgs.h gsr_backward_camera; camera_grad=True on rasterize_gaussians /
GaussianRasterizer.forward, render_api.render / render_ex / pts2render).

The spec is the autograd derivative of the forward under the rasteriser's conventions, so the gradients are checked against the dense fp64
autograd reference (oracle.gsr_torch_ref.render_ref with the camera tensors as leaves) on small scenes, and at full size against the rigid-motion
identity: moving the camera by E(xi) is moving the scene by E(xi), whose derivative the per-Gaussian gradients of the same backward give.
"""
import numpy as np
import pytest

from conftest import fragile_bounds, gaussians, simple_scene
from raster_run import batch_data, batch_with_xyz_grad, device as _dev, leaves, rasterize, render_ex_rows, run_view, settings, to_dev

pytestmark = pytest.mark.gpu

TOL = 1e-3
VIEW_ZERO = [3, 7, 11, 15]   # row 3 of the viewmatrix: never read
PROJ_ZERO = [2, 6, 10, 14]   # row 2 of the projmatrix: never read


def _render(g, dpix, maps=None, camera_grad=True, pin=False, colors_grad=True, **kw):
    """run_view with camera gradients on by default and campos a leaf like the matrices.  maps: None or (dL_ddepth, dL_dalpha) [H,W].
    -> dict(img, radii, grads, cam: the raw camera gradients, cam_tensors)"""
    dd, da = maps if maps is not None else (None, None)
    return run_view(g, dict(img=dpix, depth=dd, alpha=da), extras=maps is not None, cam=camera_grad, pinned=pin, color_grad=colors_grad,
                    campos_leaf=True, raw_cam=True, **kw)


def _ref(g, dpix, shs=None, cov=None, aa=False, maps=None):
    """Dense fp64 reference: the camera gradients of <img, dpix> (+ <depth, dd> + <alpha, da>) with view / proj / campos as autograd leaves."""
    import torch
    from aa_ref import aa_k, cov2d0
    from oracle.gsr_torch_ref import render_ref
    dt = torch.float64

    def T(x, grad=False):
        return torch.as_tensor(np.asarray(x, np.float64)).clone().requires_grad_(grad)

    view, proj, campos = T(g["view"], True), T(g["proj"], True), T(g["campos"], True)
    m3 = T(g["means3D"])
    op = T(np.asarray(g["opacities"]).reshape(-1))
    sc, rot = (None, None) if cov is not None else (T(g["scales"]), T(g["rotations"]))
    c6 = T(cov) if cov is not None else None
    if aa:
        a0, b, c0 = cov2d0(m3, view, g["W"], g["H"], g["tanfovx"], g["tanfovy"], sc, rot, c6)
        op = op * aa_k(a0, b, c0)[0]
    common = (g["W"], g["H"], g["tanfovx"], g["tanfovy"])
    img, _ = render_ref(m3, None if shs is not None else T(g["colors"]), op, sc, rot, view, proj, *common, T(g["bg"]),
                        shs=T(shs) if shs is not None else None, sh_degree=3, campos=campos, cov3D_precomp=c6)
    loss = (img * T(dpix)).sum()
    if maps is not None:
        vf = view.reshape(16)
        z = vf[2] * m3[:, 0] + vf[6] * m3[:, 1] + vf[10] * m3[:, 2] + vf[14]
        cols = torch.stack([z, torch.ones_like(z), torch.zeros_like(z)], 1)
        da_img, _ = render_ref(m3, cols, op, sc, rot, view, proj, *common, torch.zeros(3, dtype=dt), cov3D_precomp=c6)
        loss = loss + (da_img[0] * T(maps[0])).sum() + (da_img[1] * T(maps[1])).sum()
    gs = torch.autograd.grad(loss, [view, proj, campos], allow_unused=True)
    return {k: (np.zeros(n) if x is None else x.detach().numpy().reshape(-1)) for k, x, n in zip(("view", "proj", "campos"), gs, (16, 16, 3))}


def _small_scene(seed, n=40, side=48):
    rng = np.random.default_rng(seed)
    cam = simple_scene(side, side, 40.0, bg=(0.2, 0.1, 0.3))
    # a camera that is not the identity: every entry of the matrices takes part
    ang = 0.15
    R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    w2c = np.eye(4)
    w2c[:3, :3] = R
    w2c[:3, 3] = [0.05, -0.03, 0.1]
    view = np.asarray(cam["view"], np.float64)          # transposed (row-vector) form, as the reference passes it
    proj_only = np.linalg.inv(view) @ np.asarray(cam["proj"], np.float64)
    view2 = (w2c @ view.T).T
    cam = dict(cam, view=view2.astype(np.float32), proj=(view2 @ proj_only).astype(np.float32),
               campos=np.linalg.inv(view2.T)[:3, 3].astype(np.float32))
    xyz = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n), rng.uniform(1.5, 3.0, n)], 1)
    xyz = (np.linalg.inv(w2c) @ np.c_[xyz, np.ones(n)].T).T[:, :3]
    scale = np.exp(rng.uniform(np.log(0.002), np.log(0.06), (n, 3)))
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return dict(cam, **gaussians(xyz, rng.uniform(0, 1, (n, 3)), rng.uniform(0.1, 0.95, n), scale, q)), rng


CASES = ["colors", "shs", "cov3D_precomp", "depth_alpha", "antialias"]


def _case(case):
    from gps_gaussian_amd import synthetic as S
    g, rng = _small_scene(5)
    P = g["means3D"].shape[0]
    dpix = rng.standard_normal((3, g["H"], g["W"])).astype(np.float32)
    kw = {}
    if case == "shs":
        kw["shs"] = S.random_shs(P, 16)
    if case == "cov3D_precomp":
        kw["cov"] = S.covariances_from(g["scales"], g["rotations"]).astype(np.float32)
    if case == "depth_alpha":
        kw["maps"] = (rng.standard_normal((g["H"], g["W"])).astype(np.float32), rng.standard_normal((g["H"], g["W"])).astype(np.float32))
    if case == "antialias":
        kw["aa"] = True
    return g, dpix, kw


def _fragility(g, kw):
    """(solid, touched) of the fp32 oracle run with the opacities the kernels see."""
    from oracle.gsr_oracle import OracleRasterizer
    from aa_ref import opacity_eff
    op = opacity_eff(g, kw.get("cov")).reshape(-1, 1).astype(np.float32) if kw.get("aa") else g["opacities"]
    o = OracleRasterizer("f32")
    cov = kw.get("cov")
    o.forward(g["means3D"], None if kw.get("shs") is not None else g["colors"], op, None if cov is not None else g["scales"],
              None if cov is not None else g["rotations"], g["view"], g["proj"], g["W"], g["H"], g["tanfovx"], g["tanfovy"], g["bg"],
              shs=kw.get("shs"), sh_degree=3, campos=g["campos"], cov3D_precomp=cov)
    solid, touched, _ = fragile_bounds(o, None)
    return solid, touched


@pytest.mark.parametrize("lists", ["scanned", "direct"])
@pytest.mark.parametrize("family", ["valu", "tiles"])
@pytest.mark.parametrize("case", CASES)
def test_against_the_dense_fp64_reference(case, family, lists, monkeypatch):
    monkeypatch.setenv("GPSGS_COMPOSITE", family)
    monkeypatch.setenv("GPSGS_LISTS", lists)
    g, dpix, kw = _case(case)
    solid, _ = _fragility(g, kw)
    assert solid.all(), "the scene has fragile pixels: the comparison would not be meaningful"
    r = _render(g, dpix, **kw)
    assert (r["radii"] > 0).sum() >= g["means3D"].shape[0] // 2
    ref = _ref(g, dpix, **kw)
    for k in ("view", "proj", "campos"):
        mine = r["cam"][k].cpu().numpy().reshape(-1).astype(np.float64)
        assert r["cam"][k].shape == r["cam_tensors"][("view", "proj", "campos").index(k)].shape
        s = np.abs(ref[k]).max()
        if k == "campos" and kw.get("shs") is None:
            assert (mine == 0).all() and s == 0
            continue
        assert s > 0, k
        err = np.abs(mine - ref[k]).max()
        assert err <= TOL * s, "%s: %.3e of %.3e\nmine %s\nref  %s" % (k, err, s, mine, ref[k])
    assert (r["cam"]["view"].reshape(-1)[VIEW_ZERO] == 0).all()
    assert (r["cam"]["proj"].reshape(-1)[PROJ_ZERO] == 0).all()


# ---- full size: the rigid-motion identity ---------------------------------------------------------------------------------------------------------

def _qmul_pure(w, q):
    """[0, w] (x) q for q = (r, x, y, z), w [3] -> [P, 4]"""
    r, u = q[:, :1], q[:, 1:]
    return np.concatenate([-(u @ w)[:, None], r * w[None, :] + np.cross(w[None, :], u)], 1)


def test_rigid_motion_identity_at_config2():
    import torch
    from gps_gaussian_amd import synthetic as S
    dev = _dev()
    g = S.make_scene(1024, 600000)
    q = g["rotations"].astype(np.float64)
    g["rotations"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    dpix = np.random.default_rng(91).standard_normal((3, g["H"], g["W"])).astype(np.float32)
    t = leaves(g, grad=True)
    xi = torch.zeros(6, dtype=torch.float32, device=dev, requires_grad=True)   # (omega, v)
    w, v = xi[:3], xi[3:]
    z = torch.zeros((), device=dev)
    tw = torch.stack([torch.stack([z, -w[2], w[1], v[0]]), torch.stack([w[2], z, -w[0], v[1]]), torch.stack([-w[1], w[0], z, v[2]]),
                      torch.stack([z, z, z, z])])
    E = torch.eye(4, device=dev) + tw    # first order in xi: the derivative at xi = 0 is the one of exp
    Vt, Ft = torch.from_numpy(g["view"]).to(dev), torch.from_numpy(g["proj"]).to(dev)
    # the row-vector form the reference passes: camera V E  ->  (V E)^T = E^T V^T
    view, proj = E.t() @ Vt, E.t() @ Ft
    m2 = torch.zeros_like(t["means3D"], requires_grad=True)
    img, radii = rasterize(settings(g, view=view, proj=proj), t, m2, camera_grad=True)
    assert int((radii > 0).sum()) > 100000
    (img * torch.from_numpy(dpix).to(dev)).sum().backward()
    d_xi = xi.grad.double().cpu().numpy()
    dm = t["means3D"].grad.double().cpu().numpy()
    dq = t["rotations"].grad.double().cpu().numpy()
    m = g["means3D"].astype(np.float64)
    qq = g["rotations"].astype(np.float64)
    for k in range(6):
        e = np.zeros(3)
        e[k % 3] = 1.0
        if k < 3:
            terms = (dm * np.cross(e[None, :], m)).sum(1) + (dq * 0.5 * _qmul_pure(e, qq)).sum(1)
        else:
            terms = dm[:, k - 3]
        want = terms.sum()
        scale = np.abs(terms).sum()
        assert scale > 0
        assert abs(d_xi[k] - want) <= 1e-4 * scale, "generator %d: %.6e vs %.6e (scale %.3e)" % (k, d_xi[k], want, scale)


# ---- nothing else moves; determinism; batching ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["valu", "tiles"])
@pytest.mark.parametrize("colors_grad", [True, False])
def test_per_gaussian_results_are_bit_identical(family, colors_grad, monkeypatch):
    """camera_grad=True changes nothing else: image, radii and every per-Gaussian gradient keep their bits (colors_grad=False with the tile
    family: the stage-2 gradient set, GSR_FLAG_NO_COLOR_GRAD).  Two backward calls give the same camera gradients."""
    from gps_gaussian_amd import synthetic as S
    monkeypatch.setenv("GPSGS_COMPOSITE", family)
    g = S.make_scene(256, 30000)
    dpix = np.random.default_rng(17).standard_normal((3, g["H"], g["W"])).astype(np.float32)
    base = _render(g, dpix, camera_grad=False, colors_grad=colors_grad)
    a = _render(g, dpix, colors_grad=colors_grad)
    b = _render(g, dpix, colors_grad=colors_grad)
    np.testing.assert_array_equal(a["img"], base["img"])
    np.testing.assert_array_equal(a["radii"], base["radii"])
    assert set(a["grads"]) == set(base["grads"])
    for k in base["grads"]:
        np.testing.assert_array_equal(a["grads"][k], base["grads"][k], err_msg=k)
    for k in ("view", "proj"):
        x = a["cam"][k].cpu().numpy()
        assert np.abs(x).max() > 0, k
        np.testing.assert_array_equal(x, b["cam"][k].cpu().numpy(), err_msg=k)
    assert (a["cam"]["campos"].cpu().numpy() == 0).all()


def test_only_requested_outputs_and_pinned_cpu_cameras():
    """A pinned CPU camera tensor gets its gradient on the CPU, with the bits of the GPU one; a camera tensor without requires_grad gets none."""
    import torch
    from gps_gaussian_amd import synthetic as S
    g = S.make_scene(256, 30000)
    dpix = np.random.default_rng(23).standard_normal((3, g["H"], g["W"])).astype(np.float32)
    gpu = _render(g, dpix)
    cpu = _render(g, dpix, cam_device=torch.device("cpu"), pin=True)
    for k in ("view", "proj", "campos"):
        assert cpu["cam"][k].device.type == "cpu" and cpu["cam"][k].shape == gpu["cam"][k].shape
        np.testing.assert_array_equal(cpu["cam"][k].numpy(), gpu["cam"][k].cpu().numpy(), err_msg=k)
    # only the projection matrix is learnable
    dev = _dev()
    view, proj = to_dev(g["view"]), to_dev(g["proj"]).requires_grad_(True)
    img, _ = rasterize(settings(g, view=view, proj=proj), leaves(g), camera_grad=True)
    (img * torch.from_numpy(dpix).to(dev)).sum().backward()
    np.testing.assert_array_equal(proj.grad.cpu().numpy(), gpu["cam"]["proj"].cpu().numpy())
    assert view.grad is None


def _cam_leaves(data, pin=False):
    nv = data["novel_view"]
    for k in ("world_view_transform", "full_proj_transform", "camera_center"):
        x = nv[k].float().contiguous()
        if pin:
            x = x.pin_memory()
        nv[k] = x.requires_grad_(True)
    return nv


@pytest.mark.parametrize("variant", ["scanned", "direct", "repair", "pinned_cpu"])
def test_pts2render_batch_of_4_against_four_render_ex_calls(variant, monkeypatch):
    import torch
    from gps_gaussian_amd import rasterizer as RZ
    from gps_gaussian_amd import render_api
    from gps_gaussian_amd.pack import pack_views
    monkeypatch.setenv("GPSGS_COMPOSITE", "valu")
    monkeypatch.setenv("GPSGS_LISTS", "direct" if variant == "direct" else "scanned")
    B, side = 4, 64
    data = batch_with_xyz_grad(B)
    # a different camera per sample
    for i in range(B):
        data["novel_view"]["world_view_transform"][i, 3, :3] += torch.tensor([0.02 * i, -0.01 * i, 0.03 * i])
        data["novel_view"]["full_proj_transform"][i] = data["novel_view"]["world_view_transform"][i] @ (
            torch.linalg.inv(batch_data(1)["novel_view"]["world_view_transform"][0]) @ batch_data(1)["novel_view"]["full_proj_transform"][0])
    nv = _cam_leaves(data, pin=variant == "pinned_cpu")
    calls = []
    if variant == "repair":
        real = RZ._capacity_for

        def tiny_first(st, P):
            calls.append(1)
            return 64 if len(calls) <= B else real(st, P)

        monkeypatch.setattr(RZ, "_capacity_for", tiny_first)
    bg = [0.2, 0.3, 0.4]
    rng = np.random.default_rng(73)
    gi = torch.from_numpy(rng.standard_normal((B, 3, side, side)).astype(np.float32)).cuda()
    gd = torch.from_numpy(rng.standard_normal((B, 1, side, side)).astype(np.float32)).cuda()
    render_api.pts2render(data, bg, with_depth_alpha=True, camera_grad=True)
    ((nv["img_pred"] * gi).sum() + (nv["depth_pred"] * gd).sum()).backward()
    if variant == "repair":
        assert len(calls) > B
        monkeypatch.setattr(RZ, "_capacity_for", real)
    got = {k: nv[k].grad for k in ("world_view_transform", "full_proj_transform", "camera_center")}
    assert got["world_view_transform"].shape == (B, 4, 4) and got["camera_center"].shape == (B, 3)
    assert all(x.device == nv[k].device for k, x in got.items())
    # the same samples, one render_ex each
    data2 = batch_data(B)
    for i in range(B):
        data2["novel_view"]["world_view_transform"][i] = data["novel_view"]["world_view_transform"][i].detach().cpu()
        data2["novel_view"]["full_proj_transform"][i] = data["novel_view"]["full_proj_transform"][i].detach().cpu()
    nv2 = _cam_leaves(data2, pin=variant == "pinned_cpu")
    *packed, offsets = pack_views(data2)
    for i, sl, r in render_ex_rows(data2, packed, offsets, bg, camera_grad=True):
        np.testing.assert_array_equal(nv["img_pred"][i].detach().cpu().numpy(), r["img"].detach().cpu().numpy())
        ((r["img"] * gi[i]).sum() + (r["depth"] * gd[i]).sum()).backward()
    for k in ("world_view_transform", "full_proj_transform"):
        a, b = got[k].cpu().numpy(), nv2[k].grad.cpu().numpy()
        assert np.abs(a).max() > 0
        np.testing.assert_array_equal(a, b, err_msg=k)
    assert (got["camera_center"].cpu().numpy() == 0).all()


# ---- it is usable: photometric pose refinement ---------------------------------------------------------------------------------------------------

def _se3(xi):
    import torch
    w, v = xi[:3], xi[3:]
    z = torch.zeros((), dtype=xi.dtype)
    A = torch.stack([torch.stack([z, -w[2], w[1], v[0]]), torch.stack([w[2], z, -w[0], v[1]]), torch.stack([-w[1], w[0], z, v[2]]),
                     torch.stack([z, z, z, z])])
    return torch.linalg.matrix_exp(A)


def test_pose_refinement_converges():
    """A novel camera perturbed by ~1 degree and ~1 cm is pulled back by Adam on an se(3) pose through the camera gradients."""
    import torch
    from gps_gaussian_amd import synthetic as S
    dev = _dev()
    g = S.make_scene(256, 30000)
    t = leaves(g)
    Vt, Ft = torch.from_numpy(g["view"]).double(), torch.from_numpy(g["proj"]).double()

    def render(view, proj, camera_grad=False):
        img, _ = rasterize(settings(g, view=view, proj=proj), t, camera_grad=camera_grad)
        return img

    target = render(Vt.float().to(dev), Ft.float().to(dev)).detach()
    axis = np.array([0.6, -0.48, 0.64])
    xi0 = torch.tensor(np.r_[np.deg2rad(1.0) * axis, 0.01 * np.array([0.6, 0.8, 0.0])], dtype=torch.float64)
    E0 = _se3(xi0)
    Vp, Fp = E0.t() @ Vt, E0.t() @ Ft          # the perturbed camera V E0 (row-vector form)
    xi = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([xi], lr=2e-3)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: 1.0 - k / 100.0)

    def err(x):   # radians and metres (the scene is ~1-2 m away)
        return float(torch.linalg.norm(x.detach() + xi0))   # E0 E(xi) = I at xi = -xi0

    e0 = err(xi)
    for _ in range(100):
        opt.zero_grad()
        E = _se3(xi)
        view = (E.t() @ Vp).float().to(dev)
        proj = (E.t() @ Fp).float().to(dev)
        img = render(view, proj, camera_grad=True)
        loss = ((img - target) ** 2).mean()
        loss.backward()
        opt.step()
        sched.step()
    assert err(xi) < 0.25 * e0, (err(xi), e0)
