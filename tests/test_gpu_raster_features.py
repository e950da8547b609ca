"""GPU (-m gpu): the opt-in F-channel feature maps of the rasteriser (include/gpsgs.h GsrFeatures; rasterizer.rasterize_gaussians(features=...);
render_api.render_ex(features=...)).

The spec: the feature map is F more colour channels of the same blend with background 0 -- feat[c] = sum_i f[i, c] alpha_i T_i -- so every
3-column slice of it must be what the EXISTING renderer gives (VALU family) for those columns as colours and background 0, bit for bit, and the
image must be the plain VALU image.  The backward is linear in the output gradients: dL/dfeatures[:, c] is the slice runs' dL/dcolours, and every
geometry gradient is the plain run's plus the sum of the slice runs' (rounding apart).
"""
import numpy as np
import pytest

from raster_run import GEOM, batch, close as _close, run_view, scene, valu_fixture

pytestmark = pytest.mark.gpu

_valu = valu_fixture()  # the plain runs the feature runs are compared with use the VALU family too (the feature runs always do)


def _run(g, dpix=None, gfeat=None, **kw):
    """run_view (+ backward of sum(img * dpix) + sum(feat * gfeat) when either is given)."""
    return run_view(g, dict(img=dpix, feat=gfeat), **kw)


def _slices(feats, gfeat=None):
    """3-column slices of [P, F] (zero-padded) and of the map gradient [F, H, W]."""
    P, F = feats.shape
    n = (F + 2) // 3
    pad = np.zeros((P, 3 * n), np.float32)
    pad[:, :F] = feats
    out = []
    for k in range(n):
        gs = None
        if gfeat is not None:
            gs = np.zeros((3,) + gfeat.shape[1:], np.float32)
            m = min(3, F - 3 * k)
            gs[:m] = gfeat[3 * k:3 * k + m]
        out.append((np.ascontiguousarray(pad[:, 3 * k:3 * k + 3]), gs, min(3, F - 3 * k)))
    return out


def _scene(kind):
    return scene("256" if kind == "256" else "config2")


@pytest.mark.parametrize("kind,F", [("256", 1), ("256", 3), ("256", 8), ("256", 17), ("256", 64), ("cfg2", 3), ("cfg2", 17), ("cfg2", 64)])
def test_slices_forward_and_backward(kind, F):
    """Forward: each 3-column slice of the feature map is bit-equal to a plain VALU run with those columns as colours and background 0; the image
    and radii are the plain run's bits.  Backward: dL/dfeatures = the slice runs' dL/dcolours, geometry = plain + sum of slices."""
    g = _scene(kind)
    P, H, W = g["means3D"].shape[0], g["H"], g["W"]
    rng = np.random.default_rng(F)
    feats = rng.standard_normal((P, F)).astype(np.float32)
    dpix = rng.standard_normal((3, H, W)).astype(np.float32)
    gfeat = rng.standard_normal((F, H, W)).astype(np.float32)
    run = _run(g, dpix=dpix, feats=feats, gfeat=gfeat)
    plain = _run(g, dpix=dpix)
    np.testing.assert_array_equal(run["img"], plain["img"])
    np.testing.assert_array_equal(run["radii"], plain["radii"])
    assert run["feat"].shape == (F, H, W)
    geom = {k: plain["grads"][k].astype(np.float64) for k in GEOM}
    for k, (cols, gs, m) in enumerate(_slices(feats, gfeat)):
        sl = _run(g, colors=cols, bg=np.zeros(3, np.float32), dpix=gs)
        np.testing.assert_array_equal(run["feat"][3 * k:3 * k + m], sl["img"][:m], err_msg="feature slice %d" % k)
        for c in range(m):
            _close(run["grads"]["features"][:, 3 * k + c], sl["grads"]["colors"][:, c], 1e-6, "dL/dfeatures[:, %d]" % (3 * k + c))
        for key in GEOM:
            geom[key] += sl["grads"][key]
    assert np.abs(run["feat"]).max() > 0.1
    for key in GEOM:
        _close(run["grads"][key], geom[key], 1e-5, key)


def test_fp64_reference():
    """A small scene against a dense fp64 autograd reference composed from oracle.gsr_torch_ref.grads_ref: the image problem plus one 3-channel
    slice problem per three feature columns (colours = the columns, background 0, dL/dpix = the map gradient's rows).  The suite's criterion:
    the map on the pixels that sit on no branch threshold (fragile_bounds), every gradient -- dL/dfeatures and means2D included -- with
    assert_grad_parity."""
    from conftest import assert_grad_parity, fragile_bounds, oracle_render
    from gps_gaussian_amd import synthetic as S
    from oracle.gsr_torch_ref import grads_ref
    g = S.make_uniform_cloud(1500, 96, 64, seed=21, scale_med=0.02)
    P, H, W = g["means3D"].shape[0], g["H"], g["W"]
    F = 5
    rng = np.random.default_rng(22)
    feats = rng.standard_normal((P, F)).astype(np.float32)
    dpix = rng.standard_normal((3, H, W)).astype(np.float32)
    gfeat = rng.standard_normal((F, H, W)).astype(np.float32)
    run = _run(g, dpix=dpix, feats=feats, gfeat=gfeat)
    base = {k: g[k] for k in ("means3D", "colors", "opacities", "scales", "rotations", "view", "proj", "bg")}
    _, _, gr = grads_ref(base, W, H, g["tanfovx"], g["tanfovy"], dpix)
    ref = {k: np.asarray(gr[k], np.float64) for k in ("means3D", "means2D", "opacities", "scales", "rotations")}
    ref_feat = np.zeros((F, H, W))
    ref["features"] = np.zeros((P, F))
    for k, (cols, gs, m) in enumerate(_slices(feats, gfeat)):
        im, _, gk = grads_ref(dict(base, colors=cols, bg=np.zeros(3, np.float32)), W, H, g["tanfovx"], g["tanfovy"], gs)
        ref_feat[3 * k:3 * k + m] = np.asarray(im)[:m]
        ref["features"][:, 3 * k:3 * k + m] = np.asarray(gk["colors"])[:, :m]
        for key in ("means3D", "means2D", "opacities", "scales", "rotations"):
            ref[key] += np.asarray(gk[key])
    o, _, oradii = oracle_render(g, "f32")
    np.testing.assert_array_equal(run["radii"], oradii)
    solid, touched, _ = fragile_bounds(o)
    assert solid.mean() > 0.995
    err = np.abs(run["feat"] - ref_feat).max(0)
    assert err[solid].max() <= 1e-4 * max(1.0, float(np.abs(ref_feat).max())), err[solid].max()
    mine = {k: run["grads"][k].reshape(ref[k].shape) for k in ref}
    assert_grad_parity(mine, ref, touched, oradii > 0)


def test_feature_map_outside_the_loss_and_determinism():
    """A feature map outside the loss leaves every other gradient bit-identical to a plain run and gives zero dL/dfeatures; two runs give the
    same bits."""
    g = _scene("256")
    P, H, W = g["means3D"].shape[0], g["H"], g["W"]
    rng = np.random.default_rng(3)
    feats = rng.standard_normal((P, 6)).astype(np.float32)
    dpix = rng.standard_normal((3, H, W)).astype(np.float32)
    plain = _run(g, dpix=dpix)
    out = _run(g, dpix=dpix, feats=feats)
    for k in GEOM + ("colors",):
        np.testing.assert_array_equal(out["grads"][k], plain["grads"][k], err_msg=k)
    assert not np.any(out["grads"]["features"])
    gfeat = rng.standard_normal((6, H, W)).astype(np.float32)
    a = _run(g, dpix=dpix, feats=feats, gfeat=gfeat)
    b = _run(g, dpix=dpix, feats=feats, gfeat=gfeat)
    np.testing.assert_array_equal(a["feat"], b["feat"])
    for k in a["grads"]:
        np.testing.assert_array_equal(a["grads"][k], b["grads"][k], err_msg=k)


def test_empty_view():
    import torch
    from gps_gaussian_amd import synthetic as S
    g = S.make_uniform_cloud(10, 32, 24, seed=1)
    g0 = dict(g)
    for k in ("means3D", "colors", "opacities", "scales", "rotations"):
        g0[k] = g[k][:0]
    out = _run(g0, feats=np.zeros((0, 4), np.float32))
    assert out["feat"].shape == (4, 24, 32) and not np.any(out["feat"])
    torch.cuda.synchronize()


def test_capacity_repair_fills_feature_map(monkeypatch):
    from gps_gaussian_amd import rasterizer as RZ
    from gps_gaussian_amd import synthetic as S
    monkeypatch.setenv("GPSGS_LISTS", "scanned")
    g = S.make_uniform_cloud(5000, 128, 96, seed=9, scale_med=0.05)
    feats = np.random.default_rng(4).standard_normal((5000, 7)).astype(np.float32)
    ref = _run(g, feats=feats)
    calls = []
    real = RZ._capacity_for

    def tiny_first(st, P):
        calls.append(1)
        return 1024 if len(calls) == 1 else real(st, P)

    monkeypatch.setattr(RZ, "_capacity_for", tiny_first)
    out = _run(g, feats=feats)
    assert len(calls) >= 2
    np.testing.assert_array_equal(out["img"], ref["img"])
    np.testing.assert_array_equal(out["feat"], ref["feat"])
    assert np.abs(out["feat"]).max() > 0.1


@pytest.mark.parametrize("lists", ["direct", "scanned"])
def test_list_forms(monkeypatch, lists):
    monkeypatch.setenv("GPSGS_LISTS", lists)
    g = _scene("256")
    P, H, W = g["means3D"].shape[0], g["H"], g["W"]
    rng = np.random.default_rng(5)
    feats = rng.standard_normal((P, 3)).astype(np.float32)
    gfeat = rng.standard_normal((3, H, W)).astype(np.float32)
    run = _run(g, dpix=np.zeros((3, H, W), np.float32), feats=feats, gfeat=gfeat)
    sl = _run(g, colors=feats, bg=np.zeros(3, np.float32), dpix=gfeat)
    np.testing.assert_array_equal(run["feat"], sl["img"])
    _close(run["grads"]["features"], sl["grads"]["colors"], 1e-6, "dL/dfeatures")
    for k in GEOM:
        _close(run["grads"][k], sl["grads"][k], 1e-5, k)


def _cov3d(g):
    """The 3D covariances k_preprocess forms from scales + rotations (R S S^T R^T, normalised quaternion w, x, y, z), as [P, 6] upper triangles."""
    q = g["rotations"].astype(np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    r, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                  2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    M = R * g["scales"].astype(np.float64)[:, None, :]
    S = M @ M.transpose(0, 2, 1)
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).astype(np.float32)


def test_combinations():
    """Features with depth/alpha maps + antialiasing + camera gradients, with shs, with cov3D_precomp, and with colours that need no gradient
    (GSR_FLAG_NO_COLOR_GRAD, the stage-2 set): the feature map keeps the bits of a slice run with the same inputs, and dL/dfeatures and the
    geometry (camera included) match that run's."""
    g = _scene("256")
    P, H, W = g["means3D"].shape[0], g["H"], g["W"]
    rng = np.random.default_rng(6)
    feats = rng.standard_normal((P, 3)).astype(np.float32)
    gfeat = rng.standard_normal((3, H, W)).astype(np.float32)
    zero = np.zeros((3, H, W), np.float32)
    bg0 = np.zeros(3, np.float32)

    def same(run, sl, keys):
        np.testing.assert_array_equal(run["feat"], sl["img"])
        _close(run["grads"]["features"], sl["grads"]["colors"], 1e-6, "dL/dfeatures")
        for k in keys:
            _close(run["grads"][k], sl["grads"][k], 1e-5, k)

    run = _run(g, dpix=zero, feats=feats, gfeat=gfeat, extras=True, aa=True, cam=True)
    sl = _run(g, colors=feats, bg=bg0, dpix=gfeat, extras=True, aa=True, cam=True)
    np.testing.assert_array_equal(run["depth"], sl["depth"])
    same(run, sl, GEOM + ("view", "proj"))
    # cov3D_precomp instead of scales + rotations
    cov = _cov3d(g)
    run = _run(g, dpix=zero, feats=feats, gfeat=gfeat, cov=cov)
    sl = _run(g, colors=feats, bg=bg0, dpix=gfeat, cov=cov)
    same(run, sl, ("means3D", "means2D", "opacities", "cov3D_precomp"))
    # shs: the weights do not depend on the colour source (an image gradient of 0 gives the SH coefficients none)
    shs = (rng.standard_normal((P, 16, 3)) * 0.3).astype(np.float32)
    run = _run(g, dpix=zero, feats=feats, gfeat=gfeat, shs=shs)
    same(run, sl_plain_grad(g, feats, gfeat), GEOM)
    assert not np.any(run["grads"]["shs"])
    # colours that need no gradient: the per-Gaussian and feature gradients keep the bits of the run whose colours need one
    dpix = rng.standard_normal((3, H, W)).astype(np.float32)
    a = _run(g, dpix=dpix, feats=feats, gfeat=gfeat, color_grad=False)
    b = _run(g, dpix=dpix, feats=feats, gfeat=gfeat)
    assert "colors" not in a["grads"]
    np.testing.assert_array_equal(a["feat"], b["feat"])
    for k in GEOM + ("features",):
        np.testing.assert_array_equal(a["grads"][k], b["grads"][k], err_msg=k)


def sl_plain_grad(g, cols, gs):
    return _run(g, colors=cols, bg=np.zeros(3, np.float32), dpix=gs)


def test_render_ex_features():
    """render_api.render_ex(features=...) adds 'feat' with the rasteriser's bits."""
    import torch
    from gps_gaussian_amd import render_api
    from gps_gaussian_amd import synthetic as S
    g = S.make_scene(256, 30000)
    dev = torch.device("cuda:0")
    P = g["means3D"].shape[0]
    feats = torch.from_numpy(np.random.default_rng(7).standard_normal((P, 4)).astype(np.float32)).to(dev)
    nv = {"height": [g["H"]], "width": [g["W"]], "FovX": [2 * np.arctan(g["tanfovx"])], "FovY": [2 * np.arctan(g["tanfovy"])],
          "world_view_transform": torch.from_numpy(g["view"]).to(dev).reshape(1, 4, 4),
          "full_proj_transform": torch.from_numpy(g["proj"]).to(dev).reshape(1, 4, 4),
          "camera_center": torch.from_numpy(g["campos"]).to(dev).reshape(1, 3)}
    t = {k: torch.from_numpy(g[k]).to(dev) for k in ("means3D", "colors", "opacities", "scales", "rotations")}
    r = render_api.render_ex({"novel_view": nv}, 0, t["means3D"], t["colors"], t["rotations"], t["scales"], t["opacities"], g["bg"].tolist(),
                             features=feats)
    assert set(r) == {"img", "depth", "alpha", "feat"} and tuple(r["feat"].shape) == (4, g["H"], g["W"])
    assert torch.isfinite(r["feat"]).all() and r["feat"].abs().max() > 0


def _batch_feature_data(B, F=5):
    """The depth / alpha tests' B-sample stage-2 batch (tests/golden pts2render fixture) plus an F-channel map per view."""
    import torch
    data = batch(B)
    rng = np.random.default_rng(31)
    for v in ("lmain", "rmain"):
        shp = (B, F) + tuple(data[v]["img"].shape[2:])
        data[v]["sem"] = torch.from_numpy(rng.standard_normal(shp).astype(np.float32)).cuda().requires_grad_(True)
    return data


@pytest.mark.parametrize("form", ["batch", "loop"])
def test_pts2render_feature_key_against_four_render_ex_calls(form, monkeypatch):
    """pts2render(feature_key=...) at B = 4 (row-range views in the batch form): img_pred and feat_pred have the bits of four render_ex calls on the
    same packed rows, and the gradients reach the per-view feature maps and the geometry as the four calls' do."""
    import torch
    from gps_gaussian_amd import render_api
    from gps_gaussian_amd.pack import pack_features, pack_views
    monkeypatch.setenv("GPSGS_PTS2RENDER", form)
    B, F = 4, 5
    data = _batch_feature_data(B, F)
    bg = [0.2, 0.3, 0.4]
    nv = render_api.pts2render(data, bg, feature_key="sem")["novel_view"]
    assert tuple(nv["feat_pred"].shape) == (B, F, 64, 64)
    rng = np.random.default_rng(13)
    gf = torch.from_numpy(rng.standard_normal((B, F, 64, 64)).astype(np.float32)).cuda()
    gi = torch.from_numpy(rng.standard_normal((B, 3, 64, 64)).astype(np.float32)).cuda()
    ((nv["feat_pred"] * gf).sum() + (nv["img_pred"] * gi).sum()).backward()
    g_batch = {(v, k): data[v][k].grad.clone() for v in ("lmain", "rmain") for k in ("sem", "xyz")}

    data2 = _batch_feature_data(B, F)
    xyz, rgb, rot, scale, opacity, offsets, rows = pack_views(data2, return_rows=True)
    feats = pack_features(data2, "sem", rows)
    offs = offsets.tolist()
    loss = 0
    for i in range(B):
        sl = slice(offs[i], offs[i + 1])
        r = render_api.render_ex(data2, i, xyz[sl], rgb[sl], rot[sl], scale[sl], opacity[sl], bg, features=feats[sl])
        np.testing.assert_array_equal(nv["img_pred"][i].detach().cpu().numpy(), r["img"].detach().cpu().numpy())
        np.testing.assert_array_equal(nv["feat_pred"][i].detach().cpu().numpy(), r["feat"].detach().cpu().numpy())
        loss = loss + (r["feat"] * gf[i]).sum() + (r["img"] * gi[i]).sum()
    assert float(nv["feat_pred"].detach().abs().max()) > 0.1
    loss.backward()
    for (v, k), gbat in g_batch.items():
        gref = data2[v][k].grad
        s = float(gref.abs().max())
        assert s > 0
        assert float((gbat - gref).abs().max()) <= 1e-6 * s, (v, k)


def test_pack_features_follows_the_pack_rows():
    """pack_features puts pixel (b, view, s)'s feature vector on the packed row of its image pixel: the packed colours' rows equal the images packed
    as features (rgb = img * 0.5 + 0.5 in the pack), the tail rows are zeros."""
    import torch
    from gps_gaussian_amd.pack import pack_features, pack_views
    data = _batch_feature_data(2)
    xyz, rgb, rot, scale, opacity, offsets, rows = pack_views(data, return_rows=True)
    packed_img = pack_features(data, "img", rows)
    n = int(offsets[-1])
    assert torch.equal(packed_img[:n] * 0.5 + 0.5, rgb[:n])
    assert not torch.any(packed_img[n:])


def test_pts2render_feature_key_reads_nothing_back():
    """The batch form with feature_key adds no host synchronisation: the features are packed with index ops on the device."""
    import torch
    from gps_gaussian_amd import render_api
    data = _batch_feature_data(2)
    render_api.pts2render(data, [0, 0, 0], feature_key="sem")  # warm-up: capacities learnt
    torch.cuda.synchronize()
    data = _batch_feature_data(2)
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):  # set_sync_debug_mode does not police the legacy default stream
        torch.cuda.set_sync_debug_mode("error")
        try:
            feat = render_api.pts2render(data, [0, 0, 0], feature_key="sem")["novel_view"]["feat_pred"]
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert float(feat.abs().max()) > 0
