"""GPU: the z-buffer point splat of the stage-1 validation render (gps-gaussian_amd/csrc/splat.hip, gps_gaussian_amd.splat).

up_zsplat against oracle/aux_oracle.c::zsplat_oracle (sequential semantics) bit for bit; order independence and determinism; the saturating
pixel index; the fused up_flow2render_dev against its own pieces (zsplat_oracle over its projected points, up_unproject_forward_dev's world
points) and against the reference's arithmetic (tests/golden/splat_golden.npz, tests/golden/make_splat_golden.py); the drop-in class."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import gps_gaussian_amd  # noqa: F401
from gps_gaussian_amd import accelerate, splat, unproject
from oracle import gsr_oracle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

_spec = importlib.util.spec_from_file_location("make_splat_golden", os.path.join(GOLDEN, "make_splat_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


def _aux():
    aux = C.CDLL(os.path.join(os.path.dirname(gsr_oracle.__file__), "_build", "libaux_oracle.so"))
    aux.zsplat_oracle.argtypes = [C.c_void_p] * 4 + [C.c_int] * 3
    return aux


def _p(a):
    assert a.flags.c_contiguous
    return a.ctypes.data_as(C.c_void_p)


def oracle_splat(pts, mask, depth, color):
    """zsplat_oracle once per view (pts [V,B,N,6], mask [V,B,N]) on copies of depth [B,res,res] / color [B,3,res,res]."""
    aux = _aux()
    depth, color = depth.copy(), color.copy()
    V, B, N, _ = pts.shape
    for v in range(V):
        aux.zsplat_oracle(_p(np.ascontiguousarray(pts[v])), _p(np.ascontiguousarray(mask[v])), _p(depth), _p(color), B, N, depth.shape[-1])
    return depth, color


def gpu_splat(pts, mask, depth, color):
    d, c = torch.from_numpy(depth).to(DEV), torch.from_numpy(color).to(DEV)
    splat.zsplat(torch.from_numpy(pts).to(DEV), torch.from_numpy(mask).to(DEV), d, c)
    torch.cuda.synchronize()
    return d.cpu().numpy(), c.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def collision_scene(rng, V, B, N, res):
    """Points built to collide: most quantised onto a few pixels, z from a small set (exact ties), beyond every border, masked, and NaN / +inf
    / -0 / negative z; |x|, |y| < 2^31 (the oracle's (int) cast)."""
    pts = np.empty((V, B, N, 6), np.float32)
    hot = rng.integers(0, res, (8, 2)).astype(np.float32)
    pick = rng.integers(0, 8, (V, B, N))
    x = hot[pick, 0] + rng.random((V, B, N), dtype=np.float32) * 0.999
    y = hot[pick, 1] + rng.random((V, B, N), dtype=np.float32) * 0.999
    spread = rng.random((V, B, N)) < 0.4
    x[spread] = rng.uniform(-2.0 * res, 3.0 * res, int(spread.sum()))
    y[spread] = rng.uniform(-2.0 * res, 3.0 * res, int(spread.sum()))
    far = rng.random((V, B, N)) < 0.01
    x[far] = rng.choice(np.float32([-1e9, 1e9, -1.5, res + 0.5]), int(far.sum()))
    zset = np.float32([0.25, 0.5, 0.5, 1.0, 2.0, -1.0, -0.0, 0.0, np.inf, -np.inf, np.nan])
    z = zset[rng.integers(0, len(zset), (V, B, N))]
    cont = rng.random((V, B, N)) < 0.3
    z[cont] = rng.standard_normal(int(cont.sum())).astype(np.float32)
    pts[..., 0], pts[..., 1], pts[..., 2] = x, y, z
    pts[..., 3:] = rng.random((V, B, N, 3), dtype=np.float32)
    mask = (rng.random((V, B, N)) < 0.85).astype(np.float32)
    mask[rng.random((V, B, N)) < 0.05] = 0.5   # exactly the threshold: kept
    depth = rng.standard_normal((B, res, res)).astype(np.float32)
    depth[rng.random((B, res, res)) < 0.1] = 0.0
    color = rng.random((B, 3, res, res), dtype=np.float32)
    return pts, mask, depth, color


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("res", [64, 257, 1024])
def test_zsplat_is_bit_equal_to_the_sequential_oracle(B, res):
    rng = np.random.default_rng(res * 10 + B)
    for N in sorted({17, res * res // 3, 2 * res * res}):
        pts, mask, depth, color = collision_scene(rng, 2, B, N, res)
        od, oc = oracle_splat(pts, mask, depth, color)
        gd, gc = gpu_splat(pts, mask, depth, color)
        assert (bits(gd) == bits(od)).all(), "depth differs at %d pixels (N=%d)" % (int((bits(gd) != bits(od)).sum()), N)
        assert (bits(gc) == bits(oc)).all(), "colour differs at %d values (N=%d)" % (int((bits(gc) != bits(oc)).sum()), N)
        assert (bits(gd) != bits(depth)).any()


def test_one_call_per_view_equals_one_call_and_runs_are_deterministic():
    rng = np.random.default_rng(7)
    res, N = 128, 40000
    pts, mask, depth, color = collision_scene(rng, 2, 2, N, res)
    pts[..., 0] = np.floor(pts[..., 0] / 32) * 32 + 1   # very few pixels, many exact z ties
    pts[..., 1] = np.floor(pts[..., 1] / 32) * 32 + 1
    pts[..., 2] = np.float32(0.5)
    one_d, one_c = gpu_splat(pts, mask, depth, color)
    d, c = gpu_splat(pts[:1], mask[:1], depth, color)
    two_d, two_c = gpu_splat(pts[1:], mask[1:], d, c)
    assert (bits(one_d) == bits(two_d)).all() and (bits(one_c) == bits(two_c)).all()
    again_d, again_c = gpu_splat(pts, mask, depth, color)
    assert (bits(one_d) == bits(again_d)).all() and (bits(one_c) == bits(again_c)).all()
    od, oc = oracle_splat(pts, mask, depth, color)
    assert (bits(one_c) == bits(oc)).all()


def test_pixel_index_saturates_like_v_cvt_i32_f32():
    res = 16
    xs = np.float32([1e12, -1e12, np.nan, 5.7, 5.7, 5.7])
    ys = np.float32([3.2, 4.2, 5.2, 1e12, -1e12, np.nan])
    pts = np.zeros((1, 1, 6, 6), np.float32)
    pts[0, 0, :, 0], pts[0, 0, :, 1] = xs, ys
    pts[0, 0, :, 2] = np.arange(1, 7, dtype=np.float32)
    pts[0, 0, :, 3] = np.arange(10, 16, dtype=np.float32)
    mask = np.ones((1, 1, 6), np.float32)
    d, _ = gpu_splat(pts, mask, np.zeros((1, res, res), np.float32), -np.ones((1, 3, res, res), np.float32))
    expect = {(3, res - 1): 1, (4, 0): 2, (5, 0): 3, (res - 1, 5): 4, (0, 5): 6}   # y = -1e12 (z 5) and NaN y (z 6) share row 0
    for (row, col), z in expect.items():
        assert d[0, row, col] == z, (row, col, d[0, row, col])
    assert int((d != 0).sum()) == len(expect)


def test_invalid_arguments():
    lib = gps_gaussian_amd._capi.lib()
    t = torch.zeros(64, device=DEV)
    p = C.c_void_p(t.data_ptr())
    assert lib.up_zsplat(0, 1, 4, 8, p, p, p, p, p, 0, None) == 0            # empty: nothing to do
    assert lib.up_zsplat(2, 1, 4, 8, p, p, p, p, None, 0, None) == -1
    assert lib.up_zsplat(2, 1, 4, 8, p, p, p, p, p, 8, None) == -2            # scratch smaller than up_splat_scratch_bytes
    assert lib.up_zsplat(3, 1, 2 ** 31 - 1, 8, p, p, p, p, p, 1 << 20, None) == -1   # V * N + 1 does not fit in 32 bits (rejected before any launch)


# ---- the fused flow2render -----------------------------------------------------------------------------------------------------------------
def _data(sc):
    """The reference's data dict on the device (train_stage1.py:144-146 moves every item there; get_novel_calib_for_show makes novel_view)."""
    data = {}
    for name, vw in zip(("lmain", "rmain"), sc["views"]):
        data[name] = {"flow_pred": vw["flow"], "mask": vw["mask"], "img": vw["img"], "intr": vw["intr"], "ref_intr": vw["ref_intr"],
                      "extr": vw["extr"], "Tf_x": vw["tf"]}
        data[name] = {k: torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for k, a in data[name].items()}
    data["novel_view"] = {"intr": torch.from_numpy(sc["novel_intr"]).to(DEV), "extr": torch.from_numpy(sc["novel_extr"]).to(DEV)}
    return data


def _golden_scene(S):
    g = np.load(os.path.join(GOLDEN, "splat_golden.npz"))
    return G.scene(S, g["s%d_extr" % S]), g


def perspective_f32(xyz, K, E):
    """The kernel's perspective + inverse depth in float32, operation for operation (no contraction): the bits up_flow2render_dev must give."""
    f = np.float32
    q = []
    for i in range(3):
        Ci = [f(f(f(K[i, 0] * E[0, j]) + f(K[i, 1] * E[1, j])) + f(K[i, 2] * E[2, j])) for j in range(4)]
        q.append(((Ci[0] * xyz[:, 0] + Ci[1] * xyz[:, 1]) + Ci[2] * xyz[:, 2]) + Ci[3])
    with np.errstate(all="ignore"):
        return np.stack([q[0] / q[2], q[1] / q[2], f(1.0) / (q[2] + f(1e-8))], 1).astype(np.float32)


def _fused(sc):
    data = _data(sc)
    img, pts = splat.render_views(data["lmain"], data["rmain"], data["novel_view"]["intr"], data["novel_view"]["extr"], with_points=True)
    torch.cuda.synchronize()
    return data, img.cpu().numpy(), pts.cpu().numpy()


@pytest.mark.parametrize("S", [256, 1024])
def test_fused_render_equals_its_pieces(S):
    sc, _ = _golden_scene(S)
    data, img, pts = _fused(sc)
    N = S * S
    # (a) the world points are up_unproject_forward_dev's, bit for bit: its xyz through the same perspective gives pts_out's bits
    K, E = sc["novel_intr"][0], sc["novel_extr"][0]
    six, msk = np.zeros((2, 1, N, 6), np.float32), np.zeros((2, 1, N), np.float32)
    for k, name in enumerate(("lmain", "rmain")):
        v = data[name]
        depth, xyz, valid = unproject.unproject(v["flow_pred"], v["mask"], v["ref_intr"], v["intr"], v["extr"], v["Tf_x"])
        valid = valid.cpu().numpy()[0]
        assert (np.isnan(pts[k, 0, :, 0]) == ~valid).all()
        expect = perspective_f32(xyz.cpu().numpy()[0][valid], K, E)
        assert (bits(pts[k, 0][valid]) == bits(expect)).all(), "projected points differ from unproject + perspective"
        six[k, 0, :, :3] = pts[k, 0]
        six[k, 0, :, 3:] = sc["views"][k]["img"][0].reshape(3, N).T
        msk[k, 0] = valid
    # (b) the image is zsplat_oracle's over those points, bit for bit
    _, oc = oracle_splat(six, msk, np.zeros((1, S, S), np.float32), -np.ones((1, 3, S, S), np.float32))
    assert (bits(img) == bits(oc)).all(), "%d values differ" % int((bits(img) != bits(oc)).sum())
    assert (img[0, 0] != -1).sum() > N // 10


def _winner(pts, valid, S):
    """Global id of the point zsplat_oracle keeps per pixel (-1: none), from projected points [2, N, 3]."""
    return G.oracle_winner(pts, valid, S)


@pytest.mark.parametrize("S", [256, 1024])
def test_fused_render_matches_the_reference_arithmetic(S):
    sc, g = _golden_scene(S)
    _, img, pts = _fused(sc)
    N = S * S
    flat = pts[:, 0].reshape(-1, 3)
    sel, ref = g["s%d_sel" % S], g["s%d_proj" % S]
    ok = g["s%d_valid" % S]
    assert (np.isnan(flat[sel, 0]) == ~ok).all()
    # rtol 2e-6 (the 3x3 products' summation order), plus the same 2e-6 of the image extent: x and y are pixel coordinates that pass through 0
    # at the border, where an error of the size of the summed terms (~S) is a large multiple of the result
    np.testing.assert_allclose(flat[sel][ok], ref[ok], rtol=2e-6, atol=2e-6 * S)
    # the image: the fixture's winners against ours
    valid = ~np.isnan(pts[:, 0, :, 0])
    w_gpu = _winner(np.ascontiguousarray(pts[:, 0]), valid, S)
    w_ref = g["s%d_winner" % S]
    cols = np.concatenate([sc["views"][k]["img"][0].reshape(3, N).T for k in range(2)])
    ref_img = np.where(w_ref[None] >= 0, cols[np.maximum(w_ref, 0)].transpose(2, 0, 1), np.float32(-1))
    assert (bits(img[0]) == bits(np.where(w_gpu[None] >= 0, cols[np.maximum(w_gpu, 0)].transpose(2, 0, 1), np.float32(-1)))).all()
    diff = np.argwhere((bits(img[0]) != bits(ref_img)).any(0))
    covered = int((w_ref >= 0).sum())
    unexplained = []
    for r, c in diff:
        a, b = int(w_gpu[r, c]), int(w_ref[r, c])
        if a < 0 or b < 0:
            unexplained.append((r, c))
            continue
        pa, pb = flat[a], flat[b]
        near_edge = any(abs(t - np.round(t)) <= 2e-4 for t in (pa[0], pa[1], pb[0], pb[1]))
        near_z = abs(int(bits(pa[2:3])[0]) - int(bits(pb[2:3])[0])) <= 4
        if not (near_edge or near_z):
            unexplained.append((r, c))
    print("S=%d: %d of %d covered pixels differ from the reference's arithmetic (%d unexplained)" % (S, len(diff), covered, len(unexplained)))
    assert not unexplained, unexplained[:10]
    assert len(diff) <= 1e-3 * covered


def test_taichi_render_batch_drop_in():
    S = 256
    sc, _ = _golden_scene(S)
    _, img, _ = _fused(sc)
    data = _data(sc)
    for name in ("lmain", "rmain"):   # a batch of 2 (val_loader batch_size=2) rendered by TaichiRenderBatch(bs=1): only sample 0, as the reference
        data[name] = {k: torch.cat([t, t.flip(-1) if t.dim() == 4 else t]) for k, t in data[name].items()}
    data["novel_view"] = {k: torch.cat([t, t]) for k, t in data["novel_view"].items()}
    before = accelerate.calls["splat"]
    out = splat.TaichiRenderBatch(bs=1, res=S).flow2render(data)
    assert out is data and accelerate.calls["splat"] == before + 1
    pred = data["novel_view"]["img_pred"]
    assert tuple(pred.shape) == (2, 3, S, S) and pred.dtype == torch.float32 and pred.device.type == "cuda"
    pred = pred.cpu().numpy()
    assert (bits(pred[0]) == bits(img[0])).all()
    assert (pred[1] == -1).all() and (pred[0] == -1).any()
    two = splat.TaichiRenderBatch(bs=2, res=S).flow2render(data)["novel_view"]["img_pred"].cpu().numpy()
    assert (bits(two[0]) == bits(img[0])).all() and (two[1] != -1).any()
