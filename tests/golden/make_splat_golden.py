"""Generates tests/golden/splat_golden.npz by IMPORTING the reference (a read-only checkout, tools/refenv.reference_dir()): the stage-1 validation render's geometry
(lib/TaichiRender.py:26-51 -- flow2depth, depth2pc, perspective into the novel view, 1 / (z + 1e-8), lib/utils.py) in torch on CPU, and the
z-buffer of oracle/aux_oracle.c::zsplat_oracle over those points, at 256^2 and at the real 1024^2.

Run in the build container only:   python tests/golden/make_splat_golden.py
The tests read the committed .npz and rebuild the inputs with `scene()` below (exact float32 arithmetic, no stored maps).

Stored per size S (B = 1, two source views, N = S*S points each):
  s{S}_extr      [3, 3, 4] extrinsics of lmain, rmain, novel view (scene() computes them with cos / sin; the tests use the stored bits)
  s{S}_sel       4096 global point ids (view * N + i) per view, drawn at random
  s{S}_proj      [len(sel), 3] the reference's projected (x, y, 1/z) of those points
  s{S}_winner    [S, S] int32: the global id of the point zsplat_oracle keeps at each novel-view pixel, -1 where none lands
                 (the image is the winner's colour from scene()'s images, -1 for the background)
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SIZES = (256, 1024)


def _rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def scene(S, extrs=None):
    """Two source views of a bumpy surface ~2.5 m away, seen by a stereo pair rotated +-8 degrees about y, and the novel view half way.
    flow / mask / img come from float32 formulas (correctly rounded +, *, /), so every machine rebuilds the same bits; the cameras are stored."""
    u = np.arange(S, dtype=np.float32)[None, :].repeat(S, 0)
    v = np.arange(S, dtype=np.float32)[:, None].repeat(S, 1)
    fx = np.float32(1.1 * S)
    views = []
    for k, ang in enumerate((-0.14, 0.14)):
        intr = np.array([[fx, 0, 0.5 * S + 3 * k], [0, fx, 0.5 * S - 2], [0, 0, 1]], np.float32)
        ref_intr = intr.copy()
        ref_intr[0, 2] += np.float32(11.0 + k)
        R = _rot_y(ang)
        t = -R @ np.array([0.0, 0.05, -2.5]) + np.array([0.0, 0.0, 2.5])
        extr = np.concatenate([R, t[:, None]], 1).astype(np.float32) if extrs is None else extrs[k]
        tf = np.float32(0.12 * fx)
        a = (u - np.float32(0.5 * S)) / np.float32(S)
        b = (v - np.float32(0.5 * S)) / np.float32(S)
        z = np.float32(2.5) + np.float32(0.6) * (a * a + b * b) - np.float32(0.3) * a * b + np.float32(0.01 * k)
        d = np.float32(1.0) / z
        offset = ref_intr[0, 2] - intr[0, 2]
        flow = (offset + d * tf).astype(np.float32)   # flow2depth inverts this: d = -(offset - flow) / Tf_x
        iu, iv = np.arange(S)[None, :], np.arange(S)[:, None]
        mask = ((4 * (iu - S // 2) ** 2 + (iv - S // 2) ** 2) < (2 * S * S) // 9).astype(np.float32)
        mask[(iu + 3 * iv) % 97 == 0] = 0          # holes: invalid points inside the silhouette
        q = (iu * 7 + iv * 3 + 50 * k) % 256
        img = np.stack([((q + 85 * c) % 256).astype(np.float32) / np.float32(127.5) - np.float32(1.0) for c in range(3)])
        views.append(dict(flow=flow[None, None], mask=mask[None, None], img=img[None], intr=intr[None], ref_intr=ref_intr[None], extr=extr[None],
                          tf=np.array([tf], np.float32)))
    intr_n = (0.5 * views[0]["intr"][0] + 0.5 * views[1]["intr"][0]).astype(np.float32)
    Rn = _rot_y(0.0)
    tn = 0.5 * views[0]["extr"][0][:, 3] + 0.5 * views[1]["extr"][0][:, 3]
    extr_n = np.concatenate([Rn, tn[:, None]], 1).astype(np.float32) if extrs is None else extrs[2]
    return dict(views=views, novel_intr=intr_n[None], novel_extr=extr_n[None], S=S)


def reference_projection(sc):
    """[2, N, 3] projected points by the reference's lib/utils.py (torch, CPU) and the [2, N] validity, as lib/TaichiRender.py:31-51 does."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import refenv
    ref = refenv.reference_dir()
    if ref is None:
        raise SystemExit("make_splat_golden: needs a reference checkout (tools/refenv.py: $GPSGS_REFERENCE)")
    sys.path.insert(0, ref)
    from lib.utils import depth2pc, flow2depth, perspective
    calib = torch.matmul(torch.from_numpy(sc["novel_intr"]), torch.from_numpy(sc["novel_extr"]))
    out, valids = [], []
    for vw in sc["views"]:
        dv = {"flow_pred": torch.from_numpy(vw["flow"]), "mask": torch.from_numpy(vw["mask"]), "ref_intr": torch.from_numpy(vw["ref_intr"]),
              "intr": torch.from_numpy(vw["intr"]), "Tf_x": torch.from_numpy(vw["tf"]), "extr": torch.from_numpy(vw["extr"])}
        depth = flow2depth(dv).clone()
        valid = depth != 0
        pts = depth2pc(depth, dv["extr"], dv["intr"])
        valid = valid.view(1, -1, 1).squeeze(2)
        pv = torch.zeros_like(pts)
        pv[valid] = pts[valid]
        pv = perspective(pv, calib)
        pv[:, :, 2:] = 1.0 / (pv[:, :, 2:] + 1e-8)
        out.append(pv[0].numpy())
        valids.append(valid[0].numpy())
    return np.stack(out), np.stack(valids)


def oracle_winner(proj, valid, S):
    """zsplat_oracle over both views in sequence; the winner's global id rides in the red channel (exact in fp32 below 2^24)."""
    aux = C.CDLL(os.path.join(ROOT, "oracle", "_build", "libaux_oracle.so"))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    N = S * S
    depth = np.zeros((1, S, S), np.float32)
    color = -np.ones((1, 3, S, S), np.float32)
    for k in range(2):
        pts = np.zeros((1, N, 6), np.float32)
        pts[0, :, :3] = proj[k]
        pts[0, :, 3] = np.arange(N, dtype=np.float32) + k * N
        m = valid[k].astype(np.float32)[None]
        aux.zsplat_oracle(p(pts), p(m), p(depth), p(color), 1, N, S)
    return np.where(color[0, 0] < 0, -1, color[0, 0]).astype(np.int32)


def main():
    rng = np.random.default_rng(1314)
    out = {}
    for S in SIZES:
        sc = scene(S)
        proj, valid = reference_projection(sc)
        N = S * S
        sel = np.concatenate([rng.choice(N, 4096, replace=False) + k * N for k in range(2)]).astype(np.int64)
        out["s%d_sel" % S] = sel
        out["s%d_proj" % S] = proj.reshape(-1, 3)[sel]
        out["s%d_valid" % S] = valid.reshape(-1)[sel]
        out["s%d_winner" % S] = oracle_winner(proj, valid, S)
        out["s%d_extr" % S] = np.stack([sc["views"][0]["extr"][0], sc["views"][1]["extr"][0], sc["novel_extr"][0]])
        w = out["s%d_winner" % S]
        print("S=%d: %d valid points, %d covered pixels" % (S, int(valid.sum()), int((w >= 0).sum())))
    np.savez_compressed(os.path.join(HERE, "splat_golden.npz"), **out)


if __name__ == "__main__":
    main()
