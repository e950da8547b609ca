"""Reference for the per-Gaussian contribution statistics (include/gpsgs.h GsrContrib): the fp32 oracle's per-pixel blend replayed from its own
geometry and bin lists (OracleRasterizer.geom() / .binning(), read only), in upstream's order of operations.

For every pixel the tile's depth-sorted list is walked front to back with upstream's decisions -- power > 0 skip, alpha = min(0.99, o exp(power))
< 1/255 skip, T (1 - alpha) < 1e-4 stop -- and each blended pair adds w = alpha T to its Gaussian's sum, raises its max and counts one pixel.
"""
import numpy as np


def contrib_stats(oracle):
    """-> (weight_sum fp64 [P], weight_max fp64 [P], pixel_count int64 [P]) of the oracle's last forward (pass the kernel's effective opacities to
    that forward for an antialiased view)."""
    P, _, _, W, H, _, _ = oracle.args
    g = oracle.geom()
    b = oracle.binning()
    xy = g["xy"].astype(np.float32)
    co = g["conic_opacity"].astype(np.float32)
    pl = b["point_list"].astype(np.int64)
    ranges = b["ranges"]
    gx = (W + 15) // 16
    wsum = np.zeros(max(P, 1), np.float64)
    wmax = np.zeros(max(P, 1), np.float64)
    npix = np.zeros(max(P, 1), np.int64)
    one = np.float32(1.0)
    for t in range(ranges.shape[0]):
        r0, r1 = int(ranges[t, 0]), int(ranges[t, 1])
        if r1 <= r0:
            continue
        tx, ty = t % gx, t // gx
        xs = np.arange(tx * 16, min(tx * 16 + 16, W))
        ys = np.arange(ty * 16, min(ty * 16 + 16, H))
        px, py = np.meshgrid(xs.astype(np.float32), ys.astype(np.float32))
        px, py = px.reshape(-1), py.reshape(-1)
        T = np.ones(px.shape, np.float32)
        live = np.ones(px.shape, bool)
        for k in range(r0, r1):
            if not live.any():
                break
            i = pl[k]
            dx = xy[i, 0] - px
            dy = xy[i, 1] - py
            A, B, C, o = co[i]
            power = np.float32(-0.5) * (A * dx * dx + C * dy * dy) - B * dx * dy
            alpha = np.minimum(np.float32(0.99), o * np.exp(power.astype(np.float32)).astype(np.float32))
            ok = live & ~(power > 0) & ~(alpha < np.float32(1.0 / 255.0))
            test_T = T * (one - alpha)
            stop = ok & (test_T < np.float32(0.0001))
            live &= ~stop
            use = ok & ~stop
            if use.any():
                w = (alpha * T)[use]
                wsum[i] += float(np.sum(w.astype(np.float64)))
                wmax[i] = max(wmax[i], float(w.max()))
                npix[i] += int(use.sum())
            T = np.where(use, test_T, T)
    return wsum[:P], wmax[:P], npix[:P]


def fragile_in_rect(oracle, solid):
    """[P] int64: the fragile pixels (~solid) inside each Gaussian's tile rect (geom()['rect'] = x0, y0, x1, y1 in 16-pixel tiles, exclusive)."""
    g = oracle.geom()
    frag = (~solid).astype(np.int64)
    H, W = frag.shape
    S = np.zeros((H + 1, W + 1), np.int64)
    S[1:, 1:] = frag.cumsum(0).cumsum(1)
    r = g["rect"].astype(np.int64)
    x0, y0 = np.clip(r[:, 0] * 16, 0, W), np.clip(r[:, 1] * 16, 0, H)
    x1, y1 = np.clip(r[:, 2] * 16, 0, W), np.clip(r[:, 3] * 16, 0, H)
    return S[y1, x1] - S[y0, x1] - S[y1, x0] + S[y0, x0]
