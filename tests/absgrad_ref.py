"""Two references for the absolute screen-space gradient (include/gpsgs.h GsrAbsGrad): absgrad[i] = sum over pixels p of |dL_p / dmean2D_i|, in the
units of means2D.grad[:, :2] (NDC-scaled).  Neither reuses the kernel's formula (moments of s = dL/dG G, finished at flush time):

  * absgrad_jacobian: autograd through the fp64 torch renderer (oracle/gsr_torch_ref.py), one backward per pixel -- the definition itself.  Dense
    (pixels x Gaussians): tiny scenes only;
  * absgrad_replay: the fp32 oracle's blend replayed per 16 x 16 tile from its own geometry and bin lists (as tests/contrib_ref.py does), front to
    back with upstream's fp32 decisions, then back to front in fp64 with upstream's recurrence.  Any scene the oracle can render.

tests/test_absgrad_ref.py pins them against each other and against the oracle's own backward before they judge a kernel.
"""
import numpy as np


def tiny_scene(seed, n=40, W=24, H=16, fx=20.0):
    """simple_scene(24, 16, 20.0) with 40 random Gaussians, scales log-uniform in 0.02 .. 0.3 (0.1 .. 4 pixels of sigma at these depths)."""
    from conftest import gaussians, simple_scene
    rng = np.random.default_rng(seed)
    cam = simple_scene(W, H, fx, bg=(0.2, 0.1, 0.3))
    xyz = np.stack([rng.uniform(-1.0, 1.0, n), rng.uniform(-0.7, 0.7, n), rng.uniform(1.5, 3.0, n)], 1)
    scale = np.exp(rng.uniform(np.log(0.02), np.log(0.3), (n, 3)))
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return dict(cam, **gaussians(xyz, rng.uniform(0, 1, (n, 3)), rng.uniform(0.05, 0.95, n), scale, q))


def norm_err(a, ref):
    """The suite's normalised error |a - ref| / (|ref| + 1e-3 max|ref|), elementwise."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.abs(a - ref) / (np.abs(ref) + 1e-3 * (np.abs(ref).max() + 1e-30))


def absgrad_jacobian(scene, dpix):
    """-> (absgrad fp64 [P, 2], signed fp64 [P, 2]): per pixel p the loss L_p = sum_c img[c, p] dpix[c, p] of the fp64 reference render, its gradient
    with respect to every Gaussian's NDC offset (upstream's dL_dmeans2D[:, :2]) for all pixels at once (is_grads_batched), then sum_p |J| and sum_p J."""
    import torch
    from oracle.gsr_torch_ref import render_ref
    dt = torch.float64
    t = {k: torch.as_tensor(np.asarray(scene[k])).to(dt) for k in ("means3D", "colors", "opacities", "scales", "rotations", "view", "proj", "bg")}
    P = t["means3D"].shape[0]
    off = torch.zeros(P, 2, dtype=dt, requires_grad=True)
    W, H = scene["W"], scene["H"]
    img, _ = render_ref(t["means3D"], t["colors"], t["opacities"].reshape(-1), t["scales"], t["rotations"], t["view"], t["proj"], W, H,
                        scene["tanfovx"], scene["tanfovy"], t["bg"], 1.0, off)
    losses = (img * torch.as_tensor(np.asarray(dpix)).to(dt)).sum(0).reshape(-1)  # [H W]
    if not losses.requires_grad:
        z = np.zeros((P, 2))
        return z, z.copy()
    (J,) = torch.autograd.grad(losses, off, grad_outputs=torch.eye(H * W, dtype=dt), is_grads_batched=True)  # [H W, P, 2]
    return J.abs().sum(0).numpy(), J.sum(0).numpy()


def absgrad_replay(oracle, dpix):
    """-> (absgrad fp64 [P, 2], signed fp64 [P, 2]) of the oracle's last forward (pass the kernel's effective opacities to that forward for an
    antialiased view).  A pair that is blended is a pair that receives gradient: in front of the pixel's last contributor, not power > 0,
    alpha >= 1/255.  Back to front, with acc the colour seen behind the splat:
        dL/dalpha = ((c_i - acc) . dpix) T_i - T_final / (1 - alpha) (bg . dpix),   acc <- alpha c_i + (1 - alpha) acc,   s = opacity dL/dalpha G
        t_x = 0.5 W s (-A d_x - B d_y),   t_y = 0.5 H s (-C d_y - B d_x),   d = mean2D - pixel."""
    P, a, _, W, H, _, _ = oracle.args
    g = oracle.geom()
    b = oracle.binning()
    xy = g["xy"].astype(np.float32)
    co = g["conic_opacity"].astype(np.float32)
    rgb = oracle.rgb().astype(np.float64)
    bg = np.asarray(a["bg"], np.float64)
    pl = b["point_list"].astype(np.int64)
    ranges = b["ranges"]
    dpix = np.asarray(dpix, np.float64).reshape(3, H, W)
    gx = (W + 15) // 16
    ab = np.zeros((max(P, 1), 2), np.float64)
    sg = np.zeros((max(P, 1), 2), np.float64)
    one = np.float32(1.0)
    for t in range(ranges.shape[0]):
        r0, r1 = int(ranges[t, 0]), int(ranges[t, 1])
        if r1 <= r0:
            continue
        tx, ty = t % gx, t // gx
        xs = np.arange(tx * 16, min(tx * 16 + 16, W))
        ys = np.arange(ty * 16, min(ty * 16 + 16, H))
        ix, iy = np.meshgrid(xs, ys)
        ix, iy = ix.reshape(-1), iy.reshape(-1)
        px, py = ix.astype(np.float32), iy.astype(np.float32)
        dp = dpix[:, iy, ix]  # [3, n]
        T = np.ones(px.shape, np.float32)
        live = np.ones(px.shape, bool)
        trail = []  # per walked entry: (Gaussian, use, alpha, T in front of it, G, dx, dy)
        for k in range(r0, r1):
            if not live.any():
                break
            i = pl[k]
            dx = xy[i, 0] - px
            dy = xy[i, 1] - py
            A, B, C, o = co[i]
            power = np.float32(-0.5) * (A * dx * dx + C * dy * dy) - B * dx * dy
            G = np.exp(power.astype(np.float32)).astype(np.float32)
            alpha = np.minimum(np.float32(0.99), o * G)
            ok = live & ~(power > 0) & ~(alpha < np.float32(1.0 / 255.0))
            test_T = T * (one - alpha)
            stop = ok & (test_T < np.float32(0.0001))
            live &= ~stop
            use = ok & ~stop
            if use.any():
                trail.append((i, use, alpha, T, G, dx, dy))
            T = np.where(use, test_T, T)
        T_final = T.astype(np.float64)
        bg_dot = bg @ dp
        acc = np.zeros((3, px.shape[0]), np.float64)
        for i, use, alpha, Ti, G, dx, dy in reversed(trail):
            al = np.where(use, alpha, 0).astype(np.float64)
            c = rgb[i][:, None]
            dLda = ((c - acc) * dp).sum(0) * Ti.astype(np.float64) - T_final / (1.0 - al) * bg_dot
            acc = al * c + (1.0 - al) * acc
            A, B, C, o = co[i].astype(np.float64)
            s = np.where(use, o * dLda * G.astype(np.float64), 0.0)
            dx, dy = dx.astype(np.float64), dy.astype(np.float64)
            t_x = 0.5 * W * s * (-A * dx - B * dy)
            t_y = 0.5 * H * s * (-C * dy - B * dx)
            ab[i, 0] += np.abs(t_x).sum()
            ab[i, 1] += np.abs(t_y).sum()
            sg[i, 0] += t_x.sum()
            sg[i, 1] += t_y.sum()
    return ab[:P], sg[:P]
