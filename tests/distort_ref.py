"""References for the depth-distortion map (include/gpsgs.h GsrDistort): per pixel, over the splats blended into the image there,
distortion = sum_i sum_j w_i w_j |z_i - z_j| with w = alpha T and z the view-space depth.  Neither reuses the kernel's running-sum form
(2 sum_i w_i (z_i A_<i - D_<i) forward, suffix sums backward):

  * distort_definition: the pairwise double sum itself, in fp64, differentiated by autograd.  The weights come from renders of the fp64 torch renderer
    (oracle/gsr_torch_ref.py) with one-hot colours, three Gaussians per render, background 0; z from the view matrix.  Dense (Gaussians x Gaussians x
    pixels): tiny scenes only;
  * dense_definition: the same double sum for scenes in which every splat is blended into every pixel (no decisions): the blend in closed form,
    all pairs at once -- stacks of a hundred splats in a fraction of a second;
  * distort_replay: the fp32 oracle's blend replayed per 16 x 16 tile from its own geometry and bin lists (as tests/absgrad_ref.py does): fp32
    decisions, fp64 sums, in the GAP form -- the list is in depth order, so every gap z_{k+1} - z_k is crossed by the pairs (i <= k < j):
    distortion = 2 sum_k (z_{k+1} - z_k) A_<=k (A_tot - A_<=k), and d dist / d w_i = 2 sum_j w_j |z_i - z_j| = 2 (L_i + R_i) with L_i = sum_{k<i} gap_k A_<=k,
    R_i = sum_{k>=i} gap_k (A_tot - A_<=k).  Nothing in it cancels.  Any scene the oracle can render.

tests/test_distort_ref.py pins them against each other before they judge a kernel.
"""
import numpy as np


def _t64(scene):
    import torch
    return {k: torch.as_tensor(np.asarray(scene[k])).to(torch.float64).clone()
            for k in ("means3D", "colors", "opacities", "scales", "rotations", "view", "proj", "bg")}


def view_depth(means3D, view):
    """View-space depth of every Gaussian: the third row of the transform (view: flat [16], column-major, as the renderers take it)."""
    v = view.reshape(16)
    return means3D[:, 0] * v[2] + means3D[:, 1] * v[6] + means3D[:, 2] * v[10] + v[14]


def blend_weights(scene, t, off):
    """w [P, H W] fp64 (a torch graph over the leaves in t and the NDC offsets off): renders of the fp64 reference with one-hot colours, three
    Gaussians per render, background 0 -- channel c of render r is the weight map of Gaussian 3 r + c."""
    import torch
    from oracle.gsr_torch_ref import render_ref
    dt = torch.float64
    P, W, H = t["means3D"].shape[0], scene["W"], scene["H"]
    rows = []
    for r in range(0, P, 3):
        col = torch.zeros(P, 3, dtype=dt)
        for c in range(min(3, P - r)):
            col[r + c, c] = 1.0
        img, _ = render_ref(t["means3D"], col, t["opacities"].reshape(-1), t["scales"], t["rotations"], t["view"], t["proj"], W, H,
                            scene["tanfovx"], scene["tanfovy"], torch.zeros(3, dtype=dt), 1.0, off)
        rows.append(img.reshape(3, -1)[:min(3, P - r)])
    return torch.cat(rows, 0)


def pairwise(w, z):
    """sum_i sum_j w_i w_j |z_i - z_j| per pixel: w [P, N], z [P] (torch) -> [N]"""
    import torch
    return torch.einsum("ip,jp,ij->p", w, w, (z[:, None] - z[None, :]).abs())


def ordered(w, z):
    """2 sum_i w_i (z_i A_<i - D_<i) with the list in the renderers' order (fp32 depth, ties by index): w [P, N], z [P] (torch) -> [N]"""
    import torch
    order = torch.argsort(z.to(torch.float32), stable=True)
    ws, zs = w[order], z[order]
    A = torch.cumsum(ws, 0) - ws
    D = torch.cumsum(ws * zs[:, None], 0) - ws * zs[:, None]
    return 2.0 * (ws * (zs[:, None] * A - D)).sum(0)


def distort_definition(scene, g, dpix=None, gdepth=None, galpha=None, camera=False):
    """-> (map fp64 [H, W], dict of fp64 gradients named like the oracle's: means3D, colors, opacities [P,1], scales, rotations, means2D [P,3]) of
    L = sum_p g dist (+ sum dpix img + sum gdepth depth + sum galpha alpha: the image with the scene's colours and background, depth = sum w z,
    alpha = sum w, background 0).  camera: also the gradients of the view and projection matrices ([4,4], as the scene holds them)."""
    import torch
    from oracle.gsr_torch_ref import render_ref
    dt = torch.float64
    t = _t64(scene)
    leaves = ["means3D", "colors", "opacities", "scales", "rotations"] + (["view", "proj"] if camera else [])
    for k in leaves:
        t[k].requires_grad_(True)
    P, W, H = t["means3D"].shape[0], scene["W"], scene["H"]
    off = torch.zeros(P, 2, dtype=dt, requires_grad=True)
    w = blend_weights(scene, t, off)
    z = view_depth(t["means3D"], t["view"])
    dist = pairwise(w, z)

    def as64(a):
        return torch.as_tensor(np.asarray(a)).to(dt).reshape(-1)

    loss = (dist * as64(g)).sum()
    if dpix is not None:
        img, _ = render_ref(t["means3D"], t["colors"], t["opacities"].reshape(-1), t["scales"], t["rotations"], t["view"], t["proj"], W, H,
                            scene["tanfovx"], scene["tanfovy"], t["bg"], 1.0, off)
        loss = loss + (img.reshape(-1) * as64(dpix)).sum()
    if gdepth is not None:
        loss = loss + ((w * z[:, None]).sum(0) * as64(gdepth)).sum()
    if galpha is not None:
        loss = loss + (w.sum(0) * as64(galpha)).sum()
    gs = torch.autograd.grad(loss, [t[k] for k in leaves] + [off], allow_unused=True)
    out = {k: (torch.zeros_like(t[k]) if gr is None else gr).detach().numpy() for k, gr in zip(leaves, gs[:-1])}
    out["opacities"] = out["opacities"].reshape(-1, 1)
    out["means2D"] = np.concatenate([gs[-1].detach().numpy(), np.zeros((P, 1))], 1)
    return dist.detach().numpy().reshape(H, W), out


def distort_replay(oracle, g):
    """-> (map fp64 [H, W], dict(opacities [P], means2D [P, 2], conic [P, 3], dz [P]) fp64) of the oracle's last forward and L = sum_p g dist.  A pair
    that is blended is a pair that receives gradient.  Per pixel, with e_i = d dist / d w_i (gap form, see above) the distortion enters the backward
    as a colour-like channel with value e_i:
        dL/dalpha_i = g (e_i T_i - sum_{k>i} e_k w_k / (1 - alpha_i)),   s = opacity dL/dalpha G,   dL/dopacity = G dL/dalpha,
        dL/dmeans2D = (0.5 W s (-A d_x - B d_y), 0.5 H s (-C d_y - B d_x)),   dL/dconic = -0.5 s (d_x^2, 2 d_x d_y, d_y^2)  [(A, B, C); B counted once],
        dL/dz_i = g 2 w_i (A_<i - A_>i),   d = mean2D - pixel."""
    P, a, _, W, H, _, _ = oracle.args
    geo = oracle.geom()
    b = oracle.binning()
    xy = geo["xy"].astype(np.float32)
    co = geo["conic_opacity"].astype(np.float32)
    zz = geo["depth"].astype(np.float32).astype(np.float64)
    pl = b["point_list"].astype(np.int64)
    ranges = b["ranges"]
    g = np.asarray(g, np.float64).reshape(H, W)
    gx = (W + 15) // 16
    n = max(P, 1)
    dmap = np.zeros((H, W), np.float64)
    d_op, d_m2, d_con, d_z = np.zeros(n), np.zeros((n, 2)), np.zeros((n, 3)), np.zeros(n)
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
        T = np.ones(px.shape, np.float32)
        live = np.ones(px.shape, bool)
        ids, al, Tf, Gs, dxs, dys = [], [], [], [], [], []
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
                ids.append(i)
                al.append(np.where(use, alpha, 0).astype(np.float64))
                Tf.append(T.astype(np.float64))
                Gs.append(np.where(use, G, 0).astype(np.float64))
                dxs.append(dx.astype(np.float64))
                dys.append(dy.astype(np.float64))
            T = np.where(use, test_T, T)
        if not ids:
            continue
        ids = np.asarray(ids)
        al, Tf, Gs, dxs, dys = (np.stack(v) for v in (al, Tf, Gs, dxs, dys))  # [n, pixels]
        w = al * Tf
        z = zz[ids]
        gap = np.diff(z)[:, None]  # [n - 1, 1], >= 0: the list is in fp32 depth order
        assert (gap >= 0).all()
        Ale = np.cumsum(w, 0)      # A_<=k
        Atot = Ale[-1]
        cross = gap * Ale[:-1] * (Atot - Ale[:-1])
        dmap[iy, ix] = 2.0 * cross.sum(0)
        zero = np.zeros((1,) + Atot.shape)
        L = np.concatenate([zero, np.cumsum(gap * Ale[:-1], 0)])                          # L_i = sum_{k<i} gap_k A_<=k
        R = np.concatenate([np.cumsum((gap * (Atot - Ale[:-1]))[::-1], 0)[::-1], zero])   # R_i = sum_{k>=i} gap_k (A_tot - A_<=k)
        e = 2.0 * (L + R)
        gp = g[iy, ix]
        ew = e * w
        behind = np.concatenate([np.cumsum(ew[::-1], 0)[::-1][1:], zero])                 # sum_{k>i} e_k w_k
        dLda = gp * (e * Tf - behind / (1.0 - al))
        cod = co[ids].astype(np.float64)
        A, B, C, o = (cod[:, c][:, None] for c in range(4))
        s = o * dLda * Gs  # (Gs is 0 where the pair is not blended)
        np.add.at(d_op, ids, (dLda * Gs).sum(1))
        np.add.at(d_m2, ids, np.stack([(0.5 * W * s * (-A * dxs - B * dys)).sum(1), (0.5 * H * s * (-C * dys - B * dxs)).sum(1)], 1))
        np.add.at(d_con, ids, np.stack([(-0.5 * s * dxs * dxs).sum(1), (-s * dxs * dys).sum(1), (-0.5 * s * dys * dys).sum(1)], 1))
        Alt = Ale - w
        np.add.at(d_z, ids, (gp * 2.0 * w * (Alt - (Atot - Ale))).sum(1))
    return dmap, dict(opacities=d_op[:P], means2D=d_m2[:P], conic=d_con[:P], dz=d_z[:P])


def _project(scene, t, off=None):
    """The fp64 projection of the renderers (oracle/gsr_torch_ref.py), differentiable by autograd in t's means3D, scales and rotations (and the NDC
    offsets off): -> (ndc [P, 2], conic [P, 3] = (A, B, C) of cov2D + 0.3 I with upstream's conic gradient, view-space depth [P]).  The frustum clamp
    of the Jacobian's t as upstream: no gradient through a clamped coordinate."""
    import torch
    from oracle.gsr_torch_ref import _Conic
    m = t["means3D"]
    W, H = scene["W"], scene["H"]
    tanx, tany = scene["tanfovx"], scene["tanfovy"]
    fx, fy = W / (2.0 * tanx), H / (2.0 * tany)
    view, proj = t["view"].reshape(16), t["proj"].reshape(16)

    def xf(mat, rows):
        return torch.stack([mat[r] * m[:, 0] + mat[4 + r] * m[:, 1] + mat[8 + r] * m[:, 2] + mat[12 + r] for r in range(rows)], 1)

    pv, ph = xf(view, 3), xf(proj, 4)
    ndc = ph[:, :2] / (ph[:, 3:4] + 1e-7)
    if off is not None:
        ndc = ndc + off
    r, x, y, z = t["rotations"].unbind(1)
    Rm = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], 1),
                      torch.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], 1),
                      torch.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1)], 1)
    Sigma = Rm @ torch.diag_embed(t["scales"] ** 2) @ Rm.transpose(1, 2)
    tz = pv[:, 2]
    limx, limy = 1.3 * tanx, 1.3 * tany
    txtz, tytz = pv[:, 0] / tz, pv[:, 1] / tz
    tx = torch.where((txtz < -limx) | (txtz > limx), (txtz.clamp(-limx, limx) * tz).detach(), pv[:, 0])
    ty = torch.where((tytz < -limy) | (tytz > limy), (tytz.clamp(-limy, limy) * tz).detach(), pv[:, 1])
    zero = torch.zeros_like(tz)
    J = torch.stack([torch.stack([fx / tz, zero, -(fx * tx) / (tz * tz)], 1), torch.stack([zero, fy / tz, -(fy * ty) / (tz * tz)], 1)], 1)
    Rw = torch.stack([torch.stack([view[0], view[4], view[8]]), torch.stack([view[1], view[5], view[9]]), torch.stack([view[2], view[6], view[10]])])
    Tm = J @ Rw
    cov = Tm @ Sigma @ Tm.transpose(1, 2)
    a, b, c = cov[:, 0, 0] + 0.3, cov[:, 0, 1], cov[:, 1, 1] + 0.3
    return ndc, torch.stack(_Conic.apply(a, b, c), 1), tz


def means3D_chain(scene, oracle, part):
    """dL/dmeans3D that the partials of distort_replay imply, through the fp64 projection differentiated by autograd: the screen-space mean (as NDC
    coordinates: dL/dmeans2D's units), the conic and the view-space depth as functions of means3D (scales, rotations, camera fixed).
    -> (with the dz term, without it) fp64 [P, 3]"""
    import torch
    dt = torch.float64
    t = _t64(scene)
    m = t["means3D"].requires_grad_(True)
    ndc, conic, tz = _project(scene, t)
    vis = torch.as_tensor(np.asarray(oracle.geom()["radii"]) > 0)
    as64 = lambda v: torch.as_tensor(np.asarray(v)).to(dt) * vis.reshape((-1,) + (1,) * (np.asarray(v).ndim - 1))  # noqa: E731
    base = (ndc * as64(part["means2D"])).sum() + (conic * as64(part["conic"])).sum()
    (without,) = torch.autograd.grad(base, m, retain_graph=True)
    (zpart,) = torch.autograd.grad((tz * as64(part["dz"])).sum(), m)
    return (without + zpart).numpy(), without.numpy()


def stack(n, W, H, opacity, scale, seed, dz=0.005, spread=0.05):
    """n splats on a W x H image, dz apart in depth from z = 2 on, within `spread` of the optical axis: the scenes dense_definition is for."""
    from conftest import gaussians, simple_scene
    rng = np.random.default_rng(seed)
    cam = simple_scene(W, H, 20.0, bg=(0.1, 0.2, 0.3))
    xyz = np.stack([rng.uniform(-spread, spread, n), rng.uniform(-spread, spread, n), 2.0 + dz * np.arange(n)], 1)
    q = rng.standard_normal((n, 4))  # anisotropic and rotated: every gradient of the stack is a real number, none an analytic zero
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return dict(cam, **gaussians(xyz, rng.uniform(0, 1, (n, 3)), opacity, scale * rng.uniform(0.8, 1.25, (n, 3)), q))


def dense_definition(scene, g):
    """distort_definition for scenes in which EVERY splat is blended into EVERY pixel (stacks of faint, wide splats): no decision is ever taken, so
    the blend is a closed form -- alpha = opacity exp(power) for all (splat, pixel) pairs at once, T the exclusive product of 1 - alpha in depth
    order -- and fp64 autograd differentiates the pairwise double sum over it.  Raises if a pair would be skipped or a pixel would saturate.
    -> (map fp64 [H, W], gradients as distort_definition's; colours: zeros)"""
    import torch
    dt = torch.float64
    t = _t64(scene)
    leaves = ["means3D", "opacities", "scales", "rotations"]
    for k in leaves:
        t[k].requires_grad_(True)
    P, W, H = t["means3D"].shape[0], scene["W"], scene["H"]
    off = torch.zeros(P, 2, dtype=dt, requires_grad=True)
    ndc, conic, tz = _project(scene, t, off)
    px, py = ((ndc[:, 0] + 1.0) * W - 1.0) * 0.5, ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    dx, dy = px[:, None] - xs.reshape(-1).to(dt)[None, :], py[:, None] - ys.reshape(-1).to(dt)[None, :]
    power = -0.5 * (conic[:, 0:1] * dx * dx + conic[:, 2:3] * dy * dy) - conic[:, 1:2] * dx * dy
    alpha = t["opacities"].reshape(-1, 1) * torch.exp(power)
    order = torch.argsort(tz.detach().to(torch.float32), stable=True)
    al = alpha[order]
    Tin = torch.cumprod(1.0 - al, 0)
    with torch.no_grad():
        if not ((power <= 0).all() and (alpha >= 2.0 / 255.0).all() and (alpha <= 0.98).all() and (Tin >= 2e-4).all() and (tz > 0.2).all()):
            raise ValueError("not a dense scene: a pair would be skipped, clamped or a pixel would saturate")
    w = torch.empty_like(al)
    w = al * torch.cat([torch.ones(1, al.shape[1], dtype=dt), Tin[:-1]], 0)
    dist = pairwise(w, tz[order])
    loss = (dist * torch.as_tensor(np.asarray(g)).to(dt).reshape(-1)).sum()
    gs = torch.autograd.grad(loss, [t[k] for k in leaves] + [off])
    out = {k: gr.detach().numpy() for k, gr in zip(leaves, gs[:-1])}
    out["opacities"] = out["opacities"].reshape(-1, 1)
    out["colors"] = np.zeros((P, 3))
    out["means2D"] = np.concatenate([gs[-1].detach().numpy(), np.zeros((P, 1))], 1)
    return dist.detach().numpy().reshape(H, W), out
