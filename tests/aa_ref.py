"""fp64 statement of the rasteriser's opt-in antialiasing (include/gpsgs.h GSR_FLAG_ANTIALIAS), for the tests.  TEST INFRASTRUCTURE ONLY.

opacity_eff = opacity * k,  k = sqrt(max(rho, 2.5e-5)),  rho = (a0 c0 - b^2) / ((a0 + 0.3)(c0 + 0.3) - b^2),  (a0, b, c0) the undilated 2D
covariance.  The 2D covariance is restated here with the conventions of oracle/gsr_torch_ref.render_ref (EWA Jacobian, the clamped view-space
x / y held constant for the gradient), so that `opacity * k(cov2D)` can be handed to render_ref as its opacities: one autograd graph for the
whole antialiased renderer (aa_grads_dense).  For clouds too large for the dense reference the C oracles are run with opacity_eff and their
dL/dopacity_eff is chained through aa_vjp, the fp64 vector-Jacobian product of opacity * k.
"""
import numpy as np
import torch

H_DIL = 0.3
RHO_MIN = 2.5e-5
_DT = torch.float64


def aa_k(a0, b, c0):
    """k and rho (fp64 tensors or numbers); below the floor k is the constant 0.005 (no gradient)."""
    D1 = (a0 + H_DIL) * (c0 + H_DIL) - b * b
    rho = (a0 * c0 - b * b) / D1
    return torch.sqrt(torch.clamp(rho, min=RHO_MIN)), rho


def aa_partials(a0, b, c0):
    """Closed-form d rho / d(a0, b, c0) (b the single off-diagonal variable)."""
    h = H_DIL
    D1 = (a0 + h) * (c0 + h) - b * b
    return (h * (c0 * c0 + h * c0 + b * b) / D1 ** 2, -2.0 * b * h * (a0 + c0 + h) / D1 ** 2, h * (a0 * a0 + h * a0 + b * b) / D1 ** 2)


def _xf(m, p, rows):
    return torch.stack([m[r] * p[:, 0] + m[4 + r] * p[:, 1] + m[8 + r] * p[:, 2] + m[12 + r] for r in range(rows)], 1)


def cov2d0(means3D, view, W, H, tanfovx, tanfovy, scales=None, rotations=None, cov3D_precomp=None, scale_modifier=1.0):
    """Undilated 2D covariance (a0, b, c0) of every Gaussian, fp64 tensors in, differentiable (render_ref's EWA conventions)."""
    view = torch.as_tensor(view).reshape(16).to(_DT)
    fx, fy = W / (2.0 * tanfovx), H / (2.0 * tanfovy)
    if cov3D_precomp is not None:
        c6 = cov3D_precomp
        Sigma = torch.stack([torch.stack([c6[:, 0], c6[:, 1], c6[:, 2]], 1), torch.stack([c6[:, 1], c6[:, 3], c6[:, 4]], 1),
                             torch.stack([c6[:, 2], c6[:, 4], c6[:, 5]], 1)], 1)
    else:
        r, x, y, z = rotations.unbind(1)
        Rm = torch.stack([
            torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], 1),
            torch.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], 1),
            torch.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1)], 1)
        Sigma = Rm @ torch.diag_embed((scale_modifier * scales) ** 2) @ Rm.transpose(1, 2)
    pv = _xf(view, means3D, 3)
    tz = pv[:, 2]
    limx, limy = 1.3 * tanfovx, 1.3 * tanfovy
    txtz, tytz = pv[:, 0] / tz, pv[:, 1] / tz
    cx = (txtz < -limx) | (txtz > limx)
    cy = (tytz < -limy) | (tytz > limy)
    tx = torch.where(cx, (txtz.clamp(-limx, limx) * tz).detach(), pv[:, 0])
    ty = torch.where(cy, (tytz.clamp(-limy, limy) * tz).detach(), pv[:, 1])
    zero = torch.zeros_like(tz)
    J = torch.stack([torch.stack([fx / tz, zero, -(fx * tx) / (tz * tz)], 1), torch.stack([zero, fy / tz, -(fy * ty) / (tz * tz)], 1)], 1)
    Rw = torch.stack([torch.stack([view[0], view[4], view[8]]), torch.stack([view[1], view[5], view[9]]), torch.stack([view[2], view[6], view[10]])])
    T = J @ Rw
    cov = T @ Sigma @ T.transpose(1, 2)
    return cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]


def _t(x, grad=False):
    return torch.as_tensor(np.asarray(x, np.float64)).clone().requires_grad_(grad)


def opacity_eff(scene, cov3D_precomp=None):
    """fp64 numpy [P]: opacity * k of every Gaussian of a scene dict (conftest layout)."""
    with torch.no_grad():
        a0, b, c0 = _cov(scene, {k: _t(scene[k]) for k in ("means3D", "scales", "rotations")}, None if cov3D_precomp is None else _t(cov3D_precomp))
        k, _ = aa_k(a0, b, c0)
    return np.asarray(scene["opacities"], np.float64).reshape(-1) * k.numpy()


def _cov(scene, t, cov):
    return cov2d0(t["means3D"], scene["view"], scene["W"], scene["H"], scene["tanfovx"], scene["tanfovy"],
                  scales=None if cov is not None else t["scales"], rotations=None if cov is not None else t["rotations"], cov3D_precomp=cov,
                  scale_modifier=float(scene.get("scale_modifier", 1.0)))


def aa_vjp(scene, g_eff, cov3D_precomp=None):
    """Chain dL/dopacity_eff (g_eff [P] or [P,1]) through opacity_eff = opacity * k(cov2D(...)) in fp64.
    -> dict: opacities [P,1] (= g k) and the contributions to means3D, scales, rotations (or cov3D_precomp)."""
    g_eff = np.asarray(g_eff, np.float64).reshape(-1)
    P = g_eff.shape[0]
    rows = np.nonzero(g_eff)[0]  # (only these: a Gaussian at or behind the camera plane has no finite k, and receives nothing)
    sub = dict(scene, **{k: np.asarray(scene[k])[rows] for k in ("means3D", "scales", "rotations", "opacities")})
    t = {k: _t(sub[k], True) for k in ("means3D", "scales", "rotations")}
    op = _t(np.asarray(sub["opacities"]).reshape(-1), True)
    cov = None if cov3D_precomp is None else _t(np.asarray(cov3D_precomp)[rows], True)
    a0, b, c0 = _cov(sub, t, cov)
    k, _ = aa_k(a0, b, c0)
    eff = op * k
    names = ["opacities", "means3D"] + (["cov3D_precomp"] if cov is not None else ["scales", "rotations"])
    leaves = [op, t["means3D"]] + ([cov] if cov is not None else [t["scales"], t["rotations"]])
    gs = torch.autograd.grad(eff, leaves, grad_outputs=torch.as_tensor(g_eff[rows]), allow_unused=True)
    out = {}
    for n, g, x in zip(names, gs, leaves):
        full = np.zeros((P,) + tuple(x.shape[1:]), np.float64)
        if g is not None:
            full[rows] = g.numpy()
        out[n] = full
    out["opacities"] = out["opacities"].reshape(-1, 1)
    return out


def chain_oracle(og, vj):
    """Oracle gradients of a run with opacity_eff (og: dL/dopacity_eff in og['opacities']) + the k chain (aa_vjp of og['opacities'])."""
    out = dict(og)
    out["opacities"] = vj["opacities"]
    for k in ("means3D", "scales", "rotations", "cov3D_precomp"):
        if k in vj and k in og:
            out[k] = og[k].astype(np.float64) + vj[k]
    return out


def aa_grads_dense(scene, dL_dpix, cov3D_precomp=None, shs=None, sh_degree=None):
    """The dense fp64 reference of the antialiased renderer: oracle.gsr_torch_ref.render_ref fed with opacity * k(cov2D), one autograd graph.
    -> (image [3,H,W], radii [P], gradients named like the oracle's)."""
    from oracle.gsr_torch_ref import render_ref
    use_cov, use_sh = cov3D_precomp is not None, shs is not None
    t = {k: _t(scene[k], True) for k in ("means3D", "scales", "rotations")}
    op = _t(np.asarray(scene["opacities"]).reshape(-1), True)
    col = None if use_sh else _t(scene["colors"], True)
    sh = _t(shs, True) if use_sh else None
    cov = _t(cov3D_precomp, True) if use_cov else None
    a0, b, c0 = _cov(scene, t, cov)
    k, _ = aa_k(a0, b, c0)
    off = torch.zeros(t["means3D"].shape[0], 2, dtype=_DT, requires_grad=True)
    img, radii = render_ref(t["means3D"], col, op * k, None if use_cov else t["scales"], None if use_cov else t["rotations"],
                            _t(scene["view"]), _t(scene["proj"]), scene["W"], scene["H"], scene["tanfovx"], scene["tanfovy"], _t(scene["bg"]),
                            float(scene.get("scale_modifier", 1.0)), off, shs=sh, sh_degree=sh_degree or 0,
                            campos=_t(scene["campos"]) if use_sh else None, cov3D_precomp=cov)
    loss = (img * torch.as_tensor(np.asarray(dL_dpix, np.float64))).sum()
    names = ["means3D", "opacities"] + (["shs"] if use_sh else ["colors"]) + (["cov3D_precomp"] if use_cov else ["scales", "rotations"])
    leaves = dict(means3D=t["means3D"], opacities=op, colors=col, shs=sh, cov3D_precomp=cov, scales=t["scales"], rotations=t["rotations"])
    gs = torch.autograd.grad(loss, [leaves[n] for n in names] + [off], allow_unused=True)
    out = {n: (torch.zeros_like(leaves[n]) if g is None else g).detach().numpy() for n, g in zip(names, gs[:-1])}
    out["opacities"] = out["opacities"].reshape(-1, 1)
    g2 = torch.zeros_like(off) if gs[-1] is None else gs[-1]
    out["means2D"] = torch.cat([g2, torch.zeros(g2.shape[0], 1, dtype=_DT)], 1).numpy()
    return img.detach().numpy(), radii.numpy(), out
