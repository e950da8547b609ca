"""The fused Gaussian-head op (csrc/gshead.hip, gshead.head) restated in NumPy fp64, the per-element error bounds an fp32 implementation of it has
to meet, and the inputs test_gpu_gshead.py runs -- shared with test_gshead_ref.py, which checks on the CPU that the bounds are reachable and that
single-error mutants leave them.  No torch, no library.

    r = max(h, 0)      z[n,k,p] = b[k] + sum_c w[k,c] r[n,c,p]      y = act(z)
    dz = dy act'(z)    dh[n,c,p] = (h > 0) sum_k w[k,c] dz[n,k,p]   dw[k,c] = sum_{n,p} dz[n,k,p] r[n,c,p]    db[k] = sum_{n,p} dz[n,k,p]
    act: none | softplus(beta, threshold) = z where beta z > threshold, else log1p(exp(beta z)) / beta | sigmoid

Bounds.  u = 2^-24, g(n) = n u / (1 - n u); |.| elementwise; they hold for any summation order and with or without FMA contraction.
    z     Dz  = g(C + 1) (sum_c |w| r + |b|)                                   C products, C additions
    y     L Dz + E_ACT u |y|                  L = 1 (none, softplus: |act'| <= 1), 1/4 (sigmoid)
    act'  Dg  = Lg (Dz + u |z|) + E_SLOPE u s (+ exp(-threshold), softplus)    Lg = sup |act''| = beta / 4 (softplus), 1 / (6 sqrt 3) (sigmoid);
                                                                                u |z|: the rounding of beta z;  s = sigmoid(beta z) | sigmoid(z):
                                                                                both slopes are formed from the kernel's sigmoid, s | s (1 - s);
                                                                                exp(-threshold): the step of softplus' slope at the threshold
    dz    Ddz = |dy| Dg + u |dz|              (none: 0 -- dz IS dy)
    dh    (h > 0) (sum_k |w| Ddz + g(K) sum_k |w| |dz|)
    dw    (1 + g(P)) sum_{n,p} Ddz r + g(P) sum_{n,p} |dz| r                   P = N H W summed pixels
    db    sum_{n,p} Ddz + g(P) sum_{n,p} |dz|

E_ACT, in units of u |y| (one ulp of y is between u |y| and 2 u |y|).  No document on the build machine states ulp bounds for the device's expf /
log1pf, so, as the issue prescribes, the error of ATen's OWN elementwise torch.sigmoid and F.softplus(beta=100) on the GPU was measured against fp64
on the same fp32 z (2^22 points, half uniform over beta z in [-30, 30], half normal with deviation 3; results that are normal fp32 numbers; no
convolution and nothing of this package runs -- tools/bench_gshead.py act_error(), recorded in profiles/gshead_shapes.md):
    sigmoid   worst 2.737 u |y|        softplus(beta = 100)   worst 17.915 u |y|
(softplus' figure is the rounding of beta z in front of the exponential: y ~ exp(beta z) / beta for beta z << 0, so a relative u on beta z is a
relative |beta z| u on y; it grows with the range measured and only matters where y is tiny.)  Twice the measured error is allowed, with a floor of
one ulp (2 u |y|): E_ACT = 5.5 (sigmoid), 35.9 (softplus).  E_SLOPE = E_ACT[sigmoid] + 2: the kernel's sigmoid, one subtraction and one product.
"""
import zlib

import numpy as np

U = 2.0 ** -24
E_ACT = {"none": 0.0, "softplus": 35.9, "sigmoid": 5.5}
E_SLOPE = E_ACT["sigmoid"] + 2.0
KEYS = ("y", "dh", "dw", "db")


def gamma(n):
    return n * U / (1.0 - n * U)


def _sigmoid(t):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-t))


def act_value(z, act, beta=1.0, threshold=20.0):
    if act == "none":
        return z
    if act == "sigmoid":
        return _sigmoid(z)
    with np.errstate(over="ignore"):
        return np.where(beta * z > threshold, z, np.log1p(np.exp(np.minimum(beta * z, 700.0))) / beta)


def act_slope(z, act, beta=1.0, threshold=20.0):
    if act == "none":
        return np.ones_like(z)
    if act == "sigmoid":
        s = _sigmoid(z)
        return s * (1.0 - s)
    return np.where(beta * z > threshold, 1.0, _sigmoid(beta * z))


def reference(h, w, b, dy, act="none", beta=1.0, threshold=20.0):
    """fp64 forward and backward from the given (fp32) values: dict of z, y, dz, dh [N,C,H,W], dw [K,C], db [K]."""
    h, w, b, dy = (np.asarray(t, dtype=np.float64) for t in (h, w, b, dy))
    r = np.maximum(h, 0.0)
    z = np.einsum("kc,nchw->nkhw", w, r) + b[None, :, None, None]
    dz = dy * act_slope(z, act, beta, threshold)
    return dict(z=z, y=act_value(z, act, beta, threshold), dz=dz, dh=(h > 0) * np.einsum("kc,nkhw->nchw", w, dz),
                dw=np.einsum("nkhw,nchw->kc", dz, r), db=dz.sum(axis=(0, 2, 3)))


def bounds(h, w, b, dy, act="none", beta=1.0, threshold=20.0):
    """Per-element bounds on |fp32 result - reference()| for y, dh, dw, db (and z, dz), as derived at the top of this file."""
    ref = reference(h, w, b, dy, act, beta, threshold)
    h, w, b, dy = (np.asarray(t, dtype=np.float64) for t in (h, w, b, dy))
    N, C, H, W = h.shape
    K, P = w.shape[0], N * H * W
    r, aw = np.maximum(h, 0.0), np.abs(w)
    Dz = gamma(C + 1) * (np.einsum("kc,nchw->nkhw", aw, r) + np.abs(b)[None, :, None, None])
    z, y, dz = ref["z"], ref["y"], ref["dz"]
    if act == "none":
        By, Ddz = Dz, np.zeros_like(Dz)
    else:
        L, Lg = (1.0, beta / 4.0) if act == "softplus" else (0.25, 1.0 / (6.0 * np.sqrt(3.0)))
        By = L * Dz + E_ACT[act] * U * np.abs(y)
        s = _sigmoid(beta * z) if act == "softplus" else _sigmoid(z)
        Dg = Lg * (Dz + U * np.abs(z)) + E_SLOPE * U * s + (np.exp(-threshold) if act == "softplus" else 0.0)
        Ddz = np.abs(dy) * Dg + U * np.abs(dz)
    return dict(z=Dz, y=By, dz=Ddz,
                dh=(h > 0) * (np.einsum("kc,nkhw->nchw", aw, Ddz) + gamma(K) * np.einsum("kc,nkhw->nchw", aw, np.abs(dz))),
                dw=(1.0 + gamma(P)) * np.einsum("nkhw,nchw->kc", Ddz, r) + gamma(P) * np.einsum("nkhw,nchw->kc", np.abs(dz), r),
                db=Ddz.sum(axis=(0, 2, 3)) + gamma(P) * np.abs(dz).sum(axis=(0, 2, 3)))


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; an error of zero is inside any bound (also a bound of zero), an error above a zero bound (or a NaN) is infinite."""
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d == 0, 0.0, d / bound)
    q = np.where(np.isnan(q), np.inf, q)
    return float(q.max())


# ---- the inputs of the GPU test ------------------------------------------------------------------------------------------------------------------
def cases(T):
    """name -> (N, C, H, W, K, act, beta, threshold) for a tile of T pixels (gsr_head_tile()).  Every shape the issue names, every K, every
    activation on both addressing paths (H W a multiple of 4 or not), both pixel widths (C <= 32, C = 64 with its two passes over a tile, the second
    one partly and wholly outside the plane) and both depths of the partial sum (at most / more than 64 workgroups)."""
    sp, sg, no = ("softplus", 100.0, 20.0), ("sigmoid", 1.0, 20.0), ("none", 1.0, 20.0)
    return {
        "tiny_2x32x5x7_k3_softplus": (2, 32, 5, 7, 3) + sp,          # smaller than one workgroup, odd H W, misaligned planes
        "tiny_2x32x5x7_k4_none": (2, 32, 5, 7, 4) + no,
        "T-1_k1_sigmoid": (1, 32, 1, T - 1, 1) + sg,
        "T_k4_none": (1, 32, 1, T, 4) + no,
        "T_k3_softplus": (1, 32, 1, T, 3) + sp,
        "T+1_k2_sigmoid": (1, 32, 1, T + 1, 2) + sg,
        "c16_3x16x9x257_k3_softplus": (3, 16, 9, 257, 3) + sp,
        "c16_2x16x6x10_k1_none": (2, 16, 6, 10, 1) + no,
        "c64_2x64x17x64_k4_sigmoid": (2, 64, 17, 64, 4) + sg,
        "c64_1x64x3x233_k2_softplus": (1, 64, 3, 233, 2) + sp,       # C = 64 off the vector path; its second pass ends inside the plane
        "c64_1x64x1x300_k3_none": (1, 64, 1, 300, 3) + no,           # C = 64: the whole second pass lies outside the plane
        "multi_5T+3_k4_softplus": (1, 32, 1, 5 * T + 3, 4) + sp,     # six partials, the last one of three pixels
        "multi_5T+4_k4_sigmoid": (1, 32, 1, 5 * T + 4, 4) + sg,      # the same on the vector path
        "parts_65_k2_none": (65, 16, 2, 4, 2) + no,                  # 65 workgroups: the partial sums take two stages
    }


def _plant(h, w, b, n, p, target):
    """Make pixel p of sample n (h viewed [N, C, P]) give z_0 = target: non-negative activations along the part of w[0] that has the needed sign."""
    need = float(target) - float(b[0])
    part = np.maximum(w[0], 0.0) if need >= 0 else np.minimum(w[0], 0.0)
    h[n, :, p] = (part * (need / float((part * w[0]).sum()))).astype(np.float32)


def make_case(name, T):
    """The inputs of one case, a pure function of its name: dict(h, w, b, dy (fp32 arrays), act, beta, threshold, planted).

    h is standard normal (about half the entries negative) with 3 % of the entries exactly 0, one pixel all negative (z = b there) and, where the
    activation has them, pixels planted so that z_0 hits its edges: sigmoid at +-90; softplus with beta z just below and just above the threshold
    (0.1 % and 0.001 % either side) and at beta z = -200.  `planted` lists (what, n, p) of those pixels."""
    N, C, H, W, K, act, beta, threshold = cases(T)[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    P = H * W
    h = rng.standard_normal((N, C, P)).astype(np.float32)
    w = (rng.standard_normal((K, C)) * 0.3).astype(np.float32)
    b = rng.standard_normal((K,)).astype(np.float32)
    dy = rng.standard_normal((N, K, H, W)).astype(np.float32)
    h[rng.random(h.shape) < 0.03] = 0.0
    spots = rng.permutation(P)[:8]                    # distinct pixels of the last sample (P >= 8 in every case)
    n = N - 1
    h[n, :, spots[0]] = -np.abs(h[n, :, spots[0]]) - 0.125
    planted = [("all_negative", n, int(spots[0]))]
    if act == "sigmoid":
        targets = [("z=+90", 90.0), ("z=-90", -90.0)]
    elif act == "softplus":
        t = threshold / beta
        targets = [("below_1e-3", t * (1 - 1e-3)), ("above_1e-3", t * (1 + 1e-3)), ("below_1e-5", t * (1 - 1e-5)), ("above_1e-5", t * (1 + 1e-5)),
                   ("beta_z=-200", -200.0 / beta)]
    else:
        targets = []
    for (what, target), p in zip(targets, spots[1:]):
        _plant(h, w, b, n, int(p), target)
        planted.append((what, n, int(p)))
    return dict(h=h.reshape(N, C, H, W), w=w, b=b, dy=dy, act=act, beta=beta, threshold=threshold, planted=planted)
