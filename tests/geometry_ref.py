"""Plain references, input generators and comparison helpers for the geometry path in front of the rasteriser: flow -> inverse depth -> world
points (csrc/unproject.hip, unproject_common.h) and the mask compaction + pack of the per-pixel maps (csrc/pack_views.hip).  numpy only.

Two references per unprojection: `unproject_f32` restates the kernels in float32, operation for operation (the bits a correct kernel gives), and
`unproject_f64` evaluates the upstream formulas (flow2depth, depth2pc, depth != 0) in float64 and hands out, next to every value, the magnitude
sum |terms| its rounding error scales with.  The pack has one literal reference (`pack_ref`, boolean-mask gathers + concatenation) and a second,
kernel-shaped formulation (`pack_by_scan`: count, scan, rank) whose steps can be broken one at a time to show that the checks notice.

tests/test_geometry_ref.py (CPU) and tests/test_gpu_geometry_edges.py (GPU) import the same generators, the same case lists and the same
`*_fault` helpers from here: a helper returns None when everything holds and a one-line description of the first mismatch otherwise."""
import numpy as np

f32 = np.float32
U = 2.0 ** -24          # unit roundoff of float32
XYZ_ROUNDINGS = 12      # see xyz_fault
DFLOW_ROUNDINGS = 17    # see dflow_fault
EPS32 = f32(1e-8)       # the kernels' (and torch's) float32 1e-8 in z = 1 / (depth + 1e-8)
PB = 1024               # pixels per pack block
SCAN = 1024             # entries per scan chunk
MAXB = 16               # samples per launch of the host-array form

# ---- the cases both test files run --------------------------------------------------------------------------------------------------------------------
UNPROJECT_CASES = [(B, S, 100 + 10 * S + B) for S in (1, 3, 16, 17, 37) for B in (1, 3)]     # S^2 = 1, 9, 256 (one full block), 289, 1369
HOST_CASES = [(B, 5, 200 + B) for B in (16, 17, 33)]                                          # host-array form: 1, 2 and 3 launches of <= 16 samples
CHAIN_CASE = dict(B=2, S=37, V=2, seed=300)
PACK_SIZES = [(1, 1), (7, 9), (8, 8), (5, 13), (31, 33), (32, 32), (25, 41), (48, 64)]        # S2 = 1, 63, 64, 65, 1023, 1024, 1025, 3072
PACK_PATTERNS = ("all", "none", "none_in_view0", "empty_sample", "first_only", "last_only", "alternate_64", "hole_block", "random")
BIG_PACK = dict(B=6, V=2, H=325, W=325, pattern="random", seed=77, empty_samples=(3,))       # nblk = 104: 1248 scan entries, sample 5 starts at entry 1040


def pack_cases():
    """(B, V, H, W, pattern, seed): every size at V = 2 with a random mask, every view count, every pattern at 25x41 and 48x64."""
    cases = []
    for i, (H, W) in enumerate(PACK_SIZES):
        cases.append((3 if i % 2 else 1, 2, H, W, "random", 400 + i))
    for V in (1, 3, 4):
        cases.append((3, V, 31, 33, "random", 420 + V))
        cases.append((1, V, 25, 41, "random", 430 + V))
    for j, pat in enumerate(PACK_PATTERNS):
        cases.append((3, 2, 25, 41, pat, 440 + j))
        cases.append((3 if j % 2 else 1, 3 if j % 2 else 2, 48, 64, pat, 460 + j))
    return cases


# ---- unprojection: inputs -------------------------------------------------------------------------------------------------------------------------------
def _rotation(rng):
    """A rotation by 0.4 .. 1.2 rad about a random axis (Rodrigues, float64): far from symmetric, so R and R^T give different points."""
    ax = rng.standard_normal(3)
    ax /= np.linalg.norm(ax)
    th = rng.uniform(0.4, 1.2)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def unproject_inputs(B, S, seed):
    """flow [B,1,S,S], mask [B,3,S,S] (0/1; channels 1 and 2 differ from channel 0), ref_intr / intr [B,3,3], extr [B,3,4], Tf_x [B], float32, in
    which every sample differs from every other: fx != fy, cx != cy, ref cx != cx, an unsymmetric rotation, a non-zero translation and its own
    Tf_x.  About a quarter of mask channel 0 is zero.  Per sample one pixel with mask 1 has its flow set to the float32 difference ref_cx - cx
    exactly (disparity 0: inverse depth 0, invalid, and still a large gradient), and one pixel with mask 0 (a "masked" pixel in this project's
    words) carries a large flow, 6e4 (exact in fp16 too).  With S = 1 there is one pixel only: sample b takes the role b % 3 of (zero disparity,
    large masked flow, ordinary)."""
    rng = np.random.default_rng(seed)
    S2 = S * S
    flow = (rng.random((B, 1, S, S)) * 3 + 1.5).astype(f32)
    m0 = rng.random((B, S, S)) > 0.25
    mask = np.stack([m0, ~m0, rng.random((B, S, S)) > 0.5], 1).astype(f32)
    intr = np.zeros((B, 3, 3), f32)
    ref_intr = np.zeros((B, 3, 3), f32)
    extr = np.zeros((B, 3, 4), f32)
    tf = np.zeros(B, f32)
    for b in range(B):
        fx, fy = S * rng.uniform(1.0, 1.4), S * rng.uniform(1.5, 1.9)
        cx, cy = S * 0.5 + rng.uniform(0.1, 0.9), S * 0.5 - rng.uniform(0.1, 0.9)
        intr[b] = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]
        ref_intr[b] = intr[b]
        ref_intr[b, 0, 2] = cx + (0.3 + 0.05 * b) * (-1) ** b
        ref_intr[b, 1, 2] = cy + 0.21
        extr[b, :, :3] = _rotation(rng)
        extr[b, :, 3] = rng.uniform(0.3, 1.5, 3) * rng.choice([-1.0, 1.0], 3)
        tf[b] = -(5.0 + 0.61 * b + rng.uniform(0, 0.5))
    fl, mk = flow.reshape(B, S2), mask[:, 0].reshape(B, S2)       # views into flow / mask
    for b in range(B):
        zero_disp, big = (7 * b + seed) % S2, (7 * b + seed + max(1, S2 // 2)) % S2
        if S2 > 1 or b % 3 == 0:
            fl[b, zero_disp] = ref_intr[b, 0, 2] - intr[b, 0, 2]   # float32 subtraction: the kernel's `offset`, bit for bit
            mk[b, zero_disp] = 1
        if S2 > 1 or b % 3 == 1:
            fl[b, big] = 6.0e4
            mk[b, big] = 0
    mask[:, 1] = 1 - mask[:, 0]
    assert len(set(tf.tolist())) == B
    return dict(flow=flow, mask=mask, ref_intr=ref_intr, intr=intr, extr=extr, Tf_x=tf)


def unproject_grads(B, S, seed):
    """Upstream gradients: g_depth [B,1,S,S] and g_xyz [B,S*S,3], float32."""
    rng = np.random.default_rng(seed + 7919)
    return rng.standard_normal((B, 1, S, S)).astype(f32), rng.standard_normal((B, S * S, 3)).astype(f32)


def zero_disparity_pixels(inp):
    """[B, S*S] bool: mask 1 and flow == ref_cx - cx exactly."""
    B, _, S, _ = inp["flow"].shape
    off = (inp["ref_intr"][:, 0, 2] - inp["intr"][:, 0, 2]).astype(f32)
    return (inp["flow"].reshape(B, -1) == off[:, None]) & (inp["mask"][:, 0].reshape(B, -1) == 1)


# ---- unprojection: float32 restatement -------------------------------------------------------------------------------------------------------------
def _cams_f32(ref_intr, intr, extr, tf):
    """The per-sample constants as fill() / cam_from_device compute them (UnprojCam), float32."""
    Kr, K, E = (np.asarray(a, f32) for a in (ref_intr, intr, extr))
    c = dict(offset=Kr[:, 0, 2] - K[:, 0, 2], tf=np.asarray(tf, f32).reshape(-1), fx=K[:, 0, 0], fy=K[:, 1, 1], cx=K[:, 0, 2], cy=K[:, 1, 2])
    Rt = np.transpose(E[:, :3, :3], (0, 2, 1)).copy()
    c["Rt"] = Rt
    c["Rtt"] = np.stack([(Rt[:, i, 0] * E[:, 0, 3] + Rt[:, i, 1] * E[:, 1, 3]) + Rt[:, i, 2] * E[:, 2, 3] for i in range(3)], 1)
    return c


def _grid(S, swap_uv=False):
    pix = np.arange(S * S)
    v, u = pix // S, pix % S
    if swap_uv:
        u, v = v, u
    return u.astype(f32)[None], v.astype(f32)[None]


def unproject_f32(flow, mask, ref_intr, intr, extr, Tf_x, g_depth=None, g_xyz=None, backward=False, _swap_uv=False):
    """up_inverse_depth, up_world_point and k_unproject_bwd in numpy float32: every operation rounds to float32, in the kernels' order, nothing is
    contracted.  mask is [B,C,S,S]; channel 0 is the one read.  -> dict(depth [B,1,S,S], valid [B,S*S] bool, xyz [B,S*S,3]) and, with backward=True
    or a gradient given, d_flow [B,1,S,S] (g_depth [B,1,S,S] and / or g_xyz [B,S*S,3]; a missing one is the kernel's NULL)."""
    flow, mask = np.asarray(flow, f32), np.asarray(mask, f32)
    B, _, S, _ = flow.shape
    S2 = S * S
    c = _cams_f32(ref_intr, intr, extr, Tf_x)
    col = lambda k: c[k][:, None]
    m = mask[:, 0].reshape(B, S2)
    u, v = _grid(S, _swap_uv)
    half = f32(0.5)
    with np.errstate(all="ignore"):
        disparity = col("offset") - flow.reshape(B, S2)
        d = (-disparity / col("tf")) * m
        z = f32(1.0) / (d + EPS32)
        X = ((u + half) - col("cx")) * z / col("fx")
        Y = ((v + half) - col("cy")) * z / col("fy")
        Rt, Rtt = c["Rt"], c["Rtt"]
        xyz = np.stack([((Rt[:, i, 0, None] * X + Rt[:, i, 1, None] * Y) + Rt[:, i, 2, None] * z) - Rtt[:, i, None] for i in range(3)], -1)
        out = dict(depth=d.reshape(B, 1, S, S), valid=d != 0, xyz=xyz)
        if backward or g_depth is not None or g_xyz is not None:
            g = np.asarray(g_depth, f32).reshape(B, S2) if g_depth is not None else np.zeros((B, S2), f32)
            if g_xyz is not None:
                gx = np.asarray(g_xyz, f32)
                ax, ay = ((u + half) - col("cx")) / col("fx"), ((v + half) - col("cy")) / col("fy")
                dirs = [(Rt[:, i, 0, None] * ax + Rt[:, i, 1, None] * ay) + Rt[:, i, 2, None] for i in range(3)]
                g = g + (-(z * z)) * ((gx[..., 0] * dirs[0] + gx[..., 1] * dirs[1]) + gx[..., 2] * dirs[2])
            out["d_flow"] = (g * m / col("tf")).reshape(B, 1, S, S)
    assert all(a.dtype == f32 for k, a in out.items() if k != "valid")
    return out


# ---- unprojection: float64 formulas + magnitudes ----------------------------------------------------------------------------------------------------
def depth_f64(flow, mask, ref_intr, intr, Tf_x):
    """flow2depth in float64: depth = -(ref_cx - cx - flow) / Tf_x * mask[:, :1]."""
    flow, mask, Kr, K, tf = (np.asarray(a, np.float64) for a in (flow, mask, ref_intr, intr, Tf_x))
    return -((Kr[:, 0, 2] - K[:, 0, 2])[:, None, None, None] - flow) / tf[:, None, None, None] * mask[:, :1]


def unproject_f64(depth32, mask, intr, extr, Tf_x, g_depth=None, g_xyz=None, backward=False):
    """depth2pc and its gradient w.r.t. the flow in float64, from the FLOAT32 inverse depth (the kernel's own output, or unproject_f32's: the same
    function is compared, the depth's own rounding is pinned by bit equality elsewhere).  The world point is the 4x4 extrinsic inverse applied to
    the camera point; for the rigid extrinsic that inverse is [[R^T, -R^T t], [0, 1]], which is how upstream writes it (bmm(rot_t, .)), so the
    float32 R not being orthonormal to the last bit stays out of the comparison.  1e-8 is the float32 constant, as in torch's `depth + 1e-8` on a
    float32 tensor.  -> dict(xyz, xyz_mag, valid) + (d_flow, d_flow_mag):
        xyz_mag    = |R^T| |[X, Y, z]| + |R^T| |t|
        d_flow     = (g_depth - z^2 sum_i g_i sum_j Rt_ij a_j) mask / Tf_x,   a = [(u + .5 - cx) / fx, (v + .5 - cy) / fy, 1]   (dz/dd = -z^2)
        d_flow_mag = (|g_depth| + z^2 sum_i |g_i| sum_j |Rt_ij| |a_j|) |mask / Tf_x|"""
    d = np.asarray(depth32, np.float64)
    B, _, S, _ = d.shape
    S2 = S * S
    d = d.reshape(B, S2)
    K, E, tf = np.asarray(intr, np.float64), np.asarray(extr, np.float64)[:, :3, :4], np.asarray(Tf_x, np.float64).reshape(B, 1)
    u, v = _grid(S)
    u, v = u.astype(np.float64), v.astype(np.float64)
    with np.errstate(all="ignore"):
        z = 1.0 / (d + float(EPS32))
        a = np.stack([(u + 0.5 - K[:, 0, 2, None]) / K[:, 0, 0, None], (v + 0.5 - K[:, 1, 2, None]) / K[:, 1, 1, None], np.ones_like(z)], -1)   # [B,S2,3]
        cam = a * z[..., None]
        inv = np.zeros((B, 4, 4))
        inv[:, :3, :3] = np.transpose(E[:, :, :3], (0, 2, 1))
        inv[:, :3, 3] = -np.einsum("bij,bj->bi", inv[:, :3, :3], E[:, :, 3])
        inv[:, 3, 3] = 1
        xyz = np.einsum("bij,bpj->bpi", inv[:, :3, :3], cam) + inv[:, None, :3, 3]
        aRt = np.abs(inv[:, :3, :3])
        out = dict(xyz=xyz, valid=d != 0,
                   xyz_mag=np.einsum("bij,bpj->bpi", aRt, np.abs(cam)) + np.einsum("bij,bj->bi", aRt, np.abs(E[:, :, 3]))[:, None])
        if backward or g_depth is not None or g_xyz is not None:
            m = np.asarray(mask, np.float64)[:, 0].reshape(B, S2)
            gd = np.asarray(g_depth, np.float64).reshape(B, S2) if g_depth is not None else np.zeros((B, S2))
            gx = np.asarray(g_xyz, np.float64) if g_xyz is not None else np.zeros((B, S2, 3))
            dirs = np.einsum("bij,bpj->bpi", inv[:, :3, :3], a)
            adirs = np.einsum("bij,bpj->bpi", aRt, np.abs(a))
            out["d_flow"] = ((gd - z * z * (gx * dirs).sum(-1)) * m / tf).reshape(B, 1, S, S)
            out["d_flow_mag"] = ((np.abs(gd) + z * z * (np.abs(gx) * adirs).sum(-1)) * np.abs(m / tf)).reshape(B, 1, S, S)
    return out


# ---- unprojection: comparison helpers -----------------------------------------------------------------------------------------------------------------
def bits_fault(name, got, want):
    """None if both arrays hold the same bits (so -0 != +0 and a NaN equals only the same NaN), else where they first differ."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return "%s: %s %s instead of %s %s" % (name, got.dtype, got.shape, want.dtype, want.shape)
    raw = np.dtype("u%d" % got.dtype.itemsize) if got.dtype.kind == "f" else got.dtype
    bad = np.flatnonzero(got.view(raw).reshape(-1) != want.view(raw).reshape(-1))
    if bad.size:
        i = np.unravel_index(bad[0], got.shape)
        return "%s: %d of %d elements differ, first at %s: %r instead of %r" % (name, bad.size, got.size, tuple(int(k) for k in i), got[i], want[i])
    return None


def error_units(got, ref, mag):
    """max |got - ref| / (2^-24 mag) over the elements with mag > 0 (0.0 if there are none)."""
    got, ref, mag = (np.asarray(a, np.float64) for a in (got, ref, mag))
    ok = mag > 0
    return float((np.abs(got - ref)[ok] / (U * mag[ok])).max()) if ok.any() else 0.0


def _bound_fault(name, got, ref, mag, k):
    got64 = np.asarray(got, np.float64)
    if got64.shape != ref.shape:
        return "%s: shape %s instead of %s" % (name, got64.shape, ref.shape)
    if not np.isfinite(got64).all():
        return "%s: %d non-finite values" % (name, int((~np.isfinite(got64)).sum()))
    bad = np.abs(got64 - ref) > k * U * mag
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, np.abs(got64 - ref) / (U * mag + 1e-300), 0)), ref.shape)
        return "%s: %d of %d elements are off by more than %d x 2^-24 x magnitude; worst at %s: %r instead of %r, allowed error %.3e" % (
            name, int(bad.sum()), bad.size, k, tuple(int(j) for j in i), got64[i], ref[i], k * U * mag[i])
    return None


def xyz_fault(got, r64):
    """|xyz - float64| <= 12 x 2^-24 x xyz_mag per element.  The 12 counts the float32 roundings on the path, as these tests were
    specified: two for z (the add of 1e-8, the reciprocal), four for X or Y, five for the row of the 3x3 product (three products, two sums), one
    for the subtraction of R^T t.  A worst-case walk of up_world_point gives less, first order in 2^-24, relative to xyz_mag: X and Y carry z's 2 plus
    a subtraction, a product and a division (5); the first two terms of a row add a product and two sums (8), the third 2 + 1 + 1 (4); R^T t has
    three products under two sums (3, on its own share of the magnitude); the final subtraction adds 1 on the whole: 9 <= 12."""
    return _bound_fault("xyz", got, r64["xyz"], r64["xyz_mag"], XYZ_ROUNDINGS)


def dflow_fault(got, r64, mask):
    """|d_flow - float64| <= 17 x 2^-24 x d_flow_mag per element, and d_flow == 0 exactly where mask channel 0 is 0.
    The count (worst case, first order, each rounding relative to its own term and so at most to the magnitude), along k_unproject_bwd:
    z = 1 / (d + 1e-8): 2;  z * z: 2 + 2 + 1 = 5;  ax = (u + .5 - cx) / fx: 2 (u + .5 is exact);  dir_i = Rt_i0 ax + Rt_i1 ay + Rt_i2: 2 + a product
    + two sums = 5;  g_i dir_i: 6;  the sum over i: 8;  times -(z z): 8 + 5 + 1 = 14;  g_depth + that: 15;  times mask: 16;  over Tf_x: 17.
    (The g_depth share alone sees 3.)  The tests were specified with 24 for this path or, where the count comes out differently, with that
    count: 17, the tighter of the two.  Measured on the GPU: at most 4.4, equal to the float32 restatement's own error."""
    f = _bound_fault("d_flow", got, r64["d_flow"], r64["d_flow_mag"], DFLOW_ROUNDINGS)
    if f is None:
        off = np.asarray(mask)[:, :1] == 0
        if (np.asarray(got)[off] != 0).any():
            f = "d_flow: %d masked pixels carry a gradient" % int((np.asarray(got)[off] != 0).sum())
    return f


def unproject_fault(got, inp, g_depth=None, g_xyz=None, want_bits=None):
    """The whole check of one unprojection result `got` (dict with depth, valid, xyz and optionally d_flow, numpy) on the inputs `inp`:
    depth and valid bit-equal to unproject_f32; every zero-disparity pixel invalid; xyz within the xyz bound of unproject_f64 evaluated on got's own
    float32 depth; d_flow within its bound and zero where masked.  want_bits: a tuple of further keys ("xyz", "d_flow") that must also equal
    unproject_f32 bit for bit."""
    args = (inp["flow"], inp["mask"], inp["ref_intr"], inp["intr"], inp["extr"], inp["Tf_x"])
    r32 = unproject_f32(*args, g_depth=g_depth, g_xyz=g_xyz, backward="d_flow" in got)
    f = bits_fault("depth", np.asarray(got["depth"], f32), r32["depth"]) or bits_fault("valid", np.asarray(got["valid"]).astype(bool), r32["valid"])
    if f:
        return f
    if np.asarray(got["valid"]).astype(bool)[zero_disparity_pixels(inp)].any():
        return "valid: a zero-disparity pixel is marked valid"
    r64 = unproject_f64(got["depth"], inp["mask"], inp["intr"], inp["extr"], inp["Tf_x"], g_depth=g_depth, g_xyz=g_xyz, backward="d_flow" in got)
    f = xyz_fault(got["xyz"], r64)
    if f is None and "d_flow" in got:
        f = dflow_fault(got["d_flow"], r64, inp["mask"])
    for k in want_bits or ():
        f = f or bits_fault(k + " (float32 restatement)", np.asarray(got[k], f32), r32[k])
    return f


def unproject_units(got, inp, g_depth=None, g_xyz=None):
    """(xyz error, d_flow error or None) in units of 2^-24 x magnitude against unproject_f64: the figures the tests print."""
    r64 = unproject_f64(got["depth"], inp["mask"], inp["intr"], inp["extr"], inp["Tf_x"], g_depth=g_depth, g_xyz=g_xyz, backward="d_flow" in got)
    return error_units(got["xyz"], r64["xyz"], r64["xyz_mag"]), (error_units(got["d_flow"], r64["d_flow"], r64["d_flow_mag"]) if "d_flow" in got else None)


# ---- unprojection: mutants (one error each, applied to the inputs of the reference) -----------------------------------------------------------------
CHUNK_FIELDS = ("ref_intr", "intr", "extr", "Tf_x", "flow", "mask")


def chunk_mutant(inp, field):
    """The inputs a host-form launch loop sees if it forgets to advance `field` to its chunk: sample b reads that field of sample b % 16."""
    out = dict(inp)
    out[field] = inp[field][np.arange(inp[field].shape[0]) % MAXB]
    return out


def r_for_rt_mutant(inp):
    out = dict(inp)
    out["extr"] = inp["extr"].copy()
    out["extr"][:, :3, :3] = np.transpose(inp["extr"][:, :3, :3], (0, 2, 1))
    return out


def mask_channel_mutant(inp):
    out = dict(inp)
    out["mask"] = np.ascontiguousarray(inp["mask"][:, [1, 0, 2]])
    return out


def stride1_gradient_mutant(g_xyz):
    """What a kernel reads from a permuted g_xyz (memory [B,3,S2]: batch stride 3 S2, pixel stride 1, channel stride S2) if it steps the channels with
    stride 1: element (b, p, c) comes from flat offset p + c of sample b."""
    B, S2, _ = g_xyz.shape
    mem = np.ascontiguousarray(np.transpose(g_xyz, (0, 2, 1))).reshape(B, 3 * S2)
    idx = np.minimum(np.arange(S2)[:, None] + np.arange(3)[None], 3 * S2 - 1)
    return mem[:, idx]


# ---- pack: inputs -----------------------------------------------------------------------------------------------------------------------------------------
PACK_KEYS = (("xyz", 3), ("img", 3), ("rot_maps", 4), ("scale_maps", 3), ("opacity_maps", 1))
OUT_KEYS = ("xyz", "rgb", "rot", "scale", "opacity")


def _distinct(rng, n):
    """n distinct float32 in +-[0.5, 1): the 23 mantissa bits are (i + r) * odd mod 2^23, a bijection, so no two values share their bits."""
    assert n <= (1 << 23)
    mant = ((np.arange(n, dtype=np.uint64) + np.uint64(rng.integers(1 << 23))) * np.uint64(2654435761)) & np.uint64(0x7FFFFF)
    sign = rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31)
    return (mant.astype(np.uint32) | np.uint32(0x3F000000) | sign).view(f32)


def pack_inputs(B, V, H, W, pattern, seed, empty_samples=()):
    """-> (maps, valid): maps[v] = dict(xyz [B,S2,3], img [B,3,H,W], rot_maps [B,4,H,W], scale_maps [B,3,H,W], opacity_maps [B,1,H,W]) float32 and
    valid [B,V,S2] bool.  Within one kind of map all values (over all views, samples, pixels, channels) are distinct, so a swapped, repeated or missing
    row changes bits.  pattern: one of PACK_PATTERNS; empty_samples: samples whose masks are cleared on top of the pattern."""
    rng = np.random.default_rng(seed)
    S2 = H * W
    maps = [dict() for _ in range(V)]
    for key, C in PACK_KEYS:
        n = B * S2 * C
        pool = _distinct(rng, V * n)
        for v in range(V):
            maps[v][key] = pool[v * n:(v + 1) * n].reshape((B, S2, 3) if key == "xyz" else (B, C, H, W))
    pix = np.arange(S2)
    valid = np.zeros((B, V, S2), bool)
    if pattern == "all":
        valid[:] = True
    elif pattern == "none":
        pass
    elif pattern in ("random", "none_in_view0", "empty_sample"):
        dens = rng.uniform(0.2, 0.8, (B, V, 1))
        valid = rng.random((B, V, S2)) < dens
        if pattern == "none_in_view0":
            valid[:, 0] = False
        if pattern == "empty_sample":
            valid[min(1, B - 1)] = False
    elif pattern == "first_only":
        valid[:, :, 0] = True
    elif pattern == "last_only":
        valid[:, :, -1] = True
    elif pattern == "alternate_64":
        valid[:] = (pix // 64) % 2 == 0
    elif pattern == "hole_block":
        hole = ((S2 + PB - 1) // PB - 1) // 2
        valid[:] = pix // PB != hole
    else:
        raise ValueError(pattern)
    for b in empty_samples:
        valid[b] = False
    return maps, valid


def pack_row_grads(total, seed):
    """Gradients of the packed rows: dict over OUT_KEYS of float32 [total, C], all values distinct within a kind."""
    rng = np.random.default_rng(seed + 104729)
    return {k: _distinct(rng, max(1, total * C))[:total * C].reshape(total, C) for k, C in zip(OUT_KEYS, (3, 3, 4, 3, 1))}


# ---- pack: references -----------------------------------------------------------------------------------------------------------------------------------
def _rows_of_view(m, b):
    """The five [S2, C] row sources of sample b of one view, in pixel order; rgb = float32(float32(img 0.5) + 0.5)."""
    planar = lambda a: a[b].reshape(a.shape[1], -1).T
    img = planar(m["img"])
    return (m["xyz"][b], (img * f32(0.5)) + f32(0.5), planar(m["rot_maps"]), planar(m["scale_maps"]), planar(m["opacity_maps"]))


def pack_ref(maps, valid, _view_order=None):
    """The literal per-sample, per-view boolean-mask gathers followed by the concatenation (upstream's pts2render).
    -> dict(xyz, rgb, rot, scale, opacity: float32 [total, C]; offsets int64 [B+1]; row_of_pixel int32 [B,V,S2], -1 where invalid)."""
    B, V, S2 = valid.shape
    order = list(range(V)) if _view_order is None else list(_view_order)
    parts = [[] for _ in OUT_KEYS]
    offsets = [0]
    rop = np.full((B, V, S2), -1, np.int32)
    for b in range(B):
        n = offsets[-1]
        for v in order:
            ok = valid[b, v]
            rop[b, v][ok] = n + np.arange(int(ok.sum()))
            n += int(ok.sum())
            for lst, src in zip(parts, _rows_of_view(maps[v], b)):
                lst.append(src[ok])
        offsets.append(n)
    out = {k: np.concatenate(p, 0).astype(f32) for k, p in zip(OUT_KEYS, parts)}
    out["offsets"] = np.asarray(offsets, np.int64)
    out["row_of_pixel"] = rop
    return out


def pack_by_scan(maps, valid, drop_carry=False, inclusive_rank=False, skip_empty_offset=False):
    """The same result the way the kernels get it: valid pixels per 1024-pixel block, an exclusive scan over the (sample, view, block) entries in
    chunks of 1024 with a carry, row = block offset + rank inside the block; sample offsets are the scan values at each sample's first entry.
    The keywords break one step each: the carry is dropped at every chunk boundary; the rank counts the lane itself (off by one lane); the list of sample offsets is not advanced
    past an empty sample (the sample gets no entry of its own, so it appears to own the next sample's rows)."""
    B, V, S2 = valid.shape
    nblk = (S2 + PB - 1) // PB
    padded = np.zeros((B, V, nblk * PB), bool)
    padded[..., :S2] = valid
    counts = padded.reshape(B * V * nblk, PB).sum(1)
    ex = np.zeros(len(counts) + 1, np.int64)
    carry = 0
    for base in range(0, len(counts), SCAN):
        c = counts[base:base + SCAN]
        start = 0 if (drop_carry and base > 0) else carry
        ex[base:base + len(c)] = start + np.cumsum(c) - c
        carry = start + int(c.sum())
    ex[-1] = carry
    offsets = ex[np.arange(B + 1) * V * nblk].copy()
    if skip_empty_offset:
        kept = [0] + [int(offsets[b + 1]) for b in range(B) if valid[b].any()]
        offsets = np.asarray(kept + [kept[-1]] * (B + 1 - len(kept)), np.int64)
    rank = np.cumsum(padded.reshape(-1, PB), 1) - (0 if inclusive_rank else padded.reshape(-1, PB))
    rows = (ex[:-1, None] + rank).reshape(B, V, nblk * PB)[..., :S2]
    rop = np.where(valid, rows, -1).astype(np.int32)
    total = int(ex[-1])
    out = {k: np.zeros((max(total, int(rows[valid].max(initial=-1)) + 1), C), f32) for k, C in zip(OUT_KEYS, (3, 3, 4, 3, 1))}
    for b in range(B):
        for v in range(V):
            ok = valid[b, v]
            for k, src in zip(OUT_KEYS, _rows_of_view(maps[v], b)):
                out[k][rows[b, v][ok]] = src[ok]
    for k in OUT_KEYS:
        out[k] = out[k][:total]
    out["offsets"] = offsets
    out["row_of_pixel"] = rop
    return out


def pack_bwd_ref(row_of_pixel, g, hw, halve_img=True):
    """Scatters the row gradients g (dict over OUT_KEYS, or None for a missing one) back to the pixels: per view dict(xyz [B,S2,3], img [B,3,H,W],
    rot_maps [B,4,H,W], scale_maps [B,3,H,W], opacity_maps [B,1,H,W]) float32, zero where the pixel is invalid; the img gradient is float32(g 0.5)."""
    B, V, S2 = row_of_pixel.shape
    H, W = hw
    res = []
    for v in range(V):
        rows = row_of_pixel[:, v]
        ok = rows >= 0
        d = {}
        for (key, C), ok_key in zip(PACK_KEYS, OUT_KEYS):
            full = np.zeros((B, S2, C), f32)
            if g.get(ok_key) is not None:
                vals = np.asarray(g[ok_key], f32)[rows[ok]]
                full[ok] = vals * f32(0.5) if (key == "img" and halve_img) else vals
            d[key] = full if key == "xyz" else np.ascontiguousarray(np.transpose(full, (0, 2, 1))).reshape(B, C, H, W)
        res.append(d)
    return res


def pack_features_ref(feats, row_of_pixel):
    """feats[v] [B,F,H,W] -> [B V S2, F]: row r holds the F values of the pixel packed to row r; rows without a pixel are zero."""
    B, V, S2 = row_of_pixel.shape
    F = feats[0].shape[1]
    out = np.zeros((B * V * S2, F), f32)
    for v in range(V):
        src = np.transpose(np.asarray(feats[v], f32).reshape(B, F, S2), (0, 2, 1))
        ok = row_of_pixel[:, v] >= 0
        out[row_of_pixel[:, v][ok]] = src[ok]
    return out


def unpack_rows_ref(values, row_of_pixel):
    return np.where(row_of_pixel >= 0, np.asarray(values)[np.maximum(row_of_pixel, 0)], 0).astype(np.asarray(values).dtype)


# ---- pack: comparison helpers ----------------------------------------------------------------------------------------------------------------------------
def pack_fault(got, ref):
    """got / ref: dicts as pack_ref returns them (got's packed arrays may be longer: only the first offsets[-1] rows are defined and looked at).
    offsets, row_of_pixel and the five packed arrays, all bit-equal."""
    f = bits_fault("offsets", np.asarray(got["offsets"], np.int64), np.asarray(ref["offsets"], np.int64))
    f = f or bits_fault("row_of_pixel", np.asarray(got["row_of_pixel"], np.int32), ref["row_of_pixel"])
    total = int(ref["offsets"][-1])
    for k in OUT_KEYS:
        f = f or bits_fault("packed " + k, np.asarray(got[k], f32)[:total], ref[k])
    return f


def pack_bwd_fault(got, ref, keys=None):
    """got / ref: per view dicts of map gradients (pack_bwd_ref's layout); bit-equal on `keys` (default: every key of ref)."""
    for v, (gv, rv) in enumerate(zip(got, ref)):
        for k in (keys or rv.keys()):
            f = bits_fault("view %d d_%s" % (v, k), np.asarray(gv[k], f32), rv[k])
            if f:
                return f
    return None
