"""Shared references for the edge tests of the 1-D correlation sampler (k_cs_fwd, k_cs_bwd, k_cs_bwd4) and the fused multi-level lookup
(k_lookup_fwd, k_lookup_bwd), both in csrc/corr_sampler.hip.  TEST INFRASTRUCTURE ONLY: everything here runs on the CPU.

  * hat_lookup: the lookup written as a sum over the whole row with the hat weight max(0, 1 - |c / 2^l - r + k - j|), in fp64 torch.  There is no
    floor, no fractional part and no tap index in it, and its backward is torch autograd: it owes nothing to the kernels' arithmetic, to the C twin
    (oracle/aux_oracle.c, cs_oracle_*) or to oracle/corr_oracle.py, which all share `floorf` / `dx` / the tap index.
  * the error bound of the fp32 arithmetic against it, derived (bound()): the kernels and the twin form a * (1 - dx) + b * dx without contraction --
    one rounding in 1 - dx, two products, one sum, and for x in (-2^-25, 0) dx = x - floor(x) itself rounds (to 1) -- so
        |fp32 result - fp64 hat| <= 4 * 2^-24 * S,     S = the sum of |tap| over the taps with |c / 2^l - r + k - j| <= 1.
    The comparison is inclusive (<=) and so is the support: the fp64 hat loses an offset of 1e-30 next to an integer.
  * special_coords: the coordinates at which such kernels go wrong.  COORDINATE RANGE: finite, no subnormals, |c| + r + 1 < 2^31.  Beyond that
    range `(int)floorf(c)` is undefined (in the twin and in the extension the kernels replace as well); the kernels' bounds tests keep every access
    inside the tensors for any input, but the values there are unspecified and no test looks at them.
  * the C twin as torch in / torch out (per level for the lookup: the level-l coordinate is coords * float32(0.5 ** l), which is exact);
  * the shape tables of the test files, value / bit-pattern comparisons, and report().
"""
import ctypes as C
import functools
import json
import os
import zlib

import numpy as np
import torch

U = 2.0 ** -24                                    # the unit roundoff of fp32
BOUND_FACTOR = 4.0                                # roundings per result, see above

# sampler: W2 below, at and above one quad of k_cs_bwd4 (4, 8, 12, 16, 64 take it; the others k_cs_bwd); radii 0, 1 and wider than the row
SAMPLER_W2 = [1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 64]
SAMPLER_R = [0, 1, 2, 4, 7]
# fused lookup: odd widths (W2 >> l floors, the dropped column stays unwritten) and W2 < 2^l (levels of width 0, NULL pointers)
LOOKUP_LEVELS = [1, 2, 3, 4]
LOOKUP_W2 = [1, 2, 3, 5, 7, 8, 9, 15, 16, 17]
LOOKUP_R = [0, 1, 4]
ORACLE_W2 = [1, 3, 7, 8, 9, 15, 17]
# block tails: N*H1*W1 either side of one and two blocks of 256; W2 = 4: the quad count of k_cs_bwd4 equals those totals
TAIL_NHW = [(1, 1, 255), (1, 1, 256), (1, 1, 257), (1, 3, 171)]
TAIL_W2 = [4, 1, 7]
# zero fill and bounds through the C-ABI
FILL_W2 = [4, 5, 9, 12, 17]
FILL_NHW, FILL_LEVELS, FILL_R, FILL_GUARD = (2, 3, 5), 4, 4, 64


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def report(rec):
    """One JSON line per case family and quantity: printed, and appended to corr_lookup_parity.jsonl where GPSGS_PARITY_DIR names a directory."""
    line = json.dumps(rec)
    print(line)
    out = os.environ.get("GPSGS_PARITY_DIR")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "corr_lookup_parity.jsonl"), "a") as f:
            f.write(line + "\n")
    return rec


# ---- comparisons ------------------------------------------------------------------------------------------------------------
def bits(t):
    """The bit pattern of an fp32 / fp16 tensor (so that +0 and -0, or two NaNs, are told apart)."""
    t = t.detach().contiguous().cpu()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def same_values(a, b):
    """Equal element by element as numbers, no NaN: the comparison against the twin, which accumulates from +0 and so may differ in a zero's sign."""
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.dtype == b.dtype and a.shape == b.shape and not bool(torch.isnan(a).any()) and torch.equal(a, b)


# ---- coordinates ------------------------------------------------------------------------------------------------------------
FAR = [-0.0, -1e-9, 1e-9, -1e-30, 1e6 + 0.25, -1e6 - 0.25, 2.0 ** 24, -2.0 ** 24, 1e9, -1e9]
TINY = np.finfo(np.float32).tiny


def special_coords(W2, r, seed=0):
    """fp32 [len]: every integer of [-r-2, W2+r+2]; each moved one fp32 ulp down and up; each plus 0.5; FAR; 64 uniform draws of [-r-3, W2+r+3].
    Finite, |c| + r + 1 < 2^31, and no subnormals: one ulp either side of 0 is subnormal, the smallest normal of that sign stands in."""
    ints = np.arange(-r - 2, W2 + r + 3, dtype=np.float32)
    rng = np.random.default_rng(_seed("coords", W2, r, seed))
    c = np.concatenate([ints, np.nextafter(ints, np.float32(-np.inf)), np.nextafter(ints, np.float32(np.inf)), ints + np.float32(0.5),
                        np.array(FAR, np.float32), rng.uniform(-r - 3, W2 + r + 3, 64).astype(np.float32)]).astype(np.float32)
    sub = (c != 0) & (np.abs(c) < TINY)
    c[sub] = np.copysign(TINY, c[sub])
    assert np.isfinite(c).all() and not ((c != 0) & (np.abs(c) < TINY)).any() and (np.abs(c.astype(np.float64)) + r + 1 < 2.0 ** 31).all()
    return torch.from_numpy(c)


def coords_grid(W2, r, N, H1, seed=0):
    """special_coords laid over [N,1,H1,W1] with W1 = ceil(len / (N H1)), padded with uniform draws of [-r-3, W2+r+3]."""
    c = special_coords(W2, r, seed).numpy()
    W1 = -(-c.size // (N * H1))
    pad = np.random.default_rng(_seed("pad", W2, r, seed)).uniform(-r - 3, W2 + r + 3, N * H1 * W1 - c.size).astype(np.float32)
    return torch.from_numpy(np.concatenate([c, pad]).reshape(N, 1, H1, W1))


def eighths(shape, lo, hi, seed):
    """Uniform multiples of 1/8 in [lo, hi] (fp32): dx and 1 - dx are exact, and so is the level-l coordinate's fractional part down to 1/64."""
    rng = np.random.default_rng(_seed("eighths", shape, lo, hi, seed))
    return torch.from_numpy((rng.integers(int(lo) * 8, int(hi) * 8 + 1, shape) / 8.0).astype(np.float32))


def randn(shape, seed, half=False):
    """Standard normal fp32 (CPU), rounded to fp16-representable values on request."""
    t = torch.from_numpy(np.random.default_rng(_seed("randn", tuple(shape), seed)).standard_normal(shape).astype(np.float32))
    return t.half().float() if half else t


def widths(W2, levels):
    return [W2 >> l for l in range(levels)]


# ---- the hat function -------------------------------------------------------------------------------------------------------
def _c3(coords):
    c = torch.as_tensor(coords).detach().double()
    return c[:, 0] if c.dim() == 4 else c


def hat_weights(coords, r, wl, l=0):
    """-> (hat, support), both [N,H,W1,2r+1,wl] fp64: max(0, 1 - |d|) and (|d| <= 1) for d = c / 2^l - r + k - j."""
    c = _c3(coords)
    k = torch.arange(2 * r + 1, dtype=torch.float64)
    j = torch.arange(wl, dtype=torch.float64)
    d = ((c[..., None] / 2.0 ** l - r + k)[..., None] - j).abs()
    return (1.0 - d).clamp_min(0.0), (d <= 1.0).double()


def hat_lookup(pyr, coords, r):
    """pyr[l][N,H,W1,W2>>l], coords [N,1,H,W1] (or [N,H,W1]) -> [N, L*(2r+1), H, W1] fp64:
    out[n, l*(2r+1)+k, y, x] = sum_j V_l[n,y,x,j] * max(0, 1 - |c / 2^l - r + k - j|).  Differentiable in the volumes."""
    outs = []
    for l, V in enumerate(pyr):
        V = V if V.dtype == torch.float64 else V.detach().double()
        hat, _ = hat_weights(coords, r, V.shape[-1], l)
        outs.append((hat * V[..., None, :]).sum(-1).permute(0, 3, 1, 2))
    return torch.cat(outs, 1)


def hat_magnitude(pyr, coords, r):
    """S of the forward bound: the sum of |tap| over the hat's closed support, [N, L*(2r+1), H, W1] fp64."""
    outs = []
    for l, V in enumerate(pyr):
        _, sup = hat_weights(coords, r, V.shape[-1], l)
        outs.append((sup * V.detach().double().abs()[..., None, :]).sum(-1).permute(0, 3, 1, 2))
    return torch.cat(outs, 1)


def hat_backward(wl_list, coords, gout, r):
    """-> (grads, S): per level the gradient [N,H,W1,wl] of sum(hat_lookup * gout) by torch autograd, and the backward bound's S (the sum of
    |grad_out tap| over the closed support), both fp64."""
    c = _c3(coords)
    N, H, W1 = c.shape
    pyr = [torch.zeros(N, H, W1, wl, dtype=torch.float64, requires_grad=True) for wl in wl_list]
    g = torch.as_tensor(gout).detach().double()
    (hat_lookup(pyr, coords, r) * g).sum().backward()
    rd = 2 * r + 1
    mags = []
    for l, wl in enumerate(wl_list):
        _, sup = hat_weights(coords, r, wl, l)
        mags.append((sup * g[:, l * rd:(l + 1) * rd].abs().permute(0, 2, 3, 1)[..., None]).sum(-2))
    return [p.grad for p in pyr], mags


def bound_ratio(got, ref, mag):
    """max |got - ref| / (4 * 2^-24 * S), elementwise; an element with S = 0 must be exact (inf otherwise).  0 for empty tensors."""
    got = torch.as_tensor(got).detach().double().cpu()
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    b = BOUND_FACTOR * U * mag
    ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    assert not bool(torch.isnan(got).any())
    return float(ratio.max())


# ---- the C twin -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _aux():
    from oracle import gsr_oracle
    gsr_oracle.build()
    return C.CDLL(os.path.join(os.path.dirname(gsr_oracle.__file__), "_build", "libaux_oracle.so"))


def _np32(t):
    return np.ascontiguousarray(torch.as_tensor(t).detach().cpu().float().numpy(), dtype=np.float32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def twin_forward(vol, coords, r):
    """cs_oracle_forward: vol [N,H1,W1,W2], coords [N,1,H1,W1] or [N,H1,W1] -> fp32 [N,2r+1,H1,W1] (fp32 arithmetic whatever the inputs' dtype)."""
    v, c = _np32(vol), _np32(coords)
    N, H1, W1, W2 = v.shape
    out = np.zeros((N, 2 * r + 1, H1, W1), np.float32)
    if out.size and W2:
        _aux().cs_oracle_forward(_p(v), _p(c), _p(out), N, H1, W1, W2, r)
    return torch.from_numpy(out)


def twin_backward(coords, gout, W2, r):
    """cs_oracle_backward: -> fp32 [N,H1,W1,W2]."""
    c, g = _np32(coords), _np32(gout)
    N, _, H1, W1 = g.shape
    gv = np.zeros((N, H1, W1, W2), np.float32)
    if gv.size:
        _aux().cs_oracle_backward(_p(c), _p(g), _p(gv), N, H1, W1, W2, r)
    return torch.from_numpy(gv)


def level_coords(coords, l):
    """coords / 2^l as the kernels form it: one fp32 product with a power of two (exact)."""
    c = torch.as_tensor(coords).detach().cpu().float()
    return c * np.float32(0.5 ** l)


def twin_lookup(pyr, coords, r):
    """The twin once per level, concatenated: channel l*(2r+1)+k = tap k of level l."""
    return torch.cat([twin_forward(v, level_coords(coords, l), r) for l, v in enumerate(pyr)], 1)


def twin_lookup_backward(wl_list, coords, gout, r):
    rd = 2 * r + 1
    g = torch.as_tensor(gout).detach().cpu().float()
    return [twin_backward(level_coords(coords, l), g[:, l * rd:(l + 1) * rd], wl, r) for l, wl in enumerate(wl_list)]


def shift_volume(V, s):
    """V moved by s columns along the last axis with zero fill: out[..., j + s] = V[..., j]."""
    out = torch.zeros_like(V)
    w = V.shape[-1]
    if abs(s) >= w:
        return out
    if s >= 0:
        out[..., s:] = V[..., :w - s]
    else:
        out[..., :w + s] = V[..., -s:]
    return out
