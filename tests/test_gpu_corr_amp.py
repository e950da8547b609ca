"""GPU (-m gpu): the fp16 (AMP) path of the correlation pyramid -- volume, pooled levels, backward, fused lookup -- against fp64
and against the reference's own fp16 arithmetic.

Stage 2 trains with mixed precision: the feature maps reach CorrBlockFast1D as fp16, so every step runs k_cv_fwd<__half>,
k_cv_bwd<__half, *>, k_lookup_fwd<__half> and k_lookup_bwd<__half>.  The inputs here are fp16 values, so an fp64 computation on
them is the exact answer to the question the kernel is asked, and every bound below is an error analysis of the kernel's
arithmetic:
  * fp32 MFMA chain (k-ordered fmaf, one rounding per step), the backward's fold of up to four gradient levels (three fp32
    additions) and the fp32 scale multiply, u = 2^-24.  Results stored as fp16: 4 u sum|terms| -- the fp16 half-ulp is 2^13
    times the fp32 one and absorbs the chain.  Results stored as fp32 have nothing to absorb it, and a K-term recursive sum
    grows like sqrt(K) (the probabilistic bound of Higham & Mary, SIAM J. Sci. Comput. 41(5), 2019, with lambda = 2):
    (3 + 2 sqrt(K)) u sum|terms|, K = the GEMM's reduction length (D forward, W2 for d fmap1, W1 for d fmap2).  Measured on
    the MI355X beyond the store's half-ulp: at most 6.1 u sum|terms| at K = 96 and 7.0 u at K = 128 (training shape, fp32),
    against 22.6 u and 25.6 u allowed;
  * the single rounding to the storage type on store: 0.5 ulp, taken at max(|exact|, |result|) -- where the rounding carries
    a value across a power of two the spacing above it is the one that applies (round-to-nearest of an fp32 value y never
    lands below y's binade, and |result - y| <= 0.5 ulp(y) <= 0.5 ulp(result)).
The pooled levels are not bounded but pinned: the reference pools in fp16 with avg_pool2d, which sums in fp32 and rounds once."""
import json
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24  # unit roundoff of the fp32 arithmetic inside the kernels
FP16_MAX_FINITE_RN = 65520.0  # round-to-nearest(x) to fp16 is inf exactly from here (65504 + half its spacing of 32)

# (N, D, H, W1, W2): the training shape (batch 2 -> fmap12 N = 4, encoder_dims[2] = 96, 128^2 features), W2 % 8 = 4, odd widths,
# D from one MFMA K-step to three backward M-tiles (the backward tiles D by 64 * BWD_MT = 192)
SHAPES = {
    "train": (4, 96, 128, 128, 128),
    "w132": (2, 96, 3, 64, 132),
    "w33-d37": (1, 37, 3, 70, 33),
    "w257-d8": (1, 8, 2, 40, 257),
    "d193": (2, 193, 2, 66, 128),
    "d256-w132": (2, 256, 2, 96, 132),
    "d400": (1, 400, 2, 64, 96),
}


def _dt(name):
    import torch
    return getattr(torch, name)


def _randn(shape, seed, scale=1.0, dtype="float16"):
    """Normal values rounded to `dtype` (generated on the GPU: the training shape is too big for a numpy round trip per test)."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, device="cuda", generator=g, dtype=torch.float32) * scale).to(_dt(dtype))


def _ulp(x, dtype):
    """Spacing of `dtype` (fp16 / fp32) at |x| for an fp64 tensor x, subnormal range included."""
    import torch
    p, emin = (11, -24) if dtype is torch.float16 else (24, -149)
    _, e = torch.frexp(x.abs())
    e = torch.where(x == 0, torch.full_like(e, emin), (e - p).clamp(min=emin))
    return torch.ldexp(torch.ones_like(x), e)


def _assert_rounded(k, exact, S, K, what, mask=None):
    """|k - exact| <= 0.5 ulp(max(|exact|, |k|)) + c u S elementwise (S = the fp64 sum of |terms|, already scaled; c = 4 for fp16
    results, 3 + 2 sqrt(K) for fp32 results, K = the reduction length: module docstring)."""
    import torch
    if k.numel() == 0:
        return 0.0
    kd = k.double()
    sel = torch.ones_like(kd, dtype=torch.bool) if mask is None else mask
    assert torch.isfinite(kd[sel]).all(), "%s: non-finite values where the exact result is finite" % what
    c = 4.0 if k.dtype is torch.float16 else 3.0 + 2.0 * math.sqrt(K)
    bound = 0.5 * _ulp(torch.maximum(exact.abs(), kd.abs()), k.dtype) + c * U32 * S
    ratio = torch.where(sel, (kd - exact).abs() / bound, torch.zeros_like(kd))
    worst = float(ratio.max())
    assert worst <= 1.0, "%s: %d of %d elements over 0.5 ulp + %.3g u sum|terms| (worst %.3g x the bound)" % (
        what, int((ratio > 1).sum()), int(sel.sum()), c, worst)
    return worst


def _same_bits(a, b):
    """Bit-for-bit equality (signed zeros told apart); NaN only has to sit at the same places."""
    import torch
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = a.isnan(), b.isnan()
    if not torch.equal(na, nb):
        return False
    iv = torch.int16 if a.dtype is torch.float16 else torch.int32
    return torch.equal(torch.where(na, 0, a.view(iv)), torch.where(nb, 0, b.view(iv)))


# ---- fp64 restatements (torch on the GPU; pinned against oracle/corr_oracle.py by the first test) ---------------------------
def _pyr64(f1, f2, levels):
    import torch
    c = torch.einsum("ndhw,ndhv->nhwv", f1.double(), f2.double()) / math.sqrt(f1.shape[1])
    out = [c]
    for _ in range(1, levels):
        p = out[-1]
        w = p.shape[-1] // 2
        out.append(0.5 * (p[..., 0:2 * w:2] + p[..., 1:2 * w:2]))
    return out


def _bwd64(f1, f2, grads):
    """Exact d/d(f1, f2) of sum_l <level_l, grads[l]> (None: no gradient for that level)."""
    import torch
    a, b = f1.double().requires_grad_(True), f2.double().requires_grad_(True)
    pyr = _pyr64(a, b, len(grads))
    loss = sum((p * g.double()).sum() for p, g in zip(pyr, grads) if g is not None)
    return torch.autograd.grad(loss, (a, b))


def _lookup64(pyr, x, r):
    """pyr[l][N,H,W1,W2>>l] (fp64), x[N,H,W1] -> [N, L(2r+1), H, W1]: 2r+1 linear taps per level at x / 2^l, zero outside the row."""
    import torch
    outs = []
    ar = torch.arange(2 * r + 2, device=x.device, dtype=torch.float64)
    for l, v in enumerate(pyr):
        wl = v.shape[-1]
        x0 = x.double() / 2 ** l
        fl = torch.floor(x0)
        dx = (x0 - fl)[..., None]
        taps = fl[..., None] - r + ar
        ok = (taps >= 0) & (taps < wl)
        vals = torch.gather(v, -1, taps.clamp(0, wl - 1).long()) * ok
        outs.append((vals[..., :-1] * (1 - dx) + vals[..., 1:] * dx).permute(0, 3, 1, 2))
    return torch.cat(outs, 1)


def _grads_for(shape, levels, dtype, seed):
    """Per-level gradients with some levels absent (None), as autograd hands them over when a level is not used."""
    N, D, H, W1, W2 = shape
    gs = [_randn((N, H, W1, W2 >> l), seed + l, dtype=dtype) for l in range(levels)]
    if levels >= 3:
        gs[1] = None
    elif levels == 2:
        gs[0] = None
    return gs


def _fused(f1, f2, levels, grads):
    import torch
    from gps_gaussian_amd import corr as K
    t1, t2 = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    pyr = K._BuildPyramid.apply(t1, t2, levels)
    pairs = [(p, g) for p, g in zip(pyr, grads) if g is not None]
    torch.autograd.backward([p for p, _ in pairs], [g for _, g in pairs])
    return [p.detach() for p in pyr], t1.grad, t2.grad


def test_fp64_restatements_match_the_numpy_oracle():
    import torch
    from oracle import corr_oracle as CO
    shape = (2, 37, 3, 21, 45)
    N, D, H, W1, W2 = shape
    f1, f2 = _randn((N, D, H, W1), 1), _randn((N, D, H, W2), 2)
    gs = _grads_for(shape, 4, "float16", 3)
    n1, n2 = f1.double().cpu().numpy(), f2.double().cpu().numpy()
    for a, b in zip(_pyr64(f1, f2, 4), CO.build_pyramid(n1, n2, 4)):
        np.testing.assert_allclose(a.cpu().numpy(), b, rtol=1e-12, atol=1e-12)
    o1, o2 = CO.build_pyramid_backward(n1, n2, [g.double().cpu().numpy() if g is not None else None for g in gs])
    g1, g2 = _bwd64(f1, f2, gs)
    np.testing.assert_allclose(g1.cpu().numpy(), o1, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(g2.cpu().numpy(), o2, rtol=1e-12, atol=1e-12)
    x = torch.rand((N, H, W1), device="cuda", dtype=torch.float32) * (W2 + 20) - 10
    pyr = CO.build_pyramid(n1, n2, 4)
    pv = [torch.from_numpy(p).cuda().requires_grad_(True) for p in pyr]
    out = _lookup64(pv, x, 3)
    np.testing.assert_allclose(out.detach().cpu().numpy(), CO.lookup(pyr, x[:, None].cpu().numpy(), 3), rtol=1e-12, atol=1e-12)
    go = torch.randn(out.shape, device="cuda", dtype=torch.float64)
    out.backward(go)
    for v, o in zip(pv, CO.lookup_backward([p.shape[-1] for p in pyr], x[:, None].cpu().numpy(), go.cpu().numpy(), 3)):
        np.testing.assert_allclose(v.grad.cpu().numpy(), o, rtol=1e-12, atol=1e-12)


# ---- 1. forward: level 0 within one rounding of fp64, pooled levels bit-equal to avg_pool2d ------------------------------------
def _check_pyramid(pyr, f1, f2, levels, what):
    import torch
    import torch.nn.functional as F
    exact = _pyr64(f1, f2, 1)[0]
    S = _pyr64(f1.abs(), f2.abs(), 1)[0]
    _assert_rounded(pyr[0], exact, S, f1.shape[1], what + " level 0")
    for l in range(1, levels):
        prev, cur = pyr[l - 1], pyr[l]
        w = cur.shape[-1]
        assert _same_bits(cur, F.avg_pool2d(prev, [1, 2], [1, 2])), "%s level %d is not avg_pool2d of level %d" % (what, l, l - 1)
        # the same arithmetic restated: the window summed in fp32 from +0, as avg_pool2d accumulates (a window of two -0 gives +0), halved,
        # rounded once
        a, b = prev[..., 0:2 * w:2].float(), prev[..., 1:2 * w:2].float()
        assert _same_bits(cur, (((torch.zeros_like(a) + a) + b) * 0.5).to(prev.dtype)), what


@pytest.mark.parametrize("levels", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", ["float16", "float32"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_level0_one_rounding_and_pooled_levels_bitwise(name, dtype, levels):
    from gps_gaussian_amd import corr as K
    N, D, H, W1, W2 = SHAPES[name]
    f1, f2 = _randn((N, D, H, W1), 11, dtype=dtype), _randn((N, D, H, W2), 12, dtype=dtype)
    pyr = K._BuildPyramid.apply(f1, f2, levels)
    assert len(pyr) == levels and all(p.dtype == f1.dtype for p in pyr)
    _check_pyramid(pyr, f1, f2, levels, "%s/%s" % (name, dtype))


def test_fp16_forward_rounds_subnormal_correlations_instead_of_flushing():
    import torch
    from gps_gaussian_amd import corr as K
    N, D, H, W1, W2 = 2, 96, 3, 64, 132
    f1, f2 = _randn((N, D, H, W1), 21, 2.0 ** -10), _randn((N, D, H, W2), 22, 2.0 ** -10)  # |corr| ~ 2^-20: fp16 subnormals
    pyr = K._BuildPyramid.apply(f1, f2, 4)
    sub = (pyr[0] != 0) & (pyr[0].abs() < 2.0 ** -14)
    assert float(sub.float().mean()) > 0.8, "the premise: most of level 0 is subnormal in fp16"
    for p in pyr[1:]:
        assert bool(((p != 0) & (p.abs() < 2.0 ** -14)).any())
    _check_pyramid(pyr, f1, f2, 4, "subnormal")
    assert torch.isfinite(pyr[3]).all()


# ---- 2. backward against fp64, every M-tile of k_cv_bwd --------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", ["float16", "float32"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_backward_within_one_rounding_of_fp64(name, dtype, levels):
    shape = SHAPES[name]
    N, D, H, W1, W2 = shape
    f1, f2 = _randn((N, D, H, W1), 31, dtype=dtype), _randn((N, D, H, W2), 32, dtype=dtype)
    gs = _grads_for(shape, levels, dtype, 33)
    _, g1, g2 = _fused(f1, f2, levels, gs)
    assert g1.dtype == f1.dtype and g2.dtype == f2.dtype
    e1, e2 = _bwd64(f1, f2, gs)
    s1, s2 = _bwd64(f1.abs(), f2.abs(), [g.abs() if g is not None else None for g in gs])
    _assert_rounded(g1, e1, s1, W2, "%s/%s/L%d grad fmap1" % (name, dtype, levels))
    _assert_rounded(g2, e2, s2, W1, "%s/%s/L%d grad fmap2" % (name, dtype, levels))


# ---- 3. no less accurate than the reference's own fp16 chain ----------------------------------------------------------------
def _eager_block(f1, f2, coords, levels, r):
    """CorrBlockFast1D as the reference runs it under autocast, restated: fp16 einsum, divided by sqrt(D) in fp16, avg_pool2d
    pyramid, one corr_sampler call per level at coords / 2^l, concatenated."""
    import torch
    import torch.nn.functional as F
    from gps_gaussian_amd import corr as K
    N, D, H, W1 = f1.shape
    vol = torch.einsum("ndhw,ndhv->nhwv", f1, f2) / torch.sqrt(torch.tensor(float(D)))
    vols = [vol]
    for _ in range(1, levels):
        p = vols[-1]
        vols.append(F.avg_pool2d(p.reshape(N * H * W1, 1, 1, p.shape[-1]), [1, 2], stride=[1, 2]).reshape(N, H, W1, -1))
    return vols, torch.cat([K.CorrSampler.apply(v, coords / 2 ** l, r) for l, v in enumerate(vols)], dim=1)


def test_fused_fp16_chain_no_less_accurate_than_the_reference_fp16_chain_at_training_shape():
    import torch
    from gps_gaussian_amd import corr as K
    N, D, H, W1, W2 = SHAPES["train"]
    levels, r = 4, 4
    f1, f2 = _randn((N, D, H, W1), 41), _randn((N, D, H, W2), 42)
    gen = torch.Generator(device="cuda").manual_seed(43)
    coords = torch.rand((N, 1, H, W1), device="cuda", generator=gen) * (W2 + 16) - 8
    # upstream gradient as GradScaler starts: the loss scaled by 2^16
    gout = (_randn((N, levels * (2 * r + 1), H, W1), 44, 2.0 ** -10, "float32") * 2.0 ** 16).half()

    a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    blk = K.CorrBlockFast1D(a, b, num_levels=levels, radius=r)
    fused_out = blk(coords)
    fused_out.backward(gout)
    ea, eb = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    eager_vols, eager_out = _eager_block(ea, eb, coords, levels, r)
    eager_out.backward(gout)
    xa, xb = f1.double().requires_grad_(True), f2.double().requires_grad_(True)
    exact_vols = _pyr64(xa, xb, levels)
    exact_out = _lookup64(exact_vols, coords[:, 0], r)
    exact_out.backward(gout.double())

    rows = [("level%d" % l, blk.volumes[l], eager_vols[l], exact_vols[l]) for l in range(levels)]
    rows += [("lookup", fused_out, eager_out, exact_out), ("grad_fmap1", a.grad, ea.grad, xa.grad), ("grad_fmap2", b.grad, eb.grad, xb.grad)]
    report = {}
    for what, fu, ea_, ex in rows:
        assert fu.dtype == torch.float16 and ea_.dtype == torch.float16, what
        assert torch.isfinite(fu).all() and torch.isfinite(ea_).all(), what
        ef = float((fu.double() - ex.detach()).abs().max())
        ee = float((ea_.double() - ex.detach()).abs().max())
        report[what] = {"fused": ef, "eager": ee, "max_abs": float(ex.detach().abs().max())}
        assert ef <= ee, "%s: fused max|err| %.4g > the reference chain's %.4g" % (what, ef, ee)
    print(json.dumps({"fp16_chain_vs_fp64_at_training_shape": report}))


# ---- 4. the fp16 fused lookup is the per-level sampler, bit for bit -------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2, 3, 4])
@pytest.mark.parametrize("r", [4, 2])
def test_fp16_fused_lookup_is_the_per_level_sampler_bitwise(r, levels):
    import torch
    from gps_gaussian_amd import corr as K
    N, H, W1, W2 = 2, 5, 24, 72
    rd = 2 * r + 1
    vols = [_randn((N, H, W1, W2 >> l), 51 + l).requires_grad_(True) for l in range(levels)]
    gen = torch.Generator(device="cuda").manual_seed(50)
    coords = torch.rand((N, 1, H, W1), device="cuda", generator=gen) * (3 * W2 + 80) - (W2 + 40)  # well outside [0, W2) too
    out = K._LookupPyramid.apply(coords, r, *vols)
    assert out.dtype == torch.float16 and out.shape == (N, levels * rd, H, W1)
    gout = _randn(tuple(out.shape), 59)
    out.backward(gout)
    for l in range(levels):
        ref, = K.forward(vols[l].detach(), coords / 2 ** l, r)
        assert _same_bits(out[:, l * rd:(l + 1) * rd].detach(), ref), "level %d output" % l
        gref, = K.backward(vols[l].detach(), coords / 2 ** l, gout[:, l * rd:(l + 1) * rd].contiguous(), r)
        assert vols[l].grad.dtype == torch.float16 and _same_bits(vols[l].grad, gref), "level %d gradient" % l


# ---- 5. vector and scalar operand loads give the same bits ------------------------------------------------------------------
def _offset_view(t):
    """A contiguous copy of t that starts one element into its storage: data_ptr() misaligned for the 4-wide vector loads."""
    import torch
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % (4 * t.element_size()) != 0
    return v


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_misaligned_feature_maps_give_the_aligned_bits(dtype):
    N, D, H, W = 2, 40, 3, 128  # W % 4 == 0: aligned maps take the vector ld4 in both GEMMs
    f1, f2 = _randn((N, D, H, W), 61, dtype=dtype), _randn((N, D, H, W), 62, dtype=dtype)
    gs = [_randn((N, H, W, W >> l), 63 + l, dtype=dtype) for l in range(4)]
    pa, a1, a2 = _fused(f1, f2, 4, gs)
    pm, m1, m2 = _fused(_offset_view(f1), _offset_view(f2), 4, gs)
    for l in range(4):
        assert _same_bits(pa[l], pm[l]), "level %d" % l
    assert _same_bits(a1, m1) and _same_bits(a2, m2)


@pytest.mark.parametrize("which", ["all", "level3"])
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_misaligned_gradient_levels_give_the_aligned_bits(dtype, which):
    """W2 = 128 (% 8 == 0): aligned gradient levels take fold4's vector branch, one misaligned level sends the whole fold to the scalar one."""
    import torch
    from gps_gaussian_amd import corr as K
    N, D, H, W = 2, 48, 3, 128
    f1, f2 = _randn((N, D, H, W), 71, dtype=dtype), _randn((N, D, H, W), 72, dtype=dtype)
    gs = [_randn((N, H, W, W >> l), 73 + l, dtype=dtype) for l in range(4)]
    _, a1, a2 = _fused(f1, f2, 4, gs)
    ogs = [_offset_view(g) if which == "all" or l == 3 else g for l, g in enumerate(gs)]
    t1, t2 = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    pyr = K._BuildPyramid.apply(t1, t2, 4)
    seen = {}
    for l, p in enumerate(pyr):
        p.register_hook(lambda g, l=l: seen.__setitem__(l, g.data_ptr()))
    torch.autograd.backward(list(pyr), ogs)
    assert all(seen[l] == ogs[l].data_ptr() for l in range(4)), "autograd did not hand the offset views over as they are"
    assert _same_bits(a1, t1.grad) and _same_bits(a2, t2.grad)


# ---- 6. non-finite values reach the outputs (GradScaler relies on it) ------------------------------------------------------
def test_fp16_forward_overflow_is_inf_where_fp64_rounds_past_the_fp16_range():
    import torch
    import torch.nn.functional as F
    from gps_gaussian_amd import corr as K
    N, D, H, W1, W2 = 1, 64, 3, 64, 96
    f1, f2 = _randn((N, D, H, W1), 81, 200.0), _randn((N, D, H, W2), 82, 200.0)  # |corr| ~ 4e4: about one in ten rounds to inf
    pyr = K._BuildPyramid.apply(f1, f2, 4)
    exact = _pyr64(f1, f2, 1)[0]
    S = _pyr64(f1.abs(), f2.abs(), 1)[0]
    k = pyr[0].double()
    band = 4 * U32 * S + 1e-9 * FP16_MAX_FINITE_RN  # within the fp32 chain's error of the threshold either answer is right
    over = exact.abs() >= FP16_MAX_FINITE_RN + band
    under = exact.abs() < FP16_MAX_FINITE_RN - band
    assert int(over.sum()) > 100 and float((~over & ~under).float().mean()) < 1e-3, "the premise"
    assert torch.equal(k[over], torch.sign(exact[over]) * math.inf), "overflow must round to +-inf with the sign of the exact value"
    assert torch.isfinite(k[under]).all()
    _assert_rounded(pyr[0], exact, S, D, "overflow level 0", mask=under)
    saw_nan = False
    for l in range(1, 4):
        assert _same_bits(pyr[l], F.avg_pool2d(pyr[l - 1], [1, 2], [1, 2])), "level %d" % l
        saw_nan = saw_nan or bool(pyr[l].isnan().any())
        assert bool(pyr[l].isinf().any())
    assert saw_nan, "the premise: +inf and -inf meet in some pooling window"


def _oracle_backward(f1, f2, gs):
    from oracle import corr_oracle as CO
    with np.errstate(invalid="ignore", over="ignore"):
        return CO.build_pyramid_backward(f1.double().cpu().numpy(), f2.double().cpu().numpy(),
                                         [g.double().cpu().numpy() if g is not None else None for g in gs])


@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_inf_in_one_gradient_level_reaches_both_feature_map_gradients(dtype):
    import torch
    N, D, H, W1, W2 = 1, 48, 2, 40, 64
    f1, f2 = _randn((N, D, H, W1), 91, dtype=dtype), _randn((N, D, H, W2), 92, dtype=dtype)
    gs = [_randn((N, H, W1, W2 >> l), 93 + l, dtype=dtype) for l in range(4)]
    gs[2][0, 1, 5, 3] = math.inf
    _, g1, g2 = _fused(f1, f2, 4, gs)
    o1, o2 = _oracle_backward(f1, f2, gs)
    s1, s2 = _oracle_backward(f1.abs(), f2.abs(), [g.abs() for g in gs])
    for k, o, s, K, what in ((g1, o1, s1, W2, "grad fmap1"), (g2, o2, s2, W1, "grad fmap2")):
        o, s = torch.from_numpy(o).cuda(), torch.from_numpy(s).cuda()
        kd = k.double()
        assert not bool(torch.isfinite(o).all()), "the premise"
        assert torch.equal(torch.isfinite(kd), torch.isfinite(o)), what
        assert torch.equal(kd.isnan(), o.isnan()) and torch.equal(kd.isposinf(), o.isposinf()), what
        fin = torch.isfinite(o)
        _assert_rounded(k, torch.where(fin, o, 0), torch.where(fin, s, 0), K, what, mask=fin)


def test_fp16_gradient_overflow_gives_inf_not_saturation():
    import torch
    N, D, H, W1, W2 = 1, 48, 2, 40, 64
    f1, f2 = _randn((N, D, H, W1), 101, 16.0), _randn((N, D, H, W2), 102, 16.0)
    gs = [_randn((N, H, W1, W2 >> l), 103 + l, 2000.0) for l in range(4)]  # finite fp16 gradients whose result passes 65504
    assert all(bool(torch.isfinite(g).all()) for g in gs)
    _, g1, g2 = _fused(f1, f2, 4, gs)
    o1, o2 = _oracle_backward(f1, f2, gs)
    s1, s2 = _oracle_backward(f1.abs(), f2.abs(), [g.abs() for g in gs])
    for k, o, s, K, what in ((g1, o1, s1, W2, "grad fmap1"), (g2, o2, s2, W1, "grad fmap2")):
        o, s = torch.from_numpy(o).cuda(), torch.from_numpy(s).cuda()
        kd = k.double()
        band = 4 * U32 * s + 1e-9 * FP16_MAX_FINITE_RN
        over = o.abs() >= FP16_MAX_FINITE_RN + band
        under = o.abs() < FP16_MAX_FINITE_RN - band
        decided = over | under
        assert int(over.sum()) > 10 and float(decided.float().mean()) > 0.999, "the premise (%s)" % what
        # the oracle's mask: finite exactly where fp64 rounds inside the fp16 range
        assert torch.equal(torch.isfinite(kd)[decided], under[decided]), what
        assert torch.equal(kd[over], torch.sign(o[over]) * math.inf), what
        _assert_rounded(k, o, s, K, what, mask=under)


# ---- 7. fp16 upsample mask --------------------------------------------------------------------------------------------------
def test_fp16_upsample_mask_is_the_fp32_run_on_mask_float():
    import torch
    from gps_gaussian_amd import corr as K
    N, H, W, f = 2, 12, 20, 4
    flow = _randn((N, 2, H, W), 111, dtype="float32").requires_grad_(True)
    mask = _randn((N, 9 * f * f, H, W), 112, 3.0).requires_grad_(True)
    flow32 = flow.detach().clone().requires_grad_(True)
    mask32 = mask.detach().float().requires_grad_(True)
    up = K.upsample_flow(flow, mask, f)
    up32 = K.upsample_flow(flow32, mask32, f)
    assert _same_bits(up, up32)
    gout = _randn(tuple(up.shape), 113, dtype="float32")
    up.backward(gout)
    up32.backward(gout)
    assert mask.grad.dtype == torch.float16 and _same_bits(mask.grad, mask32.grad.half())
    assert _same_bits(flow.grad, flow32.grad)
