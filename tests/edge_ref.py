"""Shared restatements for the edge tests of the convex upsampling (csrc/corr_pyramid.hip k_up_*) and the fused L1 + SSIM loss
(csrc/fused_loss.hip).  TEST INFRASTRUCTURE ONLY: everything here runs on the CPU.

  * eager restatements of the reference's own formulas in torch, run in fp32 (the yardstick: what the fused kernels replace) and in fp64 with
    autograd (a gradient that owes nothing to the hand-derived maps of oracle/loss_oracle.py or to oracle/corr_oracle.py's backward):
    upsample_eager   core/raft_stereo_human.py:69-81 (softmax over the 9 taps, unfold, sum);
    ssim_eager       lib/loss.py:40-83 (fp32-normalised 11-tap window, five depthwise convolutions, the SSIM map, its mean);
  * the error criterion of tests/test_gpu_groupnorm.py: err(t) = max |t - t64| / max |t64|, fused <= max(2 x eager fp32, floor);
  * the integer one-hot routing of the upsampling (forward gather and backward scatter in exact integer arithmetic);
  * the cases (inputs, fp64 reference, eager fp32 result): computed once per process, shared, never modified.
"""
import functools
import json
import os
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import corr_oracle as CO
from oracle import loss_oracle as LO

# (N, C, H, W, f): W on both sides of one and two 64-column tiles of k_up_bwd_cells; f^2 = 1, 4, 9, 16, 64 (idle wave groups, an uneven split);
# both channel counts; H = 1, 2, 3 (every border tap)
UP_SHAPES = [(1, 1, 1, 1, 1), (2, 2, 3, 63, 2), (2, 2, 2, 64, 4), (2, 1, 3, 65, 3), (1, 2, 2, 130, 8), (1, 2, 1, 129, 1)]
# k_loss_fwd takes its 16-byte loads where x0 >= 5 and x0 + 39 <= W: from W = 71 in the second tile column, from W = 103 in the third
LOSS_SHAPES = [(1, 2, 33, W) for W in (70, 71, 72, 102, 103, 104)] + [(1, 1, 6, 38), (1, 1, 6, 39), (1, 1, 1, 1), (1, 1, 1, 200), (1, 1, 200, 1),
                                                                        (3, 1, 40, 70)]
DEGENERATE = ["identical", "ones", "zeros", "two_constants"]
DEGENERATE_SHAPE = (1, 1, 33, 71)


def sid(shape):
    return "x".join(str(s) for s in shape)


def _seed(*key):
    return zlib.crc32(repr(key).encode())


# ---- the criterion ----------------------------------------------------------------------------------------------------------
def err(t, t64):
    """max |t - t64| / max |t64| (t: anything torch / numpy, on any device)."""
    t = torch.as_tensor(t).detach().double().cpu()
    t64 = torch.as_tensor(t64).detach().double().cpu()
    return float((t - t64).abs().max() / t64.abs().max().clamp_min(1e-300))


def report(rec):
    """One JSON line per case and quantity: printed, and appended to loss_upsample_parity.jsonl where GPSGS_PARITY_DIR names a directory."""
    line = json.dumps(rec)
    print(line)
    out = os.environ.get("GPSGS_PARITY_DIR")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "loss_upsample_parity.jsonl"), "a") as f:
            f.write(line + "\n")
    return rec


def check(test, case, quantity, fused, eager, ref, floor):
    """Report and assert err(fused) <= max(2 err(eager), floor)."""
    e_f, e_e = err(fused, ref), err(eager, ref)
    bound = max(2.0 * e_e, floor)
    report(dict(test=test, case=case, quantity=quantity, err_fused=e_f, err_eager=e_e, floor=floor, bound=bound))
    assert bool(torch.isfinite(torch.as_tensor(fused)).all()), (case, quantity)
    assert e_f <= bound, "%s %s: fused %.3e, eager fp32 %.3e, floor %.3e" % (case, quantity, e_f, e_e, floor)


def bits(t):
    """The bit pattern of an fp32 / fp16 tensor (so that +0 and -0, or two NaNs, are told apart)."""
    t = t.detach().contiguous().cpu()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---- convex upsampling ------------------------------------------------------------------------------------------------------
def upsample_eager(flow, mask, f):
    """core/raft_stereo_human.py:69-81, in the dtype of its arguments."""
    N, D, H, W = flow.shape
    mask = mask.view(N, 1, 9, f, f, H, W)
    mask = torch.softmax(mask, dim=2)
    up = F.unfold(f * flow, [3, 3], padding=1)
    up = up.view(N, D, 9, 1, 1, H, W)
    up = torch.sum(mask * up, dim=2)
    up = up.permute(0, 1, 4, 2, 5, 3)
    return up.reshape(N, D, f * H, f * W)


def upsample_autograd(flow, mask, gout, f, dtype):
    """-> dict(out, gflow, gmask) of the eager restatement in `dtype` on the CPU."""
    fl = torch.as_tensor(flow).detach().to(dtype).clone().requires_grad_(True)
    mk = torch.as_tensor(mask).detach().to(dtype).clone().requires_grad_(True)
    out = upsample_eager(fl, mk, f)
    out.backward(torch.as_tensor(gout).to(dtype))
    return dict(out=out.detach(), gflow=fl.grad, gmask=mk.grad)


def upsample_oracle(flow, mask, gout, f):
    """-> dict(out, gflow, gmask), fp64, from oracle/corr_oracle.py."""
    flow, mask, gout = (np.asarray(t, np.float64) for t in (flow, mask, gout))
    gf, gm = CO.upsample_flow_backward(flow, mask, gout, f)
    return dict(out=torch.from_numpy(CO.upsample_flow(flow, mask, f)), gflow=torch.from_numpy(gf), gmask=torch.from_numpy(gm))


@functools.lru_cache(maxsize=None)
def up_case(shape, kind="random"):
    """randn flow, 3 randn mask, randn grad_out (fp32 torch, CPU) with the fp64 oracle's and the eager fp32 results.
    kind "spike": one logit per fine pixel 80 above the rest."""
    N, C, H, W, f = shape
    gen = torch.Generator().manual_seed(_seed("up", shape, kind))
    flow = torch.randn(N, C, H, W, generator=gen)
    mask = 3.0 * torch.randn(N, 9 * f * f, H, W, generator=gen)
    gout = torch.randn(N, C, f * H, f * W, generator=gen)
    if kind == "spike":
        k = torch.from_numpy(kstar(shape))                                           # [N,f,f,H,W]
        hot = F.one_hot(k, 9).permute(0, 5, 1, 2, 3, 4).reshape(N, 9 * f * f, H, W)  # tap-major, as the mask is laid out
        mask = mask + 80.0 * hot
    return dict(shape=shape, flow=flow, mask=mask, gout=gout, ref=upsample_oracle(flow.numpy(), mask.numpy(), gout.numpy(), f),
                eager=upsample_autograd(flow, mask, gout, f, torch.float32))


def kstar(shape, const=None):
    """The selected tap of every fine pixel, [N,f,f,H,W] int64: a fixed function of (n, h, w, i, j) that takes all nine values along w alone
    (and along every other index by a step coprime to 9 or 3), or one tap for the whole tensor."""
    N, C, H, W, f = shape
    n, i, j, h, w = np.meshgrid(np.arange(N), np.arange(f), np.arange(f), np.arange(H), np.arange(W), indexing="ij")
    if const is not None:
        return np.full(n.shape, int(const), np.int64)
    return ((4 * n + 2 * i + 7 * j + 5 * h + w) % 9).astype(np.int64)


def onehot_case(shape, const=None):
    """Integer flow and grad_out in [-8, 8], logits 0 at the selected tap and -200 elsewhere (fp32 softmax: exactly one-hot), and what the
    routing gives in exact integer arithmetic: out = f flow[h + k/3 - 1, w + k%3 - 1] (zero outside), grad_flow = the scatter of f grad_out."""
    N, C, H, W, f = shape
    rng = np.random.default_rng(_seed("onehot", shape, const))
    flow = rng.integers(-8, 9, (N, C, H, W))
    gout = rng.integers(-8, 9, (N, C, f * H, f * W))
    k = kstar(shape, const)
    mask = np.full((N, 9, f, f, H, W), -200.0, np.float32)
    np.put_along_axis(mask, k[:, None], 0.0, axis=1)
    n, i, j, h, w = np.meshgrid(np.arange(N), np.arange(f), np.arange(f), np.arange(H), np.arange(W), indexing="ij")
    hh, ww = h + k // 3 - 1, w + k % 3 - 1
    ok = (hh >= 0) & (hh < H) & (ww >= 0) & (ww < W)
    out = np.zeros((N, C, f * H, f * W), np.int64)
    gflow = np.zeros((N, C, H, W), np.int64)
    for c in range(C):
        out[n[ok], c, (h * f + i)[ok], (w * f + j)[ok]] = f * flow[n[ok], c, hh[ok], ww[ok]]
        np.add.at(gflow, (n[ok], c, hh[ok], ww[ok]), f * gout[n[ok], c, (h * f + i)[ok], (w * f + j)[ok]])
    # the largest magnitude any exact partial sum can reach: every tap of every fine pixel of the 9 cells around one flow element
    worst = int(max(np.abs(out).max(), 9 * f * f * f * np.abs(gout).max()))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return dict(shape=shape, flow=t(flow), mask=t(mask.reshape(N, 9 * f * f, H, W)), gout=t(gout), out=t(out), gflow=t(gflow), k=k, worst=worst)


def shift_case(shape):
    """Logits that are multiples of 1/8 in [-4, 4], and the same logits with one constant of {0, 4096, -4096} per fine pixel added to all nine
    taps (exact in fp32: 13 + 3 bits): softmax cannot tell them apart."""
    N, C, H, W, f = shape
    gen = torch.Generator().manual_seed(_seed("shift", shape))
    flow = torch.randn(N, C, H, W, generator=gen)
    gout = torch.randn(N, C, f * H, f * W, generator=gen)
    mask = torch.randint(-32, 33, (N, 9, f, f, H, W), generator=gen).float() / 8.0
    n, i, j, h, w = np.meshgrid(np.arange(N), np.arange(f), np.arange(f), np.arange(H), np.arange(W), indexing="ij")
    const = torch.from_numpy(np.array([0.0, 4096.0, -4096.0], np.float32)[(n + i + 2 * j + h + w) % 3])
    moved = mask + const[:, None]
    assert torch.equal((moved - const[:, None]), mask)           # the addition was exact
    return dict(shape=shape, flow=flow, gout=gout, mask=mask.reshape(N, 9 * f * f, H, W), moved=moved.reshape(N, 9 * f * f, H, W))


# ---- L1 + SSIM ----------------------------------------------------------------------------------------------------------------
def ssim_window(channel, like):
    """lib/loss.py:40-49: the 1-D Gaussian normalised in fp32, the 2-D window its fp32 outer product, then cast to the image's dtype."""
    g = torch.Tensor([np.exp(-(x - 11 // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)])
    g = (g / g.sum()).unsqueeze(1)
    w2 = g.mm(g.t()).float().unsqueeze(0).unsqueeze(0)
    return w2.expand(channel, 1, 11, 11).contiguous().type_as(like)


def ssim_eager(img1, img2):
    """lib/loss.py:52-83 on [B,C,H,W], in the dtype of its arguments."""
    channel = img1.size(-3)
    window = ssim_window(channel, img1)
    mu1 = F.conv2d(img1, window, padding=5, groups=channel)
    mu2 = F.conv2d(img2, window, padding=5, groups=channel)
    mu1_sq = mu1.pow(2)
    mu2_sq = mu2.pow(2)
    mu1_mu2 = mu1 * mu2
    sigma1_sq = F.conv2d(img1 * img1, window, padding=5, groups=channel) - mu1_sq
    sigma2_sq = F.conv2d(img2 * img2, window, padding=5, groups=channel) - mu2_sq
    sigma12 = F.conv2d(img1 * img2, window, padding=5, groups=channel) - mu1_mu2
    C1 = 0.01 ** 2
    C2 = 0.03 ** 2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    return ssim_map.mean()


def ssim_autograd(pred, gt, dtype):
    """-> (value, gradient w.r.t. pred) of the eager restatement in `dtype` on the CPU."""
    p = torch.as_tensor(pred).detach().to(dtype).clone().requires_grad_(True)
    s = ssim_eager(p, torch.as_tensor(gt).to(dtype))
    g, = torch.autograd.grad(s, p)
    return float(s.detach()), g


def loss_refs(pred, gt):
    """The references of one [B,C,H,W] fp32 pair: the fp64 oracle's SSIM value and gradient and its L1, fp64 autograd of the eager restatement,
    the eager fp32 result, and the floors: the distance between the two fp64 references (they differ in the fp32 normalisation of the window)."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    s_or, g_or = LO.ssim(pred, gt, with_grad=True)
    g_or = torch.from_numpy(g_or)
    s64, g64 = ssim_autograd(pred, gt, torch.float64)
    s32, g32 = ssim_autograd(pred, gt, torch.float32)
    gmax = float(g_or.abs().max())
    return dict(pred=torch.from_numpy(pred), gt=torch.from_numpy(gt), l1=float(LO.l1(pred, gt)), ssim=float(s_or), grad=g_or, ssim64=s64, grad64=g64,
                ssim32=s32, grad32=g32, floor_value=abs(float(s_or) - s64), floor_grad=err(g64, g_or) if gmax > 0 else 0.0)


@functools.lru_cache(maxsize=None)
def loss_case(shape):
    """pred ~ U(0,1), gt = clip(pred + 0.2 randn, 0, 1)."""
    rng = np.random.default_rng(_seed("loss", shape))
    pred = rng.uniform(0, 1, shape).astype(np.float32)
    gt = np.clip(pred + 0.2 * rng.standard_normal(shape), 0, 1).astype(np.float32)
    return loss_refs(pred, gt)


@functools.lru_cache(maxsize=None)
def degenerate_case(name):
    shape = DEGENERATE_SHAPE
    if name == "identical":
        pred = np.random.default_rng(_seed("degenerate")).uniform(0, 1, shape).astype(np.float32)
        gt = pred.copy()
    else:
        a, b = {"ones": (1.0, 1.0), "zeros": (0.0, 0.0), "two_constants": (0.5, 0.25)}[name]
        pred, gt = np.full(shape, a, np.float32), np.full(shape, b, np.float32)
    return loss_refs(pred, gt)


SHIFT_HW, SHIFT_BLOCK, SHIFT_AT, SHIFT_MARGIN = (96, 128), 40, (12, 12), 10
SHIFTS = [(4, 20), (32, 64), (17, 23), (43, 75)]      # the first two: multiples of 4 in both axes (the same register slot of a thread's 4 outputs)


def shift_hw(dy, dx):
    """The image of one shift: 96 x 128, or the smallest that keeps SHIFT_MARGIN zero pixels beyond the moved block (105 x 137 for (43, 75), whose
    block would otherwise end one pixel from the border, where SSIM-map pixels the gradient needs fall outside the image and the mean)."""
    return (max(SHIFT_HW[0], SHIFT_AT[0] + dy + SHIFT_BLOCK + SHIFT_MARGIN), max(SHIFT_HW[1], SHIFT_AT[1] + dx + SHIFT_BLOCK + SHIFT_MARGIN))


def shifted_pair(hw, dy, dx):
    """Zero [1,1,H,W] images holding one 40 x 40 random block (in pred and, perturbed, in gt) at (12 + dy, 12 + dx).  At least 10 zero pixels -- the
    reach of the forward window plus the backward window -- remain on every side."""
    B, (y0, x0), (H, W) = SHIFT_BLOCK, SHIFT_AT, hw
    assert min(y0 + dy, x0 + dx, H - (y0 + dy + B), W - (x0 + dx + B)) >= SHIFT_MARGIN
    rng = np.random.default_rng(_seed("shift-block"))
    bp = rng.uniform(0, 1, (B, B)).astype(np.float32)
    bg = np.clip(bp + 0.2 * rng.standard_normal((B, B)), 0, 1).astype(np.float32)
    pred, gt = np.zeros((1, 1, H, W), np.float32), np.zeros((1, 1, H, W), np.float32)
    pred[0, 0, y0 + dy:y0 + dy + B, x0 + dx:x0 + dx + B] = bp
    gt[0, 0, y0 + dy:y0 + dy + B, x0 + dx:x0 + dx + B] = bg
    return pred, gt
