"""GPU (-m gpu): the stem-convolution kernels (csrc/stem_conv.hip; stemconv.conv2d / FusedStemConv2d) against F.conv2d and its autograd in fp64 on
the CPU, starting from the same fp32 inputs (or the fp16 dy values).

The bounds are derived, not measured, and hold for any summation order.  With u = 2^-24 and g(n) = n u / (1 - n u), elementwise:
    y            |y - y64| <= g(C_in K^2 + 1) (sum |w||x| + |b|)                 =: B
    y in fp16    <= B + 2^-11 (|y64| + B) + 2^-25
    dx           <= g(C_out ceil(K/S)^2) sum |w||dy|
    dw, db       <= g(N Ho Wo) sum |dy||x|,  g(N Ho Wo) sum |dy|
the sums of absolute values coming from the same fp64 convolution (and its autograd) applied to |x|, |w|, |b|, |dy|.  Every case prints the worst
ratio error / bound of the fused op and of ATen's own GPU result and, where GPSGS_PARITY_DIR names a directory, appends them to
stemconv_parity.jsonl there.

Under fp16 autocast only ATen's FORWARD runs on the GPU (its dtype is what the fused result is compared with, and its y error is printed); ATen's fp16
BACKWARD is not run: inside the whole suite the library's solver search for the backward of [2,1,33,65] -> 40 channels (MIOpen, "EvaluateInvokers")
ended in an illegal memory access in one of its candidate kernels, which takes every later test of the process with it.  The fused op's fp16 gradients
are still held to their bounds; ATen's fp16 gradient errors are simply not printed beside them."""
import copy
import functools
import json
import os
import zlib

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import gps_gaussian_amd  # noqa: F401
from gps_gaussian_amd import _ops, accelerate as A
from gps_gaussian_amd import groupnorm as GN
from gps_gaussian_amd import stemconv as SC

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
K, S, P = 5, 2, 2
KEYS = ("y", "dx", "dw", "db")


def _gamma(n):
    return n * U / (1.0 - n * U)


def _tile():
    return _ops.tile("sc_tile")


@functools.lru_cache(maxsize=None)
def _cases():
    """name -> (N, C_in, C_out, H, W)"""
    TH, TW = _tile()
    c = {}
    for tag, (Ho, Wo) in (("T-1", (TH - 1, TW - 1)), ("T", (TH, TW)), ("T+1", (TH + 1, TW + 1)), ("2T+1_T-1", (2 * TH + 1, TW - 1)),
                          ("1_2T+1", (1, 2 * TW + 1))):
        c["tile_%s_even" % tag] = (2, 3, 32, 2 * Ho, 2 * Wo)          # H = 2 Ho and H = 2 Ho - 1 both give Ho
        c["tile_%s_odd" % tag] = (2, 3, 32, 2 * Ho - 1, 2 * Wo - 1)
    c["one_pixel"] = (1, 1, 32, 1, 1)                                  # every tap but the centre is padding
    c["tiny_3x1x2x3"] = (3, 1, 32, 2, 3)
    c["tiny_2x3x5x7"] = (2, 3, 32, 5, 7)
    c["ragged_37x41"] = (1, 3, 32, 37, 41)                             # rows start off 16-byte boundaries
    for co in (8, 40, 64):
        c["cout_%d" % co] = (2, 1, co, 33, 65)
    c["cin_1_64x130"] = (2, 1, 32, 64, 130)
    c["cin_3_64x130"] = (2, 3, 32, 64, 130)
    c["ref_cin_3"] = (2, 3, 32, 256, 256)
    c["ref_cin_1"] = (2, 1, 32, 256, 256)
    return c


TILE_TAGS = ["T-1", "T", "T+1", "2T+1_T-1", "1_2T+1"]
CASES = ["tile_%s_%s" % (t, p) for t in TILE_TAGS for p in ("even", "odd")] + \
        ["one_pixel", "tiny_3x1x2x3", "tiny_2x3x5x7", "ragged_37x41", "cout_8", "cout_40", "cout_64", "cin_1_64x130", "cin_3_64x130", "ref_cin_3", "ref_cin_1"]
FP16_CASES = ["tile_T+1_odd", "ragged_37x41", "cout_40"]


def _out_hw(H, W):
    return (H + 2 * P - K) // S + 1, (W + 2 * P - K) // S + 1


def _ref64(x, w, b, dy):
    """The fp64 convolution with its gradients, and the same applied to absolute values (the sums the bounds are made of)."""
    out = {}
    for tag, f in (("", lambda t: t), ("abs_", torch.abs)):
        x64, w64, b64 = (f(t.double().cpu()).requires_grad_(True) for t in (x, w, b))
        y = F.conv2d(x64, w64, b64, stride=S, padding=P)
        y.backward(f(dy.double().cpu()))
        out.update({tag + "y": y.detach(), tag + "dx": x64.grad, tag + "dw": w64.grad, tag + "db": b64.grad})
    return out


def _bounds(ref, N, Ci, Co, H, W, y_half):
    Ho, Wo = _out_hw(H, W)
    B = _gamma(Ci * K * K + 1) * ref["abs_y"]
    if y_half:
        B = B + 2.0 ** -11 * (ref["y"].abs() + B) + 2.0 ** -25
    taps = (-(-K // S)) ** 2
    return dict(y=B, dx=_gamma(Co * taps) * ref["abs_dx"], dw=_gamma(N * Ho * Wo) * ref["abs_dw"], db=_gamma(N * Ho * Wo) * ref["abs_db"])


def _run(op, x, w, b, dy, autocast, backward=True):
    """op(x, w, b) on the GPU -> y, dx, dw, db (as computed, dtypes included); backward=False: y alone."""
    xg, wg, bg = (t.cuda().requires_grad_(backward) for t in (x, w, b))
    with torch.autocast("cuda", torch.float16, enabled=autocast):
        y = op(xg, wg, bg)
    if backward:
        y.backward(dy.cuda().to(y.dtype))
    torch.cuda.synchronize()
    return dict(y=y.detach(), dx=xg.grad, dw=wg.grad, db=bg.grad)


def _aten(x, w, b):
    return F.conv2d(x, w, b, stride=S, padding=P)


def _fused(x, w, b):
    half = torch.is_autocast_enabled()
    return SC.conv2d(x, w, b, S, P, out_dtype=torch.float16 if half else torch.float32)


@functools.lru_cache(maxsize=None)
def _case(name, half=False):
    """Inputs, the fp64 reference, the bounds and ATen's GPU result of one case: computed once, shared by every test that needs them, never modified."""
    N, Ci, Co, H, W = _cases()[name]
    Ho, Wo = _out_hw(H, W)
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()) + int(half))
    x = torch.randn((N, Ci, H, W), generator=gen)
    w = torch.randn((Co, Ci, K, K), generator=gen) * 0.2
    b = torch.randn((Co,), generator=gen)
    w[Co // 2] = 0.0                    # one exact-zero filter
    w[0] = -w[0].abs() - 0.01           # and a negative one
    dy = torch.randn((N, Co, Ho, Wo), generator=gen)
    if half:
        dy = dy.half()                  # the gradient of an fp16 output arrives in fp16; the reference starts from these values
    ref = _ref64(x, w, b, dy)
    return dict(dims=(N, Ci, Co, H, W), x=x, w=w, b=b, dy=dy, ref=ref, bounds=_bounds(ref, N, Ci, Co, H, W, half),
                aten=_run(_aten, x, w, b, dy, half, backward=not half))   # ATen's fp16 backward is not run (see the top of the file)


def _ratio(t, t64, bound):
    """The worst error / bound; an error of zero is inside any bound (also a bound of zero), an error above a zero bound is infinite."""
    d = (t.detach().double().cpu() - t64).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / bound.clamp_min(1e-300))
    return float(r.max())


def _report(rec):
    line = json.dumps(rec)
    print(line)
    out = os.environ.get("GPSGS_PARITY_DIR")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "stemconv_parity.jsonl"), "a") as f:
            f.write(line + "\n")


def _check(test, name, got, c, half=False):
    rec = dict(test=test, case=name, dims=list(c["dims"]), y_dtype="fp16" if half else "fp32", fused={}, aten={})
    for k in KEYS:
        assert got[k].shape == c["ref"][k].shape, k
        rec["fused"][k] = _ratio(got[k], c["ref"][k], c["bounds"][k])
        rec["aten"][k] = _ratio(c["aten"][k], c["ref"][k], c["bounds"][k]) if c["aten"][k] is not None else None
    _report(rec)
    for k in KEYS:
        assert torch.isfinite(got[k]).all(), k
        assert rec["fused"][k] <= 1.0, "%s %s: error / bound = %.3f (ATen: %s)" % (name, k, rec["fused"][k], rec["aten"][k])
    return rec


@pytest.mark.parametrize("name", CASES)
def test_fp32_forward_and_backward_within_the_bounds(name):
    c = _case(name)
    got = _run(_fused, c["x"], c["w"], c["b"], c["dy"], False)
    assert all(got[k].dtype == torch.float32 for k in KEYS)
    _check("fp32", name, got, c)


@pytest.mark.parametrize("name", FP16_CASES)
def test_fp16_autocast(name):
    c = _case(name, half=True)
    N, Ci, Co, H, W = c["dims"]
    m = nn.Conv2d(Ci, Co, K, stride=S, padding=P).cuda()
    with torch.no_grad():
        m.weight.copy_(c["w"])
        m.bias.copy_(c["b"])
    assert SC.convert(m) == 1
    n0, p0 = A.calls["stemconv"], A.calls["stemconv_passthrough"]
    xg = c["x"].cuda().requires_grad_(True)
    with torch.autocast("cuda", torch.float16):
        y = m(xg)
    assert y.dtype == torch.float16 == c["aten"]["y"].dtype          # what ATen returns under the same autocast
    y.backward(c["dy"].cuda())                                         # dy in fp16
    torch.cuda.synchronize()
    assert A.calls["stemconv"] == n0 + 1 and A.calls["stemconv_passthrough"] == p0
    got = dict(y=y.detach(), dx=xg.grad, dw=m.weight.grad, db=m.bias.grad)
    assert got["dx"].dtype == got["dw"].dtype == got["db"].dtype == torch.float32
    _check("fp16_autocast", name, got, c, half=True)


def _ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


@pytest.mark.parametrize("which", ["cin3_tile+1", "cin1_9x11"])
def test_small_integers_give_the_exact_answer(which):
    """x in [-3, 3], w, b, dy in [-2, 2]: every product and partial sum is an integer far below 2^24, so y, dx, dw, db must EQUAL the fp64 result."""
    TH, TW = _tile()
    N, Ci, Co, H, W = (2, 3, 32, 2 * TH + 1, 2 * TW + 1) if which == "cin3_tile+1" else (2, 1, 8, 9, 11)
    Ho, Wo = _out_hw(H, W)
    gen = torch.Generator().manual_seed(zlib.crc32(which.encode()))
    x, w, b, dy = _ints((N, Ci, H, W), -3, 3, gen), _ints((Co, Ci, K, K), -2, 2, gen), _ints((Co,), -2, 2, gen), _ints((N, Co, Ho, Wo), -2, 2, gen)
    ref = _ref64(x, w, b, dy)
    got = _run(_fused, x, w, b, dy, False)
    for k in KEYS:
        assert torch.equal(got[k].double().cpu(), ref[k]), k


def test_two_runs_give_the_same_bits():
    c = _case("tile_2T+1_T-1_odd")
    a = _run(_fused, c["x"], c["w"], c["b"], c["dy"], False)
    b = _run(_fused, c["x"], c["w"], c["b"], c["dy"], False)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k


def test_requires_grad_handling():
    c = _case("cin_1_64x130")
    full = _run(_fused, c["x"], c["w"], c["b"], c["dy"], False)
    x, w, b, dy = (c[k].cuda() for k in ("x", "w", "b", "dy"))
    # x does not require grad: no input gradient, the same parameter gradients
    wg, bg = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = SC.conv2d(x, wg, bg, S, P)
    y.backward(dy)
    assert x.grad is None and torch.equal(y.detach(), full["y"]) and torch.equal(wg.grad, full["dw"]) and torch.equal(bg.grad, full["db"])
    # the weight frozen, then the bias frozen
    xg, bg = x.clone().requires_grad_(True), b.clone().requires_grad_(True)
    SC.conv2d(xg, w, bg, S, P).backward(dy)
    assert w.grad is None and torch.equal(xg.grad, full["dx"]) and torch.equal(bg.grad, full["db"])
    wg = w.clone().requires_grad_(True)
    SC.conv2d(x, wg, b, S, P).backward(dy)
    assert b.grad is None and torch.equal(wg.grad, full["dw"])
    # only x
    xg = x.clone().requires_grad_(True)
    SC.conv2d(xg, w, b, S, P).backward(dy)
    assert torch.equal(xg.grad, full["dx"])
    with torch.no_grad():
        y0 = SC.conv2d(x, wg, bg, S, P)
    assert y0.grad_fn is None and torch.equal(y0, full["y"])


def test_what_the_op_does_not_take_goes_through_aten():
    torch.manual_seed(4)
    plain = nn.Conv2d(3, 32, K, stride=S, padding=P).cuda()
    fused = copy.deepcopy(plain)
    assert SC.convert(fused) == 1
    x = torch.randn(2, 3, 20, 22, device="cuda")

    def both(a, b, inp, **ac):
        n0, p0 = A.calls["stemconv"], A.calls["stemconv_passthrough"]
        with torch.autocast("cuda", enabled=bool(ac), **ac):
            ya, yb = a(inp), b(inp)
        assert A.calls["stemconv"] == n0 and A.calls["stemconv_passthrough"] == p0 + 1
        assert ya.dtype == yb.dtype and ya.shape == yb.shape and ya.stride() == yb.stride() and torch.equal(ya, yb)

    both(plain, fused, x.to(memory_format=torch.channels_last))                                  # channels-last input
    both(copy.deepcopy(plain).half(), copy.deepcopy(fused).half(), x.half())                      # fp16 input outside autocast
    both(plain, fused, x, dtype=torch.bfloat16)                                                   # bf16 autocast
    nb = nn.Conv2d(3, 32, K, stride=S, padding=P, bias=False).cuda()
    fb = copy.deepcopy(nb)
    assert SC.convert(fb) == 0
    fb.__class__ = SC.FusedStemConv2d
    both(nb, fb, x)                                                                               # no bias
    c3 = nn.Conv2d(3, 32, 3, padding=1).cuda()
    f3 = copy.deepcopy(c3)
    assert SC.convert(f3) == 0
    f3.__class__ = SC.FusedStemConv2d                                                             # a 3x3 layer force-swapped
    both(c3, f3, x)
    both(plain, fused, x[:0])                                                                     # an empty batch
    n0 = A.calls["stemconv"]
    assert fused(x).dtype == torch.float32 and A.calls["stemconv"] == n0 + 1                      # and the ordinary call is the fused one


def _err(t, t64):
    return float((t.detach().double().cpu() - t64).abs().max() / t64.abs().max().clamp_min(1e-300))


def test_the_whole_stem():
    """Conv -> GroupNorm -> ReLU with all three layers on this package's kernels, against the fp64 module on the CPU under the criterion of
    test_gpu_groupnorm_epilogue.py: err = max |t - t64| / max |t64|, fused <= max(2 x ATen's error, floor) -- floor 1e-6 for the output, 1e-3 for
    the gradients (that file's stand-in network: an activation within rounding of the ReLU's kink flips a mask in either fp32 run)."""
    torch.manual_seed(33)
    base = nn.Sequential(nn.Conv2d(3, 32, K, stride=S, padding=P), nn.GroupNorm(8, 32), nn.ReLU(inplace=True))
    with torch.no_grad():
        base[1].weight.normal_()
        base[1].bias.normal_()
    x, g = torch.randn(2, 3, 40, 36), torch.randn(2, 32, 20, 18)
    ref = copy.deepcopy(base).double()
    out64 = ref(x.double())
    out64.backward(g.double())
    aten, fused = copy.deepcopy(base).cuda(), copy.deepcopy(base).cuda()
    assert SC.convert(fused) == 1 and GN.convert(fused) == 1 and GN.fuse_sequential_relu(fused) == 1
    assert [type(m) for m in fused] == [SC.FusedStemConv2d, GN.FusedGroupNormReLU, nn.Identity]
    assert list(fused.state_dict().keys()) == list(base.state_dict().keys())
    n0, g0 = A.calls["stemconv"], A.calls["groupnorm"]
    res = {}
    for tag, net in (("aten", aten), ("fused", fused)):
        out = net(x.cuda())
        out.backward(g.cuda())
        torch.cuda.synchronize()
        res[tag] = [out.detach()] + [p.grad for p in net.parameters()]
    assert A.calls["stemconv"] > n0 and A.calls["groupnorm"] > g0
    names = ["out"] + [n for n, _ in base.named_parameters()]
    refs = [out64.detach()] + [p.grad for p in ref.parameters()]
    rec = dict(test="whole_stem", fused={}, aten={})
    for n, t64, ta, tf in zip(names, refs, res["aten"], res["fused"]):
        rec["aten"][n], rec["fused"][n] = _err(ta, t64), _err(tf, t64)
    _report(rec)
    for n in names:
        floor = 1e-6 if n == "out" else 1e-3
        assert rec["fused"][n] <= max(2.0 * rec["aten"][n], floor), "%s: fused %.3e, ATen %.3e" % (n, rec["fused"][n], rec["aten"][n])
