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

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import gps_gaussian_amd  # noqa: F401
from gps_gaussian_amd import _ops, accelerate as A
from gps_gaussian_amd import groupnorm as GN
from gps_gaussian_amd import stemconv as SC

import convop_run as R
from convop_run import KEYS, gamma

pytestmark = pytest.mark.gpu
K, S, P = 5, 2, 2


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
CONV = dict(stride=S, padding=P)


def _out_hw(H, W):
    return (H + 2 * P - K) // S + 1, (W + 2 * P - K) // S + 1


def _bounds(ref, N, Ci, Co, H, W, y_half=False):
    Ho, Wo = _out_hw(H, W)
    B = gamma(Ci * K * K + 1) * ref["abs_y"]
    if y_half:
        B = B + 2.0 ** -11 * (ref["y"].abs() + B) + 2.0 ** -25
    taps = (-(-K // S)) ** 2
    return dict(y=B, dx=gamma(Co * taps) * ref["abs_dx"], dw=gamma(N * Ho * Wo) * ref["abs_dw"], db=gamma(N * Ho * Wo) * ref["abs_db"])


def _aten(x, w, b, half=False):
    with torch.autocast("cuda", torch.float16, enabled=half):
        return F.conv2d(x, w, b, **CONV)


def _fused(x, w, b):
    return SC.conv2d(x, w, b, S, P)


def _inputs(gen, N, Ci, Co, H, W, half=False):
    x = torch.randn((N, Ci, H, W), generator=gen)
    w = torch.randn((Co, Ci, K, K), generator=gen) * 0.2
    b = torch.randn((Co,), generator=gen)
    w[Co // 2] = 0.0                    # one exact-zero filter
    w[0] = -w[0].abs() - 0.01           # and a negative one
    dy = torch.randn((N, Co) + _out_hw(H, W), generator=gen)
    if half:
        dy = dy.half()                  # the gradient of an fp16 output arrives in fp16; the reference starts from these values
    return dict(x=x, w=w, b=b, dy=dy, conv=CONV)


_inputs_ref_bounds = R.case_cache(_cases, _inputs, _bounds)


@functools.lru_cache(maxsize=None)
def _case(name, half=False):
    """The shared case and ATen's GPU result for it, computed once as well; ATen's fp16 backward is not run (see the top of the file)."""
    c = _inputs_ref_bounds(name, half)
    return dict(c, aten=R.run_case(functools.partial(_aten, half=half), c, backward=not half))


def _report(rec):
    R.emit(rec)
    out = os.environ.get("GPSGS_PARITY_DIR")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "stemconv_parity.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")


def _check(test, name, got, c, half=False):
    aten = {k: R.ratio(c["aten"][k], c["ref"][k], c["bounds"][k]) if c["aten"][k] is not None else None for k in KEYS}
    return R.check(dict(test=test, case=name, dims=list(c["dims"]), y_dtype="fp16" if half else "fp32"), "fused", got, c["ref"], c["bounds"],
                   dtype=None, more=dict(aten=aten), emit=_report)


@pytest.mark.parametrize("name", CASES)
def test_fp32_forward_and_backward_within_the_bounds(name):
    c = _case(name)
    got = R.run_case(_fused, c)
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


@pytest.mark.parametrize("which", ["cin3_tile+1", "cin1_9x11"])
def test_small_integers_give_the_exact_answer(which):
    TH, TW = _tile()
    N, Ci, Co, H, W = (2, 3, 32, 2 * TH + 1, 2 * TW + 1) if which == "cin3_tile+1" else (2, 1, 8, 9, 11)
    R.exact_integers(which, _fused, ((N, Ci, H, W), (Co, Ci, K, K), (Co,), (N, Co) + _out_hw(H, W)), **CONV)


def test_two_runs_give_the_same_bits():
    R.two_runs(functools.partial(R.run_case, _fused), [("tile_2T+1_T-1_odd", _case("tile_2T+1_T-1_odd"))])


def test_requires_grad_handling(monkeypatch):
    R.requires_grad_matrix(monkeypatch, SC, "sc_backward", _fused, _case("cin_1_64x130"), double_weight=False)


def test_what_the_op_does_not_take_goes_through_aten():
    torch.manual_seed(4)
    plain = nn.Conv2d(3, 32, K, stride=S, padding=P).cuda()
    fused = copy.deepcopy(plain)
    assert SC.convert(fused) == 1
    x = torch.randn(2, 3, 20, 22, device="cuda")

    both = R.passthrough_pair(A.calls, "stemconv")

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
        rec["aten"][n], rec["fused"][n] = R.rel_err(ta, t64), R.rel_err(tf, t64)
    _report(rec)
    for n in names:
        floor = 1e-6 if n == "out" else 1e-3
        assert rec["fused"][n] <= max(2.0 * rec["aten"][n], floor), "%s: fused %.3e, ATen %.3e" % (n, rec["fused"][n], rec["aten"][n])
