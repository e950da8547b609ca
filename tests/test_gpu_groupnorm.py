"""GPU (-m gpu): the chip-wide GroupNorm kernels (csrc/group_norm.hip; groupnorm.group_norm / FusedGroupNorm) against F.group_norm in fp64 on the
CPU, with ATen's own fp32 / autocast result on the GPU as the yardstick for the error.

The bound is measured, not guessed: for y, dx, dgamma, dbeta the error is max |t - t64| / max |t64|, and the fused op must stay within
max(2 x ATen's error on the same input, 1e-6) -- the factor 2 for a different summation order, the floor so that a lucky ATen run cannot make
the test flaky.  With fp16 input the fp64 reference starts from the fp16 values, and dx (stored as fp16) gets half an fp16 ulp of its own
magnitude on top.  Every case prints both errors and, where the
environment names an output directory in GPSGS_PARITY_DIR, appends them to groupnorm_parity.jsonl there (profiles/groupnorm_shapes.md holds a copy)."""
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
from gps_gaussian_amd import _capi, accelerate as A
from gps_gaussian_amd import groupnorm as GN

pytestmark = pytest.mark.gpu
EPS = 1e-5


def _K():
    return int(_capi.lib().gn_chunk_elems())


def _shape_for_row(L):
    """[2, 2 cpg, 1, L / cpg] with G = 2: a row of exactly L elements ([2, 8, 1, L / 4] where 4 divides L)."""
    for cpg in (4, 3, 5, 7, 2, 1):
        if L % cpg == 0:
            return (2, 2 * cpg, 1, L // cpg), 2
    raise AssertionError(L)


def _cases():
    K = _K()
    c = {}
    for name, L in (("row_K-1", K - 1), ("row_K", K), ("row_K+1", K + 1), ("row_2K", 2 * K), ("row_2K+1", 2 * K + 1)):
        c[name] = _shape_for_row(L)
    for name, HW in (("plane_K-1", K - 1), ("plane_K", K), ("plane_K+1", K + 1), ("plane_2K", 2 * K), ("plane_2K+1", 2 * K + 1)):
        c[name] = ((2, 4, 1, HW), 2)                     # the backward's chunks are per (sample, channel) plane
    c["misaligned_105"] = ((2, 6, 5, 7), 2)              # 3 channels per group, 105-float rows: every second row starts off a 16-byte boundary
    c["ragged_15"] = ((1, 32, 3, 5), 8)
    c["one_element_planes"] = ((3, 8, 1, 1), 1)
    c["ref_32ch_G8"] = ((2, 32, 64, 64), 8)
    c["ref_32ch_G4"] = ((2, 32, 64, 64), 4)
    c["ref_96ch_G12"] = ((4, 96, 16, 16), 12)
    c["long_row"] = ((1, 32, 512, 512), 4)               # 2 M elements per row: the multi-hundred-chunk combine
    c["offset"] = ((2, 16, 32, 32), 2)
    return c


CASES = ["row_K-1", "row_K", "row_K+1", "row_2K", "row_2K+1", "plane_K-1", "plane_K", "plane_K+1", "plane_2K", "plane_2K+1", "misaligned_105", "ragged_15",
         "one_element_planes", "ref_32ch_G8", "ref_32ch_G4", "ref_96ch_G12", "long_row", "offset"]
FP16_CASES = ["row_K-1", "row_K+1", "row_2K+1", "plane_K+1", "misaligned_105", "ragged_15", "ref_32ch_G8", "ref_96ch_G12"]


def _weights(Cn, gen):
    w = torch.randn(Cn, generator=gen)
    b = torch.randn(Cn, generator=gen)
    w[0] = -abs(w[0]) - 0.1          # a negative one
    w[Cn // 2] = 0.0                 # and an exact zero
    return w, b


def _ref64(x, G, w, b, dy, relu=False):
    x64 = x.double().cpu().requires_grad_(True)
    w64 = w.double().cpu().requires_grad_(True)
    b64 = b.double().cpu().requires_grad_(True)
    y = F.group_norm(x64, G, w64, b64, EPS)
    if relu:
        y = F.relu(y)
    y.backward(dy.double().cpu())
    return dict(y=y.detach(), dx=x64.grad, dgamma=w64.grad, dbeta=b64.grad)


def _run(op, x, G, w, b, dy, autocast, relu=False):
    """op(x, G, w, b) on the GPU -> y, dx, dgamma, dbeta (as computed, dtypes included)."""
    xg = x.cuda().requires_grad_(True)
    wg = w.cuda().requires_grad_(True)
    bg = b.cuda().requires_grad_(True)
    with torch.autocast("cuda", torch.float16, enabled=autocast):
        y = op(xg, G, wg, bg)
        if relu:
            y = F.relu_(y)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    return dict(y=y.detach(), dx=xg.grad, dgamma=wg.grad, dbeta=bg.grad)


def _aten(x, G, w, b):
    return F.group_norm(x, G, w, b, EPS)


def _fused(x, G, w, b):
    return GN.group_norm(x, G, w, b, EPS)


@functools.lru_cache(maxsize=None)
def _case(name, half=False, relu=False):
    """Inputs, the fp64 reference and ATen's result of one case: computed once, shared by every test that needs them, never modified."""
    shape, G = _cases()[name]
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()) + int(half))
    x = torch.randn(shape, generator=gen)
    if name == "offset":
        x = 100.0 + 0.1 * x
    if half:
        x = x.half()
    w, b = _weights(shape[1], gen)
    dy = torch.randn(shape, generator=gen)
    return dict(shape=shape, G=G, x=x, w=w, b=b, dy=dy, ref=_ref64(x, G, w, b, dy, relu), aten=_run(_aten, x, G, w, b, dy, half, relu))


def _err(t, t64, half_ulp16=False):
    t, t64 = t.detach(), t64.detach()
    d = (t.double().cpu() - t64).abs()
    if half_ulp16:   # one fp16 rounding of a value of this magnitude: half a unit in the last place (subnormal spacing below 2^-14)
        ulp = torch.exp2(torch.floor(torch.log2(t64.abs().clamp_min(2.0 ** -14))) - 10)
        d = (d - 0.5 * ulp).clamp_min(0.0)
    return float(d.max() / t64.abs().max().clamp_min(1e-300))


def _report(rec):
    line = json.dumps(rec)
    print(line)
    out = os.environ.get("GPSGS_PARITY_DIR")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "groupnorm_parity.jsonl"), "a") as f:
            f.write(line + "\n")


def _check(test, name, got, c, half=False, keys=("y", "dx", "dgamma", "dbeta")):
    rec = dict(test=test, case=name, shape=list(c["shape"]), G=c["G"], x_dtype="fp16" if half else "fp32", fused={}, aten={})
    for k in keys:
        rec["fused"][k] = _err(got[k], c["ref"][k], half and k == "dx")
        rec["aten"][k] = _err(c["aten"][k], c["ref"][k], half and k == "dx")
    _report(rec)
    for k in keys:
        assert torch.isfinite(got[k]).all(), k
        assert rec["fused"][k] <= max(2.0 * rec["aten"][k], 1e-6), "%s %s: fused %.3e, ATen %.3e" % (name, k, rec["fused"][k], rec["aten"][k])
    return rec


@pytest.mark.parametrize("name", CASES)
def test_fp32_forward_and_backward_within_twice_atens_error(name):
    c = _case(name)
    got = _run(_fused, c["x"], c["G"], c["w"], c["b"], c["dy"], False)
    assert got["y"].dtype == torch.float32 and got["dx"].dtype == torch.float32 and got["y"].shape == c["shape"]
    _check("fp32", name, got, c)


def test_offset_data_keeps_the_spread():
    """mean 100, sigma 0.1: sum x^2 - (sum x)^2 / n returns noise in fp32; the {mean, M2} partials must not."""
    c = _case("offset")
    xg = c["x"].cuda().requires_grad_(True)
    y = GN.group_norm(xg, c["G"], c["w"].cuda(), c["b"].cuda(), EPS)
    saved = y.grad_fn.saved_tensors
    assert len(saved) == 4 and all(t.data_ptr() != y.data_ptr() for t in saved)      # x, mean, rstd, weight -- not the output
    mean, rstd = saved[1].double().cpu(), saved[2].double().cpu()
    N, G = c["shape"][0], c["G"]
    rows = c["x"].double().reshape(N, G, -1)
    sigma = (rows.var(dim=2, unbiased=False) + EPS).sqrt()
    rel = max((rstd * sigma - 1.0).abs().max().item(), (rstd * rows.std(dim=2, unbiased=False) - 1.0).abs().max().item())   # with and without eps
    merr = ((mean - rows.mean(dim=2)).abs() / sigma).max().item()
    _report(dict(test="offset_rstd", rstd_times_sigma_minus_1=rel, mean_error_in_sigmas=merr))
    assert rel <= 1e-3 and merr <= 1e-3


def test_a_constant_group_gives_exactly_beta_and_finite_gradients():
    shape, G = (2, 16, 48, 48), 4         # rows of 4 x 2304 = 9216 elements: two chunks each
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(shape, generator=gen)
    x[0, 4:8] = 3.25                       # sample 0, group 1
    x[1, 12:16] = -1e4                     # sample 1, group 3
    w, b = _weights(shape[1], gen)
    dy = torch.randn(shape, generator=gen)
    got = _run(_fused, x, G, w, b, dy, False)
    bb = b.cuda().view(1, -1, 1, 1).expand(shape)
    assert torch.equal(got["y"][0, 4:8], bb[0, 4:8]) and torch.equal(got["y"][1, 12:16], bb[1, 12:16])
    for k, t in got.items():
        assert torch.isfinite(t).all(), k
    ref = _ref64(x, G, w, b, dy)
    keep = torch.ones(shape, dtype=torch.bool)
    keep[0, 4:8] = False
    keep[1, 12:16] = False                 # the other groups are ordinary: still right
    assert _err(got["y"].cpu()[keep], ref["y"][keep]) <= 1e-5


@pytest.mark.parametrize("name", FP16_CASES)
def test_fp16_input_under_autocast(name):
    c = _case(name, half=True)
    shape, G = c["shape"], c["G"]
    m = nn.GroupNorm(G, shape[1], eps=EPS).cuda()
    with torch.no_grad():
        m.weight.copy_(c["w"])
        m.bias.copy_(c["b"])
    assert GN.convert(m) == 1
    n0, p0 = A.calls["groupnorm"], A.calls["groupnorm_passthrough"]
    xg = c["x"].cuda().requires_grad_(True)
    with torch.autocast("cuda", torch.float16):
        y = m(xg)
    y.backward(c["dy"].cuda())
    torch.cuda.synchronize()
    assert A.calls["groupnorm"] == n0 + 1 and A.calls["groupnorm_passthrough"] == p0
    assert y.dtype == torch.float32 and xg.grad.dtype == torch.float16
    assert c["aten"]["y"].dtype == torch.float32 and c["aten"]["dx"].dtype == torch.float16   # what ATen under autocast returns
    _check("fp16_autocast", name, dict(y=y.detach(), dx=xg.grad, dgamma=m.weight.grad, dbeta=m.bias.grad), c, half=True)
    # outside autocast an fp16 input is ATen's business (it returns fp16)
    m.half()
    out = m(c["x"].cuda())
    assert out.dtype == torch.float16 and A.calls["groupnorm_passthrough"] == p0 + 1


def test_in_place_relu_on_the_output():
    """The backward reads x, never y: the consumer may overwrite y (the reference applies nn.ReLU(inplace=True) to it)."""
    c = _case("ref_32ch_G8", relu=True)
    got = _run(_fused, c["x"], c["G"], c["w"], c["b"], c["dy"], False, relu=True)
    _check("relu_", "ref_32ch_G8", got, c)


def test_gradient_subsets_and_no_grad():
    c = _case("ref_32ch_G4")
    full = _run(_fused, c["x"], c["G"], c["w"], c["b"], c["dy"], False)
    x, w, b, dy = c["x"].cuda(), c["w"].cuda(), c["b"].cuda(), c["dy"].cuda()
    # only x
    xg = x.clone().requires_grad_(True)
    y = GN.group_norm(xg, c["G"], w, b, EPS)
    y.backward(dy)
    assert torch.equal(y.detach(), full["y"]) and torch.equal(xg.grad, full["dx"])
    # only the weights
    wg, bg = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = GN.group_norm(x, c["G"], wg, bg, EPS)
    y.backward(dy)
    assert torch.equal(wg.grad, full["dgamma"]) and torch.equal(bg.grad, full["dbeta"])
    # only the bias
    bg = b.clone().requires_grad_(True)
    GN.group_norm(x, c["G"], w, bg, EPS).backward(dy)
    assert torch.equal(bg.grad, full["dbeta"])
    # no_grad: nothing kept, the same bits
    with torch.no_grad():
        y0 = GN.group_norm(x.clone().requires_grad_(True), c["G"], wg, bg, EPS)
    assert y0.grad_fn is None and not y0.requires_grad and torch.equal(y0, full["y"])
    y1 = GN.group_norm(x, c["G"], w, b, EPS)             # nothing requires grad
    assert y1.grad_fn is None and torch.equal(y1, full["y"])


@pytest.mark.parametrize("name,half", [("ref_32ch_G4", False), ("row_2K+1", False), ("misaligned_105", True)])
def test_two_runs_give_the_same_bits(name, half):
    c = _case(name, half=half)
    a = _run(_fused, c["x"], c["G"], c["w"], c["b"], c["dy"], half)
    b = _run(_fused, c["x"], c["G"], c["w"], c["b"], c["dy"], half)
    for k in a:
        assert torch.equal(a[k], b[k]), k


class _StandIn(nn.Module):
    """Conv -> GroupNorm -> in-place ReLU, twice through ONE shared norm, a third norm, and a residual add (written for this test)."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 16, 3, padding=1)
        self.conv2 = nn.Conv2d(16, 16, 3, padding=1)
        self.conv3 = nn.Conv2d(16, 16, 1)
        self.shared = nn.GroupNorm(2, 16)
        self.last = nn.GroupNorm(4, 16)
        self.relu = nn.ReLU(inplace=True)
        self.again = nn.Sequential(self.conv2, self.shared)      # a second parent of the shared norm

    def forward(self, x):
        y = self.relu(self.shared(self.conv1(x)))
        z = self.relu(self.again(y))
        return self.relu(self.last(self.conv3(z)) + y)


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast"])
def test_stand_in_network(autocast):
    torch.manual_seed(21)
    base = _StandIn()
    with torch.no_grad():
        for m in (base.shared, base.last):
            m.weight.normal_()
            m.bias.normal_()
    x = torch.randn(2, 3, 40, 36)                         # rows of 8 x 1440 = 11,520 elements: two chunks, the second ragged
    g = torch.randn(2, 16, 40, 36)
    ref = copy.deepcopy(base).double()
    out64 = ref(x.double())
    out64.backward(g.double())
    aten, fused = copy.deepcopy(base).cuda(), copy.deepcopy(base).cuda()
    assert GN.convert(fused) == 2 and fused.again[1] is fused.shared
    n0, p0 = A.calls["groupnorm"], A.calls["groupnorm_passthrough"]
    res = {}
    for tag, net in (("aten", aten), ("fused", fused)):
        with torch.autocast("cuda", torch.float16, enabled=autocast):
            out = net(x.cuda())
        out.backward(g.cuda())
        torch.cuda.synchronize()
        res[tag] = [out.detach()] + [p.grad for p in net.parameters()]
    assert A.calls["groupnorm"] == n0 + 3 and A.calls["groupnorm_passthrough"] == p0
    names = ["out"] + [n for n, _ in base.named_parameters()]
    refs = [out64.detach()] + [p.grad for p in ref.parameters()]
    rec = dict(test="stand_in", autocast=autocast, fused={}, aten={})
    for n, t64, ta, tf in zip(names, refs, res["aten"], res["fused"]):
        rec["aten"][n], rec["fused"][n] = _err(ta, t64), _err(tf, t64)
    _report(rec)
    for n in names:
        assert rec["fused"][n] <= max(2.0 * rec["aten"][n], 1e-3), "%s: fused %.3e, ATen %.3e" % (n, rec["fused"][n], rec["aten"][n])


def test_channels_last_and_bf16_go_through_aten():
    torch.manual_seed(8)
    plain = nn.GroupNorm(4, 16).cuda()
    with torch.no_grad():
        plain.weight.normal_()
        plain.bias.normal_()
    fused = copy.deepcopy(plain)
    assert GN.convert(fused) == 1
    x = torch.randn(2, 16, 12, 10, device="cuda")
    n0, p0 = A.calls["groupnorm"], A.calls["groupnorm_passthrough"]
    cl = x.to(memory_format=torch.channels_last)
    a, b = plain(cl), fused(cl)
    assert torch.equal(a, b) and a.stride() == b.stride()
    xb = x.bfloat16()
    pb, fb = copy.deepcopy(plain).bfloat16(), copy.deepcopy(fused).bfloat16()
    a, b = pb(xb), fb(xb)
    assert b.dtype == torch.bfloat16 and torch.equal(a, b)
    assert A.calls["groupnorm_passthrough"] == p0 + 2 and A.calls["groupnorm"] == n0
    # a permuted (not channels-last) view is made contiguous and fused
    xt = x.transpose(2, 3)
    assert not xt.is_contiguous()
    got = fused(xt)
    assert A.calls["groupnorm"] == n0 + 1
    want = F.group_norm(xt.double().cpu(), 4, plain.weight.double().cpu(), plain.bias.double().cpu(), plain.eps)
    assert _err(got, want) <= 1e-5
