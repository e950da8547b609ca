"""GPU (-m gpu): the GroupNorm kernels with the ReLU / residual add + ReLU epilogue fused in (csrc/group_norm.hip EP_RELU, EP_RELU_ADD_RELU;
groupnorm.group_norm(relu=True[, residual=r]), FusedGroupNorm.forward_relu, residual_block_forward, fuse_sequential_relu).

Two yardsticks:
  * BITS against the composition of the plain op on the same device: relu_(group_norm(x)) and relu(res + relu_(group_norm(x))).  Exact by
    construction -- the same stored value, the mask of ATen's threshold_backward, the same summation order -- so out, dx, dgamma, dbeta, dres are
    compared with torch.equal.
  * fp64 on the CPU, independently, with ATen's eager composition on the GPU as the yardstick for the error: the fused result must stay within
    max(2 x ATen's error, 1e-6) (half an fp16 ulp on top for an fp16 dx), as in tests/test_gpu_groupnorm.py; out, dx, dres are compared outside the
    guard band of tests/gn_epilogue_cases.py, whose share is capped.  Each such case prints its numbers and appends them to groupnorm_parity.jsonl
    where GPSGS_PARITY_DIR names a directory (profiles/groupnorm_epilogue.md holds a copy)."""
import copy
import functools
import json
import os

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import gps_gaussian_amd  # noqa: F401
from gps_gaussian_amd import accelerate as A
from gps_gaussian_amd import groupnorm as GN

import gn_epilogue_cases as E

pytestmark = pytest.mark.gpu
KEYS = ("out", "dx", "dgamma", "dbeta", "dres")


def _run(kind, c, form, *, grads=("x", "w", "b", "res"), backward=True):
    """kind: 'fused' (one node), 'composed' (the plain fused op + relu_ / add / relu: what the parent commit runs) or 'aten' (eager F.group_norm + the
    same).  fp16 cases run under fp16 autocast through a module, as the networks do; fp32 ones through the functional op.  -> dict of KEYS."""
    half = c["half"]
    xg = c["x"].cuda().requires_grad_("x" in grads)
    wg = c["w"].cuda().requires_grad_("w" in grads)
    bg = c["b"].cuda().requires_grad_("b" in grads)
    rg = c["res"].cuda().requires_grad_("res" in grads) if form == "relu_add_relu" else None
    if half:
        m = nn.GroupNorm(c["G"], c["shape"][1], eps=E.EPS).cuda()
        m.weight, m.bias = nn.Parameter(wg.detach(), requires_grad="w" in grads), nn.Parameter(bg.detach(), requires_grad="b" in grads)
        wg, bg = m.weight, m.bias
        if kind != "aten":
            GN.convert(m)
    with torch.autocast("cuda", torch.float16, enabled=half):
        if kind == "fused":
            out = m.forward_relu(xg, rg) if half else GN.group_norm(xg, c["G"], wg, bg, E.EPS, relu=True, residual=rg)
        else:
            y = m(xg) if half else (GN.group_norm if kind == "composed" else F.group_norm)(xg, c["G"], wg, bg, E.EPS)
            out = torch.relu_(y)
            if rg is not None:
                out = torch.relu(rg + out)
    if grads and backward:
        out.backward(c["dout"].cuda())
    torch.cuda.synchronize()
    return dict(out=out.detach(), dx=xg.grad, dgamma=wg.grad, dbeta=bg.grad, dres=rg.grad if rg is not None else None, node=out)


def _same_bits(a, b, what):
    for k in KEYS:
        assert (a[k] is None) == (b[k] is None), (what, k)
        if a[k] is not None:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), "%s: %s differs in %d elements" % (what, k, int((a[k] != b[k]).sum()))


@pytest.mark.parametrize("form", E.FORMS)
@pytest.mark.parametrize("name", E.NAMES)
def test_fp32_bits_of_the_composition(name, form):
    c = E.inputs(name)
    fused = _run("fused", c, form)
    assert fused["out"].dtype == torch.float32 and fused["out"].shape == c["shape"] and float(fused["out"].min()) >= 0.0
    assert fused["dx"] is not None and (fused["dres"] is not None) == (form == "relu_add_relu")
    _same_bits(fused, _run("composed", c, form), "%s %s" % (name, form))


@pytest.mark.parametrize("form", E.FORMS)
@pytest.mark.parametrize("name", E.FP16_NAMES)
def test_fp16_autocast_bits_of_the_composition(name, form):
    c = E.inputs(name, True)
    n0, p0 = A.calls["groupnorm"], A.calls["groupnorm_passthrough"]
    fused = _run("fused", c, form)
    assert A.calls["groupnorm"] == n0 + 1 and A.calls["groupnorm_passthrough"] == p0
    assert fused["out"].dtype == torch.float32 and fused["dx"].dtype == torch.float16
    _same_bits(fused, _run("composed", c, form), "%s %s fp16" % (name, form))


@pytest.mark.parametrize("form", E.FORMS)
def test_a_constant_group_with_y_exactly_zero_positive_and_negative(form):
    """x constant over a group: y is exactly beta there.  beta = 0, +1, -1 puts y on the kink and on either side of it: out is 0, 1, 0 in the relu form,
    the gradient of the y = 0 channel is masked (threshold_backward: y <= 0), and everything still has the composition's bits."""
    shape, G = (2, 16, 48, 48), 4         # rows of 4 x 2304 = 9216 elements: two chunks each
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(shape, generator=gen)
    x[0, 4:8] = 3.25                       # sample 0, group 1
    w, b = torch.randn(16, generator=gen), torch.randn(16, generator=gen)
    b[4], b[5], b[6] = 0.0, 1.0, -1.0
    c = dict(shape=shape, G=G, half=False, x=x, w=w, b=b, res=torch.randn(shape, generator=gen), dout=torch.randn(shape, generator=gen))
    fused = _run("fused", c, form)
    _same_bits(fused, _run("composed", c, form), "constant group %s" % form)
    for k in KEYS:
        assert fused[k] is None or torch.isfinite(fused[k]).all(), k
    if form == "relu":
        o = fused["out"][0]
        assert float(o[4].abs().max()) == 0.0 and torch.equal(o[5], torch.ones_like(o[5])) and float(o[6].abs().max()) == 0.0
    else:
        r = c["res"].cuda()[0]
        assert torch.equal(fused["out"][0, 4], torch.relu(r[4])) and torch.equal(fused["out"][0, 5], torch.relu(r[5] + 1.0))
        # dres is the outer-masked gradient, +0.0 where masked
        want = torch.where(fused["out"] > 0, c["dout"].cuda(), torch.zeros((), device="cuda"))
        assert torch.equal(fused["dres"], want) and not torch.signbit(fused["dres"][fused["out"] <= 0]).any()


def _err(t, t64, keep=None, half_ulp16=False):
    d = (t.detach().double().cpu() - t64).abs()
    if half_ulp16:   # one fp16 rounding of a value of this magnitude: half a unit in the last place (subnormal spacing below 2^-14)
        ulp = torch.exp2(torch.floor(torch.log2(t64.abs().clamp_min(2.0 ** -14))) - 10)
        d = (d - 0.5 * ulp).clamp_min(0.0)
    if keep is not None:
        d = d[keep]
    return float(d.max() / t64.abs().max().clamp_min(1e-300))


def _report(rec):
    line = json.dumps(rec)
    print(line)
    out = os.environ.get("GPSGS_PARITY_DIR")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "groupnorm_parity.jsonl"), "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("name,form,half", [(n, f, False) for n in ("ref_32ch_G8", "plane_2K+1", "misaligned_105") for f in E.FORMS] +
                         [("ref_32ch_G8", f, True) for f in E.FORMS])
def test_against_fp64_within_twice_atens_error(name, form, half):
    c, ref = E.inputs(name, half), E.ref64(name, form, half)
    assert ref["excluded_share"] <= E.SHARE_CAP
    fused, aten = _run("fused", c, form), _run("aten", c, form)
    rec = dict(test="epilogue_" + form, case=name, shape=list(c["shape"]), G=c["G"], x_dtype="fp16" if half else "fp32",
               excluded_share=ref["excluded_share"], fused={}, aten={})
    keys = [k for k in KEYS if ref[k] is not None]
    for k in keys:
        keep = ref["keep"] if k in ("out", "dx", "dres") else None
        rec["fused"][k] = _err(fused[k], ref[k], keep, half and k == "dx")
        rec["aten"][k] = _err(aten[k], ref[k], keep, half and k == "dx")
    _report(rec)
    for k in keys:
        assert torch.isfinite(fused[k]).all(), k
        assert rec["fused"][k] <= max(2.0 * rec["aten"][k], 1e-6), "%s %s %s: fused %.3e, ATen %.3e" % (name, form, k, rec["fused"][k], rec["aten"][k])


def test_the_relu_node_saves_nothing_that_aliases_its_output():
    c = E.inputs("ref_96ch_G12")
    x, w, b, r = c["x"].cuda().requires_grad_(True), c["w"].cuda(), c["b"].cuda(), c["res"].cuda()
    out = GN.group_norm(x, c["G"], w, b, E.EPS, relu=True)
    saved = out.grad_fn.saved_tensors
    assert len(saved) == 5 and all(t.data_ptr() != out.data_ptr() for t in saved)          # x, mean, rstd, weight, bias
    assert sum(t.numel() == x.numel() for t in saved) == 1                                  # one activation-sized tensor: x
    out2 = GN.group_norm(x, c["G"], w, b, E.EPS, relu=True, residual=r)
    saved2 = out2.grad_fn.saved_tensors
    assert len(saved2) == 6 and sum(t.data_ptr() == out2.data_ptr() for t in saved2) == 1   # ... and the output, for the outer sign
    assert sum(t.numel() == x.numel() for t in saved2) == 2                                 # never the residual, never a normalised activation


@functools.lru_cache(maxsize=None)
def _full(form):
    return _run("fused", E.inputs("ref_96ch_G12"), form)


@pytest.mark.parametrize("form", E.FORMS)
def test_gradient_subsets_no_grad_and_repeatability(form):
    c, full = E.inputs("ref_96ch_G12"), _full(form)
    only_x = _run("fused", c, form, grads=("x",))
    assert torch.equal(only_x["out"], full["out"]) and torch.equal(only_x["dx"], full["dx"])
    assert only_x["dgamma"] is None and only_x["dbeta"] is None and only_x["dres"] is None
    only_w = _run("fused", c, form, grads=("w", "b"))
    assert only_w["dx"] is None and torch.equal(only_w["dgamma"], full["dgamma"]) and torch.equal(only_w["dbeta"], full["dbeta"])
    if form == "relu_add_relu":
        only_r = _run("fused", c, form, grads=("res",))
        assert only_r["dx"] is None and only_r["dgamma"] is None and torch.equal(only_r["dres"], full["dres"])
    with torch.no_grad():
        quiet = _run("fused", c, form, backward=False)      # inputs that require grad, under no_grad: nothing kept, the same bits
    assert quiet["node"].grad_fn is None and not quiet["node"].requires_grad and torch.equal(quiet["out"], full["out"])
    nothing = _run("fused", c, form, grads=())               # nothing requires grad
    assert nothing["node"].grad_fn is None and torch.equal(nothing["out"], full["out"])
    _same_bits(_run("fused", c, form), full, "second run")


def test_two_runs_give_the_same_bits_across_chunks_and_in_fp16():
    for name, half in (("row_2K+1", False), ("misaligned_105", True)):
        c = E.inputs(name, half)
        _same_bits(_run("fused", c, "relu_add_relu"), _run("fused", c, "relu_add_relu"), name)


def test_bad_residuals_raise():
    c = E.inputs("ragged_15")
    x, w, b = c["x"].cuda(), c["w"].cuda(), c["b"].cuda()
    with pytest.raises(RuntimeError, match="residual"):
        GN.group_norm(x, c["G"], w, b, E.EPS, relu=True, residual=c["res"])                  # on the CPU
    with pytest.raises(RuntimeError, match="relu=True"):
        GN.group_norm(x, c["G"], w, b, E.EPS, residual=c["res"].cuda())
    with pytest.raises(RuntimeError, match="residual"):
        GN.group_norm(x, c["G"], w, b, E.EPS, relu=True, residual=c["res"].cuda().half())
    with pytest.raises(RuntimeError, match="residual"):
        GN.group_norm(x, c["G"], w, b, E.EPS, relu=True, residual=c["res"].cuda()[:, :1])


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast"])
def test_stand_in_block(autocast):
    base, x, g = E.stand_in()
    ref = copy.deepcopy(base).double()
    out64 = ref(x.double())
    out64.backward(g.double())
    aten, own, fused = copy.deepcopy(base).cuda(), copy.deepcopy(base).cuda(), copy.deepcopy(base).cuda()
    assert GN.convert(own) == 4                               # the parent commit's path: fused norms, the block's own forward
    assert GN.convert(fused) == 4 and GN.fuse_sequential_relu(fused) == 1
    fused.fused_forward = True
    res = {}
    for tag, net in (("aten", aten), ("own", own), ("fused", fused)):
        n0, p0, r0 = A.calls["groupnorm"], A.calls["groupnorm_passthrough"], A.calls["resblock"]
        with torch.autocast("cuda", torch.float16, enabled=autocast):
            out = net(x.cuda())
        out.backward(g.cuda())
        torch.cuda.synchronize()
        res[tag] = [out.detach()] + [p.grad for p in net.parameters()]
        want = 0 if tag == "aten" else 4                      # stem, norm1, norm2, norm3: the kernels were reached, nothing handed on
        assert A.calls["groupnorm"] == n0 + want and A.calls["groupnorm_passthrough"] == p0
        assert A.calls["resblock"] == r0 + (tag == "fused")
    if not autocast:
        assert torch.equal(res["fused"][0], res["own"][0])    # the bits of the block's own forward on the converted norms
    names = ["out"] + [n for n, _ in base.named_parameters()]
    refs = [out64.detach()] + [p.grad for p in ref.parameters()]
    rec = dict(test="epilogue_stand_in", autocast=autocast, fused={}, aten={})
    for n, t64, ta, tf in zip(names, refs, res["aten"], res["fused"]):
        rec["aten"][n], rec["fused"][n] = _err(ta, t64), _err(tf, t64)
    _report(rec)
    for n in names:
        assert rec["fused"][n] <= max(2.0 * rec["aten"][n], 1e-3), "%s: fused %.3e, ATen %.3e" % (n, rec["fused"][n], rec["aten"][n])
