"""GPU (-m gpu): the fused Gaussian-head kernels (csrc/gshead.hip; gshead.head / FusedHeadConv) against the NumPy fp64 restatement of
gshead_ref.py, under the bounds derived there, on the inputs defined there (test_gshead_ref.py shows on the CPU that those bounds are reachable
and that nine single-error mutants leave them on the same inputs).  Every case prints its worst error / bound per output.

The reference is fp64 on the CPU everywhere, also for the converted Sequential.  ATen's convolution runs on the GPU in one place only, because that
is what the test there is about: the pass-through of a FusedHeadConv (forward only, under no_grad, on the smallest case)."""
import copy
import functools

import numpy as np
import pytest
import torch
from torch import nn

import gps_gaussian_amd  # noqa: F401
from gps_gaussian_amd import _capi, accelerate as A
from gps_gaussian_amd import gshead as GH

import convop_run
import gshead_ref as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _tile():
    return int(_capi.lib().gsr_head_tile())


CASES = sorted(R.cases(1024))     # the names do not depend on the tile (test_gshead_ref.py checks that)


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs, the fp64 reference and the bounds of one case: computed once, shared by every test that needs them, never modified."""
    c = R.make_case(name, _tile())
    args = (c["h"], c["w"], c["b"], c["dy"], c["act"], c["beta"], c["threshold"])
    return c, R.reference(*args), R.bounds(*args)


def _run(c, need=("h", "w", "b"), op=None):
    """The op on the GPU -> dict of y, dh, dw, db as NumPy arrays (None where no gradient was asked for)."""
    t = {k: torch.from_numpy(c[k]).cuda().requires_grad_(k in need) for k in ("h", "w", "b")}
    op = op or (lambda h, w, b: GH.head(h, w, b, c["act"], c["beta"], c["threshold"]))
    y = op(t["h"], t["w"], t["b"])
    if need:
        y.backward(torch.from_numpy(c["dy"]).cuda())
    torch.cuda.synchronize()
    out = dict(y=y.detach(), dh=t["h"].grad, dw=t["w"].grad, db=t["b"].grad)
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


def _check(name, got, ref, bnd, keys=R.KEYS):
    convop_run.check(dict(case=name), "error_over_bound", got, ref, bnd, keys=keys, ratio=R.worst_ratio)


@pytest.mark.parametrize("name", CASES)
def test_forward_and_backward_within_the_bounds(name):
    c, ref, bnd = _case(name)
    got = _run(c)
    _check(name, got, ref, bnd)
    assert (got["dh"][c["h"] == 0] == 0).all()                       # the gradient is exactly zero where h == 0 ...
    assert (got["dh"][c["h"] < 0] == 0).all()                        # ... and where h < 0
    N, C, H, W = c["h"].shape
    y0 = got["y"][:, 0].reshape(N, -1)
    spots = {what: y0[n, p] for what, n, p in c["planted"]}
    if c["act"] == "none":
        assert spots["all_negative"] == c["b"][0]                      # z = b: no product contributes
    if c["act"] == "sigmoid":
        assert 0.0 <= spots["z=-90"] <= 1e-38 and spots["z=+90"] == 1.0 and (got["y"] >= 0).all() and (got["y"] <= 1).all()
    if c["act"] == "softplus":
        assert spots["beta_z=-200"] == 0.0 and (got["y"] >= 0).all()


def _ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


@pytest.mark.parametrize("which", ["2x32x5x7_k4", "1x32x1x(2T+5)_k3", "2x16x8x12_k1", "1x64x1x(T+8)_k2", "65x16x1x8_k4"])
def test_small_integers_give_the_exact_answer(which):
    """h in [-3, 3], w, b, dy in [-2, 2], no activation: every product and partial sum is an integer far below 2^24 (|z| <= 2 + 64 * 6, the largest
    weight sum 65 * 8 * 6 or (2T + 5) * 6), so y, dh, dw, db must EQUAL the fp64 result bit for bit, whatever the order of the sums."""
    T = _tile()
    N, C, H, W, K = {"2x32x5x7_k4": (2, 32, 5, 7, 4), "1x32x1x(2T+5)_k3": (1, 32, 1, 2 * T + 5, 3), "2x16x8x12_k1": (2, 16, 8, 12, 1),
                     "1x64x1x(T+8)_k2": (1, 64, 1, T + 8, 2), "65x16x1x8_k4": (65, 16, 1, 8, 4)}[which]
    rng = np.random.default_rng(len(which) + N)
    c = dict(h=_ints(rng, (N, C, H, W), -3, 3), w=_ints(rng, (K, C), -2, 2), b=_ints(rng, (K,), -2, 2), dy=_ints(rng, (N, K, H, W), -2, 2),
             act="none", beta=1.0, threshold=20.0)
    assert (2 * T + 5) * 6 < 2 ** 24
    ref = R.reference(c["h"], c["w"], c["b"], c["dy"])
    got = _run(c)
    for k in R.KEYS:
        assert np.array_equal(got[k].astype(np.float64), ref[k]), k


def test_two_runs_give_the_same_bits():
    names = ("multi_5T+3_k4_softplus", "c64_2x64x17x64_k4_sigmoid", "parts_65_k2_none")
    convop_run.two_runs(_run, [(name, _case(name)[0]) for name in names], keys=R.KEYS)


def test_only_the_gradients_asked_for_are_computed(monkeypatch):
    c, ref, bnd = _case("multi_5T+4_k4_sigmoid")
    full = _run(c)
    seen = []
    real = GH.call

    def spy(name, dev, *args):
        if name == "gsr_head_backward":
            seen.append(dict(dh=args[-4] is not None, dw=args[-3] is not None, db=args[-2] is not None, scratch=args[-1] is not None))
        return real(name, dev, *args)

    monkeypatch.setattr(GH, "call", spy)
    only_x = _run(c, need=("h",))
    assert seen[-1] == dict(dh=True, dw=False, db=False, scratch=False)
    assert only_x["dw"] is None and only_x["db"] is None and np.array_equal(only_x["dh"], full["dh"]) and np.array_equal(only_x["y"], full["y"])
    params = _run(c, need=("w", "b"))
    assert seen[-1] == dict(dh=False, dw=True, db=True, scratch=True)          # the input gradient was not asked of the kernel
    assert params["dh"] is None and np.array_equal(params["dw"], full["dw"]) and np.array_equal(params["db"], full["db"])
    only_b = _run(c, need=("b",))
    assert seen[-1] == dict(dh=False, dw=True, db=True, scratch=True)          # dw and db are written both or neither
    assert only_b["dw"] is None and only_b["dh"] is None and np.array_equal(only_b["db"], full["db"])
    n = len(seen)
    nothing = _run(c, need=())
    assert len(seen) == n and np.array_equal(nothing["y"], full["y"])           # no backward at all


def _chain(c):
    """Conv3x3 -> ReLU(inplace) -> Conv1x1 -> activation, as the reference builds a head, with the case's 1x1 weights."""
    K, C = c["w"].shape
    act = {"none": [], "softplus": [nn.Softplus(beta=c["beta"], threshold=c["threshold"])], "sigmoid": [nn.Sigmoid()]}[c["act"]]
    torch.manual_seed(5)
    net = nn.Sequential(nn.Conv2d(C, C, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(C, K, 1), *act)
    with torch.no_grad():
        net[2].weight.copy_(torch.from_numpy(c["w"]).reshape(K, C, 1, 1))
        net[2].bias.copy_(torch.from_numpy(c["b"]))
    return net


def test_what_the_op_does_not_take_goes_through_torch_and_agrees():
    """A channels-last and a strided input: the converted convolution computes the same function with torch.relu / conv / activation, counts it,
    and the result agrees with the fused one within the bounds (both are held to the fp64 reference)."""
    name = "tiny_2x32x5x7_k3_softplus"
    c, ref, bnd = _case(name)
    K, C = c["w"].shape
    m = nn.Sequential(nn.ReLU(), nn.Conv2d(C, K, 1), nn.Softplus(beta=c["beta"], threshold=c["threshold"])).cuda()
    with torch.no_grad():
        m[1].weight.copy_(torch.from_numpy(c["w"]).reshape(K, C, 1, 1))
        m[1].bias.copy_(torch.from_numpy(c["b"]))
    assert GH.convert(m) == 1 and [type(l) for l in m] == [nn.Identity, GH.FusedHeadConv, nn.Identity]
    h = torch.from_numpy(c["h"]).cuda()
    for tag, x in (("channels_last", h.to(memory_format=torch.channels_last)), ("strided", torch.cat([h, h], dim=1)[:, :C])):
        assert not x.is_contiguous()
        n0, p0 = A.calls["gshead"], A.calls["gshead_passthrough"]
        with torch.no_grad():
            y = m(x)
        torch.cuda.synchronize()
        assert A.calls["gshead"] == n0 and A.calls["gshead_passthrough"] == p0 + 1
        _check(name + ":" + tag, dict(y=y.contiguous().cpu().numpy()), ref, bnd, keys=("y",))
    n0, p0 = A.calls["gshead"], A.calls["gshead_passthrough"]
    with torch.no_grad():
        y = m(h)
    assert A.calls["gshead"] == n0 + 1 and A.calls["gshead_passthrough"] == p0
    _check(name + ":fused", dict(y=y.cpu().numpy()), ref, bnd, keys=("y",))


@pytest.mark.parametrize("name", ["tiny_2x32x5x7_k3_softplus", "T-1_k1_sigmoid", "T_k4_none"])
def test_a_converted_sequential_matches_the_fp64_module(name):
    """The three head shapes.  The unconverted chain runs on the CPU in fp64; the converted one on the GPU with its 3x3 convolution replaced by the
    fp64 module's output rounded to fp32 (so that ATen's convolution does not run on the GPU and both tails start from the same h): what is compared
    is everything from the ReLU on, under the bounds of the op for that h."""
    c, _, _ = _case(name)
    base = _chain(c)
    ref64 = copy.deepcopy(base).double()
    x = torch.randn(c["h"].shape, generator=torch.Generator().manual_seed(9)).double()
    with torch.no_grad():
        h32 = ref64[0](x).float()                                      # the hidden tensor, fp32 values
    tail64 = ref64[1:]
    h64 = h32.double().requires_grad_(True)
    y64 = tail64(h64.clone())                                          # (the ReLU is in place)
    dy = torch.from_numpy(c["dy"])
    y64.backward(dy.double())
    fused = copy.deepcopy(base)
    assert GH.convert(fused) == 1
    assert [type(l) for l in fused][1:3] == [nn.Identity, GH.FusedHeadConv] and list(fused.state_dict()) == list(base.state_dict())
    tail = fused[1:].cuda()
    n0 = A.calls["gshead"]
    hg = h32.cuda().requires_grad_(True)
    y = tail(hg)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    assert A.calls["gshead"] == n0 + 1
    cc = dict(c, h=h32.numpy())
    bnd = R.bounds(cc["h"], cc["w"], cc["b"], cc["dy"], cc["act"], cc["beta"], cc["threshold"])
    ref = dict(y=y64.detach().numpy(), dh=h64.grad.numpy(), dw=tail64[1].weight.grad.numpy().reshape(c["w"].shape), db=tail64[1].bias.grad.numpy())
    got = dict(y=y.detach().cpu().numpy(), dh=hg.grad.cpu().numpy(), dw=tail[1].weight.grad.cpu().numpy().reshape(c["w"].shape),
               db=tail[1].bias.grad.cpu().numpy())
    _check(name + ":sequential", got, ref, bnd)


def test_head_refuses_what_it_does_not_implement():
    h = torch.randn(1, 24, 4, 4, device="cuda")
    with pytest.raises(RuntimeError):
        GH.head(h, torch.randn(3, 24, device="cuda"), torch.randn(3, device="cuda"))
    h = torch.randn(1, 32, 4, 4, device="cuda")
    with pytest.raises(RuntimeError):
        GH.head(h, torch.randn(5, 32, device="cuda"), torch.randn(5, device="cuda"))
    with pytest.raises(RuntimeError):
        GH.head(h, torch.randn(3, 32, device="cuda"), torch.randn(3, device="cuda"), act="softplus", beta=0.0)
    with pytest.raises(RuntimeError):
        GH.head(h.half(), torch.randn(3, 32, device="cuda"), torch.randn(3, device="cuda"))
