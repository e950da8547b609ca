"""GPU (-m gpu): the 3x3 matrix-core convolution (csrc/conv3x3.hip; conv3x3.conv3x3 / FusedConv3x3) against F.conv2d (+ relu) and its autograd in
fp64 on the CPU, starting from the same fp32 inputs.  No ATen convolution on the GPU serves as a reference or runs a backward in this file
(test_gpu_stemconv.py records a fault inside the library's solver search); only the pass-through cases run ATen's forward there, and they compare
the converted module with the plain one, which is the same ATen call twice.

The bounds are derived, not measured, and hold for any summation order.  With u = 2^-24 and g(n) = n u / (1 - n u), elementwise:
    y        |y - y64| <= g(9 C_in + 1) (sum |w||x| + |b|)  =: B       (ReLU is 1-Lipschitz: the same bound with it)
    dx       <= g(9 * 32) sum |w||g|
    dw, db   <= g(N H W) sum |g||x|,  g(N H W) sum |g|
with g = dy, or dy [z64 > 0] for the ReLU form; the sums of absolute values come from the same fp64 convolution (and its autograd) applied to
|x|, |w|, |b|, |g|.  Every ReLU case first asserts that no pre-activation z64 lies within its own B of zero, so the fp32 mask must be the
reference's: no error is excused by a flipped mask."""
import copy
import functools
import json

import pytest
import torch
from torch import nn

import gps_gaussian_amd  # noqa: F401
from gps_gaussian_amd import accelerate as A
from gps_gaussian_amd import conv3x3 as C3
from gps_gaussian_amd import gshead as GH

import convop_run as R
from convop_run import gamma

pytestmark = pytest.mark.gpu
CO = 32


@pytest.fixture(scope="module", autouse=True)
def _counters():
    A.counters("conv3x3")
    yield
    A.restore()      # the process's counter keys are what they were


_tile = C3.tile


@functools.lru_cache(maxsize=None)
def _cases():
    """name -> (N, C_in, H, W, relu)"""
    TH, TW = _tile()
    c = {}
    for tag, hw in (("T-1", (TH - 1, TW - 1)), ("T", (TH, TW)), ("T+1", (TH + 1, TW + 1)), ("2T+1_T-1", (2 * TH + 1, TW - 1)), ("1_2T+1", (1, 2 * TW + 1))):
        c["tile_%s_52_relu" % tag] = (2, 52) + hw + (True,)
        c["tile_%s_32" % tag] = (2, 32) + hw + (False,)
    c["one_pixel"] = (1, 4, 1, 1, False)                   # every tap but the centre is padding
    c["tiny_3x8x2x3"] = (3, 8, 2, 3, True)
    c["ragged_37x41"] = (1, 52, 37, 41, True)              # rows start off 16-byte boundaries
    for ci in (4, 36, 64):
        c["cin_%d" % ci] = (2, ci, 33, 65, ci != 36)
    c["ref_52_128"] = (1, 52, 128, 128, True)
    c["ref_32_64x130"] = (2, 32, 64, 130, False)
    return c


TILE_TAGS = ["T-1", "T", "T+1", "2T+1_T-1", "1_2T+1"]
CASES = ["tile_%s_%s" % (t, k) for t in TILE_TAGS for k in ("52_relu", "32")] + \
        ["one_pixel", "tiny_3x8x2x3", "ragged_37x41", "cin_4", "cin_36", "cin_64", "ref_52_128", "ref_32_64x130"]


def _bounds(ref, N, Ci, H, W, relu):
    return dict(y=gamma(9 * Ci + 1) * ref["abs_y"], dx=gamma(9 * CO) * ref["abs_dx"], dw=gamma(N * H * W) * ref["abs_dw"],
                db=gamma(N * H * W) * ref["abs_db"])


def _assert_no_preactivation_near_zero(c):
    """The ReLU cases: |z64| > B everywhere, so the sign of the fp32 pre-activation is the reference's (the inputs of _inputs() are built so)."""
    if c["conv"]["relu"]:
        margin = (c["ref"]["z"].abs() - c["bounds"]["y"]).min()
        assert margin > 0, "a pre-activation lies within its bound of zero: %.3e" % float(margin)


def _inputs(gen, N, Ci, H, W, relu):
    """Seeded random inputs.  Without ReLU: normal x, w (x 0.2), b, dy.  With ReLU no plain random tensor of these sizes keeps every pre-activation
    further than B ~ 4e-4 sigma(z) from zero, so the pre-activations sit near a lattice that misses zero: x = (multiples of 1/2) + d with
    |d| <= 2^-12 at full fp32 precision, w multiples of 1/16, b ODD multiples of 1/64 -- sum w x_lattice is a multiple of 1/32, so |z| >= 1/64 less
    the d terms (sigma ~ 1e-3), against B ~ 2e-3.  The x still carry full mantissas, so every product and sum rounds; dy is plain normal."""
    x = torch.randn((N, Ci, H, W), generator=gen)
    w = torch.randn((CO, Ci, 3, 3), generator=gen) * 0.2
    b = torch.randn((CO,), generator=gen)
    if relu:
        x = torch.round(x * 2) / 2 + (torch.rand(x.shape, generator=gen) - 0.5) * 2.0 ** -11
        w = torch.round(w * 16) / 16
        b = (2 * torch.randint(-64, 64, (CO,), generator=gen) + 1).float() / 64
    w[CO // 2] = 0.0                    # one exact-zero filter (its bias decides the sign)
    w[0] = -w[0].abs() - 1.0 / 16       # and a negative one
    dy = torch.randn((N, CO, H, W), generator=gen)
    return dict(x=x, w=w, b=b, dy=dy, conv=dict(padding=1, relu=relu))


_case = R.case_cache(_cases, _inputs, _bounds)


def _op(relu):
    return lambda x, w, b: C3.conv3x3(x, w, b, relu)


def _run(c):
    return R.run_case(_op(c["conv"]["relu"]), c)


@pytest.mark.parametrize("name", CASES)
def test_forward_and_backward_within_the_bounds(name):
    c = _case(name)
    _assert_no_preactivation_near_zero(c)
    got = _run(c)
    R.check(dict(test="fp32", case=name, dims=list(c["dims"][:4]), relu=c["conv"]["relu"]), "fused", got, c["ref"], c["bounds"])
    if c["conv"]["relu"]:                                             # the mask is the reference's, element for element
        assert torch.equal(got["y"].cpu() > 0, c["ref"]["z"] > 0)


@pytest.mark.parametrize("which", ["cin52_relu_2tile+1", "cin8_9x11"])
def test_small_integers_give_the_exact_answer(which):
    """Pre-activations of exactly zero occur; the gradient there is 0 ([z > 0]) in both."""
    TH, TW = _tile()
    N, Ci, H, W, relu = (2, 52, 2 * TH + 1, 2 * TW + 1, True) if which == "cin52_relu_2tile+1" else (2, 8, 9, 11, False)
    _, ref = R.exact_integers(which, _op(relu), ((N, Ci, H, W), (CO, Ci, 3, 3), (CO,), (N, CO, H, W)), padding=1, relu=relu)
    if relu:
        assert int((ref["z"] == 0).sum()) > 0


def test_two_runs_give_the_same_bits():
    R.two_runs(_run, [(name, _case(name)) for name in ("tile_2T+1_T-1_52_relu", "ref_32_64x130")])


@pytest.mark.parametrize("name", ["cin_64", "ref_32_64x130"])
def test_requires_grad_handling(name, monkeypatch):
    c = _case(name)
    R.requires_grad_matrix(monkeypatch, C3, "c3_backward", _op(c["conv"]["relu"]), c)


def test_cpu_tensors_are_an_error():
    with pytest.raises(RuntimeError):
        C3.conv3x3(torch.zeros(1, 4, 3, 3), torch.zeros(32, 4, 3, 3), torch.zeros(32))
    with pytest.raises(RuntimeError):
        C3.conv3x3(torch.zeros(1, 6, 3, 3, device="cuda"), torch.zeros(32, 6, 3, 3, device="cuda"), torch.zeros(32, device="cuda"))


def test_what_the_op_does_not_take_goes_through_torch():
    torch.manual_seed(4)
    plain = nn.Sequential(nn.Conv2d(32, 32, 3, padding=1)).cuda()
    fused = copy.deepcopy(plain)
    assert C3.convert(fused) == 1 and type(fused[0]) is C3.FusedConv3x3
    plain, fused = plain[0], fused[0]
    x = torch.randn(2, 32, 20, 22, device="cuda")

    both = R.passthrough_pair(A.calls, "conv3x3")

    def forced(m, relu=False):
        f = copy.deepcopy(m)
        assert C3.convert(nn.Sequential(f)) == 0
        f.__class__ = C3.FusedConv3x3
        f.relu = relu
        return f

    both(plain, fused, x.to(memory_format=torch.channels_last))                                  # channels-last input
    both(copy.deepcopy(plain).half(), copy.deepcopy(fused).half(), x.half())                      # fp16 input outside autocast
    both(plain, fused, x, dtype=torch.float16)                                                    # fp16 autocast
    both(plain, fused, x, dtype=torch.bfloat16)                                                   # bf16 autocast
    nb = nn.Conv2d(32, 32, 3, padding=1, bias=False).cuda()
    both(nb, forced(nb), x)                                                                       # no bias
    s2 = nn.Conv2d(32, 32, 3, stride=2, padding=1).cuda()
    both(s2, forced(s2), x)                                                                       # stride 2
    c5 = nn.Conv2d(32, 32, 5, padding=2).cuda()
    both(c5, forced(c5), x)                                                                       # a 5x5 layer force-swapped
    c48 = nn.Conv2d(32, 48, 3, padding=1).cuda()
    both(c48, forced(c48), x)                                                                     # C_out = 48
    both(nn.Sequential(c48, nn.ReLU()), forced(c48, relu=True), x)                                # ... and the pass-through applies the ReLU itself
    both(plain, fused, x[:0])                                                                     # an empty batch
    n0 = A.calls["conv3x3"]
    assert fused(x).dtype == torch.float32 and A.calls["conv3x3"] == n0 + 1                       # and the ordinary call is the fused one


def test_a_graphless_forward_of_a_ragged_plane_is_atens():
    """The one row of profiles/conv3x3_shapes.md on which the fused op lost: a forward that records no graph, on a plane that is not whole tiles.
    With a graph the same plane is the fused op's, and so is a graphless forward of whole tiles."""
    TH, TW = _tile()
    assert C3.tile() == (TH, TW)
    torch.manual_seed(8)
    plain = nn.Conv2d(32, 32, 3, padding=1).cuda()
    fused = copy.deepcopy(plain)
    fused.__class__ = C3.FusedConv3x3
    ragged, whole = torch.randn(1, 32, TH + 1, TW + 1, device="cuda"), torch.randn(1, 32, TH, 2 * TW, device="cuda")

    def counts(fn):
        n0, p0 = A.calls["conv3x3"], A.calls["conv3x3_passthrough"]
        out = fn()
        return out, A.calls["conv3x3"] - n0, A.calls["conv3x3_passthrough"] - p0

    with torch.no_grad():
        y, n, p = counts(lambda: fused(ragged))
        assert (n, p) == (0, 1) and torch.equal(y, plain(ragged))
        y, n, p = counts(lambda: fused(whole))
        assert (n, p) == (1, 0) and torch.equal(y, C3.conv3x3(whole, plain.weight, plain.bias))
    y, n, p = counts(lambda: fused(ragged))                       # the parameters require grad: a graph is recorded
    assert (n, p) == (1, 0) and y.grad_fn is not None
    frozen = copy.deepcopy(fused).requires_grad_(False)
    assert counts(lambda: frozen(ragged))[1:] == (0, 1)           # nothing requires grad: graphless
    assert counts(lambda: frozen(ragged.clone().requires_grad_(True)))[1:] == (1, 0)


def test_the_composed_head():
    """Conv3x3(32, 32) -> ReLU -> Conv1x1(32, 3) -> Softplus(100) with conv3x3.convert and gshead.convert applied in both orders: the same module
    classes, and output and parameter gradients under the criterion of test_gpu_stemconv.py::test_the_whole_stem -- err = max |t - t64| / max |t64|,
    fused <= max(2 x the fp32 torch CPU error, floor), floor 1e-6 for the output and 1e-3 for the gradients, both against the fp64 module."""
    torch.manual_seed(35)
    base = nn.Sequential(nn.Conv2d(32, 32, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(32, 3, 1), nn.Softplus(beta=100))
    x, g = torch.randn(2, 32, 40, 70), torch.randn(2, 3, 40, 70)
    ref = copy.deepcopy(base).double()
    out64 = ref(x.double())
    out64.backward(g.double())
    cpu32 = copy.deepcopy(base)
    out32 = cpu32(x)
    out32.backward(g)
    a, b = copy.deepcopy(base).cuda(), copy.deepcopy(base).cuda()
    assert C3.convert(a) == 1 and GH.convert(a) == 1
    assert GH.convert(b) == 1 and C3.convert(b) == 1
    want = [C3.FusedConv3x3, nn.Identity, GH.FusedHeadConv, nn.Identity]
    assert [type(m) for m in a] == want == [type(m) for m in b]
    assert a[0].relu is False and b[0].relu is False
    assert list(a.state_dict().keys()) == list(base.state_dict().keys()) == list(b.state_dict().keys())
    names = ["out"] + [n for n, _ in base.named_parameters()]
    refs = [out64.detach()] + [p.grad for p in ref.parameters()]
    torch_err = [R.rel_err(t, t64) for t, t64 in zip([out32.detach()] + [p.grad for p in cpu32.parameters()], refs)]
    n0, h0 = A.calls["conv3x3"], A.calls["gshead"]
    res = []
    for net in (a, b):
        out = net(x.cuda())
        out.backward(g.cuda())
        torch.cuda.synchronize()
        res.append([out.detach()] + [p.grad for p in net.parameters()])
    assert A.calls["conv3x3"] == n0 + 2 and A.calls["gshead"] == h0 + 2
    for ta, tb in zip(*res):
        assert torch.equal(ta, tb)                                     # the same modules: the same bits
    rec = dict(test="composed_head", fused={}, torch_cpu={})
    for n, t64, te, tf in zip(names, refs, torch_err, res[0]):
        rec["torch_cpu"][n], rec["fused"][n] = te, R.rel_err(tf, t64)
    print(json.dumps(rec))
    for n in names:
        floor = 1e-6 if n == "out" else 1e-3
        assert rec["fused"][n] <= max(2.0 * rec["torch_cpu"][n], floor), "%s: fused %.3e, torch %.3e" % (n, rec["fused"][n], rec["torch_cpu"][n])
