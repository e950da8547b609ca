"""CPU: gshead.convert / FusedHeadConv as modules -- what is converted and what is left alone, state_dict untouched, the pass-through computing
the SAME function as the unconverted chain bit for bit (on a CPU tensor everything is the pass-through), the counters, and the opt-in name."""
import copy

import pytest
import torch
from torch import nn

import gps_gaussian_amd
from gps_gaussian_amd import accelerate as A
from gps_gaussian_amd import gshead as GH

import hook_run


@pytest.fixture(autouse=True)
def _built():
    gps_gaussian_amd.build()


def _heads(C=32):
    """The three heads as lib/gs_parm_network.py:34-50 builds them."""
    torch.manual_seed(3)
    return nn.ModuleDict(dict(
        rot=nn.Sequential(nn.Conv2d(C, C, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(C, 4, 1)),
        scale=nn.Sequential(nn.Conv2d(C, C, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(C, 3, 1), nn.Softplus(beta=100)),
        opacity=nn.Sequential(nn.Conv2d(C, C, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(C, 1, 1), nn.Sigmoid())))


def _classes(seq):
    return [type(m) for m in seq]


def test_convert_takes_the_three_head_shapes():
    for C in (16, 32, 64):
        net = _heads(C)
        before = {k: v.clone() for k, v in net.state_dict().items()}
        assert GH.convert(net) == 3
        assert _classes(net["rot"]) == [nn.Conv2d, nn.Identity, GH.FusedHeadConv]
        assert _classes(net["scale"]) == [nn.Conv2d, nn.Identity, GH.FusedHeadConv, nn.Identity]
        assert _classes(net["opacity"]) == [nn.Conv2d, nn.Identity, GH.FusedHeadConv, nn.Identity]
        assert (net["rot"][2].act, net["scale"][2].act, net["opacity"][2].act) == ("none", "softplus", "sigmoid")
        assert (net["scale"][2].beta, net["scale"][2].threshold) == (100, 20)
        after = net.state_dict()
        assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
        assert GH.convert(net) == 0                                                     # idempotent
        assert isinstance(net["rot"][2], nn.Conv2d)
        net2 = _heads(C)
        net2.load_state_dict(after)                                                     # and the keys load into the plain modules


def test_convert_leaves_everything_else_alone():
    def untouched(seq):
        want = _classes(seq)
        assert GH.convert(seq) == 0 and _classes(seq) == want

    untouched(nn.Sequential(nn.ReLU(), nn.Conv2d(32, 4, 3, padding=1)))                 # a ReLU followed by a 3x3 convolution
    untouched(nn.Sequential(nn.ReLU(), nn.Conv2d(32, 4, 1, bias=False)))                # no bias
    untouched(nn.Sequential(nn.ReLU(), nn.Conv2d(24, 4, 1)))                            # C_in = 24
    untouched(nn.Sequential(nn.ReLU(), nn.Conv2d(32, 5, 1)))                            # C_out = 5
    untouched(nn.Sequential(nn.ReLU(), nn.Conv2d(32, 4, 1, stride=2)))
    untouched(nn.Sequential(nn.ReLU(), nn.Conv2d(32, 4, 1, padding=1)))
    untouched(nn.Sequential(nn.ReLU(), nn.Conv2d(32, 4, 1, groups=2)))
    untouched(nn.Sequential(nn.ReLU(), nn.Conv2d(32, 4, 1, padding_mode="reflect")))
    untouched(nn.Sequential(nn.Conv2d(32, 4, 1), nn.Sigmoid()))                         # no ReLU in front
    untouched(nn.Sequential(nn.ReLU(), nn.GroupNorm(4, 32), nn.Conv2d(32, 4, 1)))       # a ReLU followed by anything else
    untouched(nn.Sequential(nn.LeakyReLU(), nn.Conv2d(32, 4, 1)))
    loose = nn.ModuleList([nn.ReLU(), nn.Conv2d(32, 4, 1)])                             # the same pair outside a Sequential: no order of execution
    untouched(loose)

    class MyConv(nn.Conv2d):
        pass

    untouched(nn.Sequential(nn.ReLU(), MyConv(32, 4, 1)))                               # a subclass
    tanh = nn.Sequential(nn.ReLU(), nn.Conv2d(32, 4, 1), nn.Tanh())                     # another activation stays where it is
    assert GH.convert(tanh) == 1 and _classes(tanh) == [nn.Identity, GH.FusedHeadConv, nn.Tanh] and tanh[1].act == "none"


def test_the_passthrough_is_the_same_function_bit_for_bit():
    """On CPU tensors every converted forward is the pass-through; output and all gradients must equal the unconverted module's bits: the ReLU and
    the activation, whose slots are now nn.Identity, are still applied."""
    plain = _heads(16)
    fused = copy.deepcopy(plain)
    assert GH.convert(fused) == 3
    x = torch.randn(2, 16, 9, 11)
    g = {k: torch.randn(2, m[2].out_channels, 9, 11) for k, m in plain.items()}
    n0, p0 = A.calls["gshead"], A.calls["gshead_passthrough"]
    for key in plain:
        res = []
        for net in (plain, fused):
            xin = x.clone().requires_grad_(True)
            y = net[key](xin)
            y.backward(g[key])
            res.append([y.detach(), xin.grad] + [p.grad for p in net[key].parameters()])
        assert len(res[0]) == 6 and all(torch.equal(a, b) for a, b in zip(*res)), key
    assert A.calls["gshead"] == n0 and A.calls["gshead_passthrough"] == p0 + 3
    # the ReLU really is inside: a chain whose 1x1 convolution sees negative values
    seq = nn.Sequential(nn.ReLU(), nn.Conv2d(16, 2, 1), nn.Sigmoid())
    ref = copy.deepcopy(seq)
    assert GH.convert(seq) == 1
    xn = -torch.rand(1, 16, 3, 3) - 1
    with torch.no_grad():
        assert torch.equal(seq(xn), ref(xn)) and torch.equal(seq(xn), torch.sigmoid(seq[1].bias).view(1, 2, 1, 1).expand(1, 2, 3, 3))


def test_head_has_no_cpu_path():
    with pytest.raises(RuntimeError, match="GPU"):
        GH.head(torch.randn(1, 32, 4, 4), torch.randn(4, 32), torch.randn(4))


def test_the_opt_in_name():
    hook_run.assert_the_names(A)
    assert "gshead" in A.calls and "gshead_passthrough" in A.calls
    assert A.requested("gshead") == ("gshead",)
    assert "gshead" not in A.requested("all") and A.requested("all") == A.FEATURES
    for other in ("groupnorm", "resblock", "stemconv", "all,groupnorm,splat"):
        assert "gshead" not in A.requested(other)
    assert A.requested("resblock,stemconv,gshead") == ("resblock", "stemconv", "gshead")
    with pytest.raises(ValueError):
        A.requested("gsheads")
