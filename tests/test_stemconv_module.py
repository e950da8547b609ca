"""CPU: stemconv.convert / FusedStemConv2d on a stand-in tree (which layers are swapped, what stays the same, the pass-through for CPU tensors), the
op's refusal of a CPU tensor, and the `stemconv` name of GPSGS_ACCELERATE."""
import copy

import pytest
import torch
from torch import nn

import gps_gaussian_amd  # noqa: F401
from gps_gaussian_amd import accelerate as A
from gps_gaussian_amd import stemconv as SC

import hook_run


@pytest.fixture(scope="module", autouse=True)
def _built():
    gps_gaussian_amd.build()


class _StandIn(nn.Module):
    """Two encoders' worth of stems and the convolutions that must be left alone (written for this test)."""

    def __init__(self):
        super().__init__()
        self.in_ds = nn.Sequential(nn.Conv2d(3, 32, 5, stride=2, padding=2), nn.GroupNorm(8, 32), nn.ReLU(inplace=True))
        self.depth = nn.Conv2d(1, 32, 5, stride=2, padding=2)
        self.c3 = nn.Conv2d(32, 32, 3, padding=1)
        self.c5s1 = nn.Conv2d(3, 32, 5, stride=1, padding=2)
        self.nobias = nn.Conv2d(3, 32, 5, stride=2, padding=2, bias=False)
        self.reflect = nn.Conv2d(3, 32, 5, stride=2, padding=2, padding_mode="reflect")
        self.wide = nn.Conv2d(3, 72, 5, stride=2, padding=2)
        self.again = nn.Sequential(self.depth)             # a second parent of a supported layer


def test_convert_swaps_exactly_the_supported_layers():
    torch.manual_seed(2)
    net = _StandIn()
    keys = list(net.state_dict().keys())
    params = {n: p for n, p in net.named_parameters()}
    assert SC.convert(net) == 2
    assert type(net.in_ds[0]) is SC.FusedStemConv2d and type(net.depth) is SC.FusedStemConv2d and net.again[0] is net.depth
    for m in (net.c3, net.c5s1, net.nobias, net.reflect, net.wide):
        assert type(m) is nn.Conv2d
    assert type(net.in_ds[1]) is nn.GroupNorm and type(net.in_ds[2]) is nn.ReLU
    assert list(net.state_dict().keys()) == keys
    assert all(p is params[n] for n, p in net.named_parameters()) and len(params) == len(list(net.named_parameters()))
    assert SC.convert(net) == 0                            # idempotent
    assert isinstance(net.depth, nn.Conv2d) and SC.convert(nn.Conv2d(1, 8, 5, stride=2, padding=2)) == 1   # the module itself


def test_cpu_input_is_nn_conv2d_forward_and_counted():
    torch.manual_seed(3)
    plain = nn.Conv2d(3, 32, 5, stride=2, padding=2)
    fused = copy.deepcopy(plain)
    assert SC.convert(fused) == 1
    x = torch.randn(2, 3, 19, 23)
    n0, p0 = A.calls["stemconv"], A.calls["stemconv_passthrough"]
    a, b = plain(x), fused(x)
    assert torch.equal(a, b) and A.calls["stemconv_passthrough"] == p0 + 1 and A.calls["stemconv"] == n0
    xg = x.clone().requires_grad_(True)
    fused(xg).sum().backward()                             # ATen's autograd, as for any nn.Conv2d
    assert xg.grad is not None and fused.weight.grad is not None


def test_the_op_itself_raises_on_a_cpu_tensor():
    w, b = torch.randn(32, 3, 5, 5), torch.randn(32)
    with pytest.raises(RuntimeError, match="GPU"):
        SC.conv2d(torch.randn(1, 3, 8, 8), w, b, 2, 2)


def test_the_stemconv_name():
    hook_run.assert_the_names(A)
    assert A.requested("stemconv") == ("stemconv",)
    assert A.requested("all,stemconv") == A.FEATURES + ("stemconv",)
    assert "stemconv" not in A.requested("all") and A.requested("all") == A.FEATURES
    assert A.requested("stemconv,resblock,groupnorm,splat") == ("splat", "groupnorm", "resblock", "stemconv")   # after the existing names
    assert "stemconv" in A.calls and "stemconv_passthrough" in A.calls
    with pytest.raises(ValueError):
        A.requested("stemconv,stemconvs")
    with pytest.raises(ValueError):
        A.requested("conv")
