"""CPU: groupnorm.convert / FusedGroupNorm on a module tree the test builds itself, and the `groupnorm` name of GPSGS_ACCELERATE.

On the CPU a FusedGroupNorm hands every call to nn.GroupNorm.forward (there is no GPU to run the kernels on): the converted tree must then give
the bits of an unconverted copy, forward and backward, and count each call in accelerate.calls["groupnorm_passthrough"]."""
import copy

import pytest
import torch
from torch import nn

import gps_gaussian_amd  # noqa: F401
from gps_gaussian_amd import accelerate as A
from gps_gaussian_amd import groupnorm as GN

import hook_run


class _Branch(nn.Module):
    def __init__(self, norm):
        super().__init__()
        self.conv = nn.Conv2d(8, 8, 3, padding=1)
        self.norm = norm                                  # the SAME module object in both branches

    def forward(self, x):
        return torch.relu_(self.norm(self.conv(x)))


class _Tree(nn.Module):
    """Four GroupNorm objects reachable through five attribute paths (one shared by two parents), one affine=False, one BatchNorm."""

    def __init__(self):
        super().__init__()
        shared = nn.GroupNorm(2, 8)
        self.a = _Branch(shared)
        self.b = _Branch(shared)
        self.head = nn.Sequential(nn.Conv2d(8, 12, 1), nn.GroupNorm(3, 12), nn.ReLU(inplace=True), nn.BatchNorm2d(12))
        self.plain = nn.GroupNorm(4, 12, affine=False)
        self.tail = nn.GroupNorm(1, 12)

    def forward(self, x):
        return self.tail(self.plain(self.head(self.a(x) + self.b(x))))


def _tree():
    torch.manual_seed(3)
    t = _Tree()
    with torch.no_grad():
        for m in t.modules():
            if isinstance(m, nn.GroupNorm) and m.affine:
                m.weight.normal_()
                m.bias.normal_()
    return t


def test_convert_counts_shared_modules_once_keeps_the_state_dict_and_is_idempotent():
    t = _tree()
    keys = list(t.state_dict().keys())
    params = [id(p) for p in t.parameters()]
    assert GN.convert(t) == 4
    assert t.a.norm is t.b.norm and type(t.a.norm) is GN.FusedGroupNorm
    assert all(type(m) is GN.FusedGroupNorm for m in t.modules() if isinstance(m, nn.GroupNorm))
    assert type(t.head[3]) is nn.BatchNorm2d
    assert list(t.state_dict().keys()) == keys and [id(p) for p in t.parameters()] == params
    assert GN.convert(t) == 0
    assert GN.convert(nn.GroupNorm(2, 4)) == 1            # the root itself counts
    fresh = _tree()
    fresh.load_state_dict(t.state_dict())                 # the keys and shapes of an unconverted tree
    c = copy.deepcopy(t)
    assert type(c.tail) is GN.FusedGroupNorm and c.a.norm is c.b.norm


def test_cpu_forward_and_backward_are_the_bits_of_the_unconverted_tree():
    ref = _tree()
    fused = copy.deepcopy(ref)
    assert GN.convert(fused) == 4
    x = torch.randn(2, 8, 9, 7)
    before = dict(A.calls)
    outs = []
    for net in (ref, fused):
        xi = x.clone().requires_grad_(True)
        y = net(xi)
        y.square().sum().backward()
        outs.append((y.detach(), xi.grad, [p.grad for p in net.parameters()]))
    (y0, g0, p0), (y1, g1, p1) = outs
    assert torch.equal(y0, y1) and torch.equal(g0, g1)
    assert len(p0) == len(p1) and all(torch.equal(a, b) for a, b in zip(p0, p1))
    # five GroupNorm calls per forward (the shared one runs twice), all handed to nn.GroupNorm.forward; none counted as fused
    assert A.calls["groupnorm_passthrough"] - before["groupnorm_passthrough"] == 5
    assert A.calls["groupnorm"] == before["groupnorm"]


def test_the_op_itself_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match="GPU"):
        GN.group_norm(torch.zeros(1, 4, 2, 2), 2, torch.ones(4), torch.zeros(4))


def test_groupnorm_is_accepted_by_name_only():
    hook_run.assert_the_names(A)
    assert A.requested("groupnorm") == ("groupnorm",)
    assert A.requested("all") == A.FEATURES and "groupnorm" not in A.FEATURES
    assert A.requested("all,groupnorm,splat") == A.FEATURES + ("splat", "groupnorm")
    assert A.requested("groupnorm,loss") == ("loss", "groupnorm")
    assert "groupnorm" in A.calls and "groupnorm_passthrough" in A.calls
    with pytest.raises(ValueError):
        A.requested("groupnrom")
