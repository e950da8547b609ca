"""CPU: the Python side of the fused GroupNorm epilogues -- FusedGroupNorm.forward_relu, residual_block_forward and fuse_sequential_relu on a
stand-in the tests build themselves (tests/gn_epilogue_cases.py), and the `resblock` name of GPSGS_ACCELERATE.

On the CPU nothing can run the kernels: every norm hands its call to nn.GroupNorm.forward followed by the reference's own relu_ / add / relu, so the
converted network must give the bits of an unconverted copy, forward and backward, and count each call as a pass-through.  The last test checks the
precondition of the GPU test's guard band."""
import copy

import pytest
import torch
from torch import nn

import gps_gaussian_amd  # noqa: F401
from gps_gaussian_amd import accelerate as A
from gps_gaussian_amd import groupnorm as GN

import gn_epilogue_cases as E
import hook_run


def _run(net, x, g):
    xi = x.clone().requires_grad_(True)
    y = net(xi)
    y.backward(g)
    return y.detach(), xi.grad, [p.grad for p in net.parameters()]


def test_cpu_bits_state_dict_counters_deepcopy_and_idempotence():
    base, x, g = E.stand_in()
    fused = copy.deepcopy(base)
    keys = list(fused.state_dict().keys())
    params = [id(p) for p in fused.parameters()]
    assert GN.convert(fused) == 4
    assert GN.fuse_sequential_relu(fused) == 1               # the stem; the downsample Sequential has no ReLU
    assert type(fused.stem[1]) is GN.FusedGroupNormReLU and type(fused.stem[2]) is nn.Identity and len(fused.stem) == 3
    assert type(fused.block.norm3) is GN.FusedGroupNorm and fused.block.downsample[1] is fused.block.norm3
    assert GN.fuse_sequential_relu(fused) == 0 and GN.convert(fused) == 0
    assert list(fused.state_dict().keys()) == keys and [id(p) for p in fused.parameters()] == params
    fresh = E.stand_in()[0]
    fresh.load_state_dict(fused.state_dict())                # the keys and shapes of an unconverted network
    fused.fused_forward = True
    twin = copy.deepcopy(fused)
    assert type(twin.stem[1]) is GN.FusedGroupNormReLU and twin.block.downsample[1] is twin.block.norm3

    before = dict(A.calls)
    y0, g0, p0 = _run(base, x, g)
    y1, g1, p1 = _run(fused, x, g)
    assert torch.equal(y0, y1) and torch.equal(g0, g1)
    assert len(p0) == len(p1) and all(torch.equal(a, b) for a, b in zip(p0, p1))
    # stem, norm1, norm2, norm3: all handed to nn.GroupNorm.forward, none counted as fused; the block went through residual_block_forward
    assert A.calls["groupnorm_passthrough"] - before["groupnorm_passthrough"] == 4 and A.calls["groupnorm"] == before["groupnorm"]
    assert A.calls["resblock"] - before["resblock"] == 1 and A.calls["resblock_passthrough"] == before["resblock_passthrough"]
    y2, g2, p2 = _run(twin, x, g)
    assert torch.equal(y0, y2) and torch.equal(g0, g2)


def test_residual_block_forward_on_an_unconverted_block_and_without_downsample():
    base, x, g = E.stand_in()
    for drop in (False, True):
        blk = copy.deepcopy(base.block)
        if drop:
            blk.downsample = None
        xi = torch.randn(2, 16, 9, 7)
        a = blk(xi)
        b = GN.residual_block_forward(blk, xi)               # plain nn.GroupNorm layers: the same ops, written out
        assert torch.equal(a, b)


def test_forward_relu_on_cpu_is_the_references_ops():
    torch.manual_seed(4)
    m = nn.GroupNorm(2, 8)
    with torch.no_grad():
        m.weight.normal_()
        m.bias.normal_()
    f = copy.deepcopy(m)
    assert GN.convert(f) == 1
    x, r = torch.randn(2, 8, 5, 3), torch.randn(2, 8, 5, 3)
    before = A.calls["groupnorm_passthrough"]
    assert torch.equal(f.forward_relu(x), torch.relu_(m(x)))
    assert torch.equal(f.forward_relu(x, r), torch.relu(r + torch.relu_(m(x))))
    assert torch.equal(f(x), m(x))                           # forward itself is unchanged
    assert A.calls["groupnorm_passthrough"] == before + 3


def test_blocks_without_groupnorm_run_their_own_forward():
    class _Batch(E.StandInBlock):
        def __init__(self):
            super().__init__()
            self.norm1, self.norm2 = nn.BatchNorm2d(16), nn.BatchNorm2d(16)

    blk = _Batch().eval()
    x = torch.randn(2, 16, 6, 5)
    before = dict(A.calls)
    assert torch.equal(GN.residual_block_forward(blk, x), blk(x))
    assert A.calls["resblock_passthrough"] == before["resblock_passthrough"] + 1 and A.calls["resblock"] == before["resblock"]


def test_a_norm_with_two_users_is_not_fused_with_one_users_relu():
    shared = nn.GroupNorm(2, 8)
    net = nn.ModuleDict(dict(a=nn.Sequential(nn.Conv2d(8, 8, 1), shared, nn.ReLU()), b=nn.Sequential(nn.Conv2d(8, 8, 1), shared)))
    assert GN.fuse_sequential_relu(net) == 0 and type(net["a"][2]) is nn.ReLU
    lone = nn.Sequential(nn.GroupNorm(2, 8), nn.Tanh(), nn.GroupNorm(2, 8), nn.ReLU(), nn.ReLU())
    assert GN.fuse_sequential_relu(lone) == 1
    assert type(lone[0]) is nn.GroupNorm and type(lone[2]) is GN.FusedGroupNormReLU and type(lone[3]) is nn.Identity and type(lone[4]) is nn.ReLU


def test_the_op_itself_refuses_cpu_tensors_and_a_residual_without_relu():
    x, w, b = torch.zeros(1, 4, 2, 2), torch.ones(4), torch.zeros(4)
    with pytest.raises(RuntimeError, match="GPU"):
        GN.group_norm(x, 2, w, b, relu=True)
    with pytest.raises(RuntimeError, match="GPU"):
        GN.group_norm(x, 2, w, b, relu=True, residual=torch.zeros_like(x))
    with pytest.raises(RuntimeError, match="relu=True"):
        GN.group_norm(x, 2, w, b, residual=torch.zeros_like(x))


def test_resblock_is_accepted_by_name_only():
    hook_run.assert_the_names(A)
    assert A.requested("resblock") == ("resblock",)
    assert A.requested("all") == A.FEATURES and "resblock" not in A.FEATURES
    assert A.requested("all,resblock") == A.FEATURES + ("resblock",)
    assert A.requested("resblock,groupnorm,loss") == ("loss", "groupnorm", "resblock")
    assert A.requested("all,groupnorm,splat") == A.FEATURES + ("splat", "groupnorm")
    for k in ("resblock", "resblock_passthrough"):
        assert k in A.calls
    with pytest.raises(ValueError):
        A.requested("resblok")
    # the table: the constructors once, under whichever name asks first; the forward only with resblock
    rows = lambda feats: {f: [m + "." + a for m, a, _ in r] for f, r in A._table(feats).items()}
    inits = ["core.extractor.ResidualBlock.__init__", "core.extractor.UnetExtractor.__init__"]
    assert rows(("groupnorm",)) == {"groupnorm": inits}
    assert rows(("resblock",)) == {"resblock": inits + ["core.extractor.ResidualBlock.forward"]}
    assert rows(("groupnorm", "resblock")) == {"groupnorm": inits, "resblock": ["core.extractor.ResidualBlock.forward"]}


@pytest.mark.parametrize("name", E.NAMES)
def test_guard_band_precondition(name):
    """What the GPU test's fp64 comparison leaves out stays under its cap for every case and form, and is nothing at all for the short rows."""
    for form in E.FORMS:
        share = E.ref64(name, form)["excluded_share"]
        print(name, form, "excluded share %.3e" % share)
        assert share <= E.SHARE_CAP
        if name in E.SHORT_ROWS:
            assert share == 0.0
    if name in E.FP16_NAMES:
        assert E.ref64(name, "relu_add_relu", half=True)["excluded_share"] <= E.SHARE_CAP
