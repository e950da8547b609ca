"""CPU: conv3x3.convert / fuse_relu / convert_regresser / FusedConv3x3 as modules -- what is converted and what is left alone, state_dict untouched,
the pass-through computing the SAME function as the unconverted layers bit for bit (on a CPU tensor everything is the pass-through), the counters
that appear only when the name is asked for, and the by-name opt-in."""
import copy
import json
import subprocess
import sys

import pytest
import torch
from torch import nn

from conftest import ROOT

import gps_gaussian_amd
from gps_gaussian_amd import accelerate as A
from gps_gaussian_amd import conv3x3 as C3
from gps_gaussian_amd import gshead as GH

import hook_run

SIXTEEN = ["pack", "loss", "corr", "upsample", "unproject", "splat", "groupnorm", "resblock", "stemconv", "gshead", "loss_passthrough",
           "unproject_passthrough", "groupnorm_passthrough", "resblock_passthrough", "stemconv_passthrough", "gshead_passthrough"]


@pytest.fixture(autouse=True)
def _built():
    gps_gaussian_amd.build()
    yield
    A.restore()          # the process's counter keys are what they were: other files assert them


class Block(nn.Module):
    """Convolutions as attributes, as core/extractor.py's ResidualBlock holds them: no Sequential says in which order they run."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(32, 32, 3, padding=1)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(32, 32, 3, padding=1)

    def forward(self, x):
        return self.relu(self.conv2(self.relu(self.conv1(x))))


class Regresser(nn.Module):
    """The full-resolution stage of lib/gs_parm_network.py:26-50 with stand-in decoders."""

    def __init__(self, dec=48, head=32):
        super().__init__()
        self.decoder1 = nn.Sequential(Block(), Block())
        self.in_ds = nn.Sequential(nn.Conv2d(3, 32, 5, stride=2, padding=2), nn.GroupNorm(8, 32), nn.ReLU(inplace=True))
        self.mid = nn.Sequential(nn.Conv2d(32, 48, 3, padding=1), nn.Conv2d(48, 96, 3, padding=1))
        self.out_conv = nn.Conv2d(dec + 3 + 1, head, kernel_size=3, padding=1)
        self.out_relu = nn.ReLU(inplace=True)
        self.rot_head = nn.Sequential(nn.Conv2d(head, head, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(head, 4, 1))
        self.scale_head = nn.Sequential(nn.Conv2d(head, head, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(head, 3, 1), nn.Softplus(beta=100))
        self.opacity_head = nn.Sequential(nn.Conv2d(head, head, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(head, 1, 1), nn.Sigmoid())

    def forward(self, x):
        out = self.out_relu(self.out_conv(x))
        return self.rot_head(out), self.scale_head(out), self.opacity_head(out)


def _classes(seq):
    return [type(m) for m in seq]


def _same_state(a, before):
    after = a.state_dict()
    return list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)


def test_convert_regresser_takes_four_layers_and_nothing_else():
    torch.manual_seed(5)
    net = Regresser()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    assert C3.convert_regresser(net) == 4
    assert type(net.out_conv) is C3.FusedConv3x3 and net.out_conv.relu is True and type(net.out_relu) is nn.Identity
    for head in (net.rot_head, net.scale_head, net.opacity_head):
        assert type(head[0]) is C3.FusedConv3x3 and head[0].relu is False and type(head[1]) is nn.ReLU and type(head[2]) is nn.Conv2d
    fused = [m for m in net.modules() if isinstance(m, C3.FusedConv3x3)]
    assert len(fused) == 4
    for blk in net.decoder1:                                                          # attribute convolutions of a block: left alone
        assert type(blk.conv1) is nn.Conv2d and type(blk.conv2) is nn.Conv2d and type(blk.relu) is nn.ReLU
    assert _classes(net.in_ds) == [nn.Conv2d, nn.GroupNorm, nn.ReLU] and _classes(net.mid) == [nn.Conv2d, nn.Conv2d]   # other shapes
    assert _same_state(net, before)
    assert C3.convert_regresser(net) == 0 and C3.convert(net) == 0                    # idempotent
    Regresser().load_state_dict(net.state_dict())                                     # and the keys load into the plain modules
    assert "relu=True" in repr(net.out_conv) and "relu=False" in repr(net.rot_head[0])


def test_convert_and_gshead_compose_in_either_order():
    a, b = Regresser(), Regresser()
    assert C3.convert_regresser(a) == 4 and GH.convert(a) == 3
    assert GH.convert(b) == 3 and C3.convert_regresser(b) == 4
    for name in ("rot_head", "scale_head", "opacity_head"):
        assert _classes(getattr(a, name)) == _classes(getattr(b, name))
        assert _classes(getattr(a, name))[:3] == [C3.FusedConv3x3, nn.Identity, GH.FusedHeadConv]
    assert list(a.state_dict()) == list(b.state_dict()) == list(Regresser().state_dict())


def test_convert_leaves_everything_else_alone():
    def untouched(m):
        want = [type(x) for x in m.modules()]
        assert C3.convert(m) == 0 and [type(x) for x in m.modules()] == want

    untouched(Block())                                                                  # attribute convolutions, no Sequential
    untouched(nn.ModuleList([nn.Conv2d(32, 32, 3, padding=1)]))
    untouched(nn.Conv2d(32, 32, 3, padding=1))                                          # a bare layer is in no Sequential either
    untouched(nn.Sequential(nn.Conv2d(32, 48, 3, padding=1)))                           # C_out != 32
    untouched(nn.Sequential(nn.Conv2d(32, 16, 3, padding=1)))
    untouched(nn.Sequential(nn.Conv2d(3, 32, 3, padding=1)))                            # C_in no multiple of 4
    untouched(nn.Sequential(nn.Conv2d(96, 32, 3, padding=1)))                           # C_in > 64
    untouched(nn.Sequential(nn.Conv2d(32, 32, 3, padding=1, bias=False)))
    untouched(nn.Sequential(nn.Conv2d(32, 32, 3, padding=1, stride=2)))
    untouched(nn.Sequential(nn.Conv2d(32, 32, 3, padding=0)))
    untouched(nn.Sequential(nn.Conv2d(32, 32, 3, padding="same")))                      # a padding given as a string
    untouched(nn.Sequential(nn.Conv2d(32, 32, 3, padding=2, dilation=2)))
    untouched(nn.Sequential(nn.Conv2d(32, 32, 3, padding=1, groups=2)))
    untouched(nn.Sequential(nn.Conv2d(32, 32, 3, padding=1, padding_mode="reflect")))
    untouched(nn.Sequential(nn.Conv2d(32, 32, 5, padding=2)))
    untouched(nn.Sequential(nn.Conv2d(32, 32, (3, 1), padding=(1, 0))))

    class MyConv(nn.Conv2d):
        pass

    untouched(nn.Sequential(MyConv(32, 32, 3, padding=1)))                              # a subclass
    seq = nn.Sequential(nn.Conv2d(52, 32, 3, padding=1), nn.ReLU())                     # convert() never folds a ReLU: that is fuse_relu's
    assert C3.convert(seq) == 1 and _classes(seq) == [C3.FusedConv3x3, nn.ReLU] and seq[0].relu is False


def test_fuse_relu_needs_a_plain_pair():
    for owner, names in ((Block(), ("conv1", "relu")),):
        assert C3.fuse_relu(owner, *names) == 1 and type(owner.conv1) is C3.FusedConv3x3 and owner.conv1.relu and type(owner.relu) is nn.Identity
        assert C3.fuse_relu(owner, *names) == 0                                         # already converted
    net = Regresser(head=16)                                                            # C_out = 16: nothing changes
    assert C3.fuse_relu(net, "out_conv", "out_relu") == 0 and type(net.out_conv) is nn.Conv2d and type(net.out_relu) is nn.ReLU
    assert C3.convert_regresser(net) == 0
    net = Regresser()
    net.out_relu = nn.LeakyReLU()
    assert C3.fuse_relu(net, "out_conv", "out_relu") == 0 and type(net.out_conv) is nn.Conv2d
    assert C3.fuse_relu(net, "out_conv", "missing") == 0 and C3.fuse_relu(net, "missing", "out_relu") == 0
    assert C3.convert_regresser(net) == 3                                               # the heads still convert


def test_the_cpu_forward_is_torchs_bit_for_bit():
    """On CPU tensors every converted forward is the pass-through; outputs and all gradients equal the unconverted module's bits: the ReLU whose
    attribute is now nn.Identity is still applied."""
    torch.manual_seed(6)
    plain = Regresser()
    fused = copy.deepcopy(plain)
    assert C3.convert_regresser(fused) == 4
    x = torch.randn(2, 52, 9, 11)
    gs = [torch.randn(2, k, 9, 11) for k in (4, 3, 1)]
    assert list(A.calls) == SIXTEEN                                                     # converting creates no counter, counting does
    res = []
    for net in (plain, fused):
        xin = x.clone().requires_grad_(True)
        outs = net(xin)
        torch.autograd.backward(outs, gs)
        params = [net.out_conv] + [h[i] for h in (net.rot_head, net.scale_head, net.opacity_head) for i in (0, 2)]
        res.append(list(outs) + [xin.grad] + [p.grad for m in params for p in m.parameters()])
    assert len(res[0]) == 18 and all(torch.equal(a.detach(), b.detach()) for a, b in zip(*res))
    assert (res[1][0] != 0).any() and A.calls["conv3x3"] == 0 and A.calls["conv3x3_passthrough"] == 4
    assert list(A.calls) == SIXTEEN + ["conv3x3", "conv3x3_passthrough"]
    # the ReLU really is inside the relu=True layer
    with torch.no_grad():
        y = fused.out_conv(x)
    assert float(y.min()) == 0.0 and torch.equal(y, torch.relu(plain.out_conv(x)))


def test_the_op_has_no_cpu_path():
    with pytest.raises(RuntimeError, match="GPU"):
        C3.conv3x3(torch.randn(1, 32, 4, 4), torch.randn(32, 32, 3, 3), torch.randn(32))


def test_the_name_is_by_name_only():
    hook_run.assert_the_names(A)
    assert list(A.calls) == SIXTEEN
    assert "conv3x3" not in A.requested("all") and A.requested("all") == A.FEATURES
    for other in ("groupnorm", "resblock", "stemconv", "gshead", "all,groupnorm,splat", "resblock,stemconv,gshead"):
        assert "conv3x3" not in A.requested(other)
    assert list(A.calls) == SIXTEEN                                                     # nothing above asked for it
    assert A.requested("conv3x3") == ("conv3x3",)
    assert list(A.calls) == SIXTEEN + ["conv3x3", "conv3x3_passthrough"] and A.calls["conv3x3"] == 0 == A.calls["conv3x3_passthrough"]
    assert A.requested("all,conv3x3") == A.FEATURES + ("conv3x3",)
    assert A.requested("conv3x3,gshead,resblock") == ("resblock", "gshead", "conv3x3")  # after OPT_IN, whatever the order given
    with pytest.raises(ValueError):
        A.requested("conv3x3s")
    A.restore()
    assert list(A.calls) == SIXTEEN


def test_a_process_that_never_asks_keeps_todays_sixteen_keys():
    code = ("import sys, json; sys.path.insert(0, %r); import gps_gaussian_amd; from gps_gaussian_amd import accelerate as A, conv3x3\n"
            "a = list(A.calls); A.requested('all'); A.requested('gshead'); b = list(A.calls); A.requested('all,conv3x3'); c = list(A.calls)\n"
            "print(json.dumps([a, b, c]))" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    a, b, c = json.loads(out.stdout.strip().splitlines()[-1])
    assert a == SIXTEEN and b == SIXTEEN and c == SIXTEEN + ["conv3x3", "conv3x3_passthrough"]
