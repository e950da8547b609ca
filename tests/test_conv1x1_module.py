"""CPU: conv1x1.convert / FusedConv1x1 as modules -- what is converted and what is left alone, state_dict untouched, the pass-through computing the
SAME function as the unconverted layers bit for bit (on a CPU tensor everything is the pass-through), the counters that appear only when the name is
asked for, and the by-name opt-in."""
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
from gps_gaussian_amd import conv1x1 as C1
from gps_gaussian_amd import conv3x3 as C3
from gps_gaussian_amd import groupnorm as GN

import hook_run

SIXTEEN = ["pack", "loss", "corr", "upsample", "unproject", "splat", "groupnorm", "resblock", "stemconv", "gshead", "loss_passthrough",
           "unproject_passthrough", "groupnorm_passthrough", "resblock_passthrough", "stemconv_passthrough", "gshead_passthrough"]
OURS = ["conv1x1", "conv1x1_passthrough"]


@pytest.fixture(autouse=True)
def _built():
    gps_gaussian_amd.build()
    yield
    A.restore()          # the process's counter keys are what they were: other files assert them


class Block(nn.Module):
    """core/extractor.py:6-60, ResidualBlock with norm_fn 'group': 3x3 convolutions as attributes, the shortcut a Sequential of a 1x1 convolution
    and norm3 -- only where input and output differ."""

    def __init__(self, in_planes, planes, stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, planes, 3, padding=1, stride=stride)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1)
        self.relu = nn.ReLU(inplace=True)
        self.norm1, self.norm2 = nn.GroupNorm(planes // 8, planes), nn.GroupNorm(planes // 8, planes)
        self.downsample = None
        if not (stride == 1 and in_planes == planes):
            self.norm3 = nn.GroupNorm(planes // 8, planes)
            self.downsample = nn.Sequential(nn.Conv2d(in_planes, planes, 1, stride=stride), self.norm3)

    def forward(self, x):
        y = self.relu(self.norm1(self.conv1(x)))
        y = self.relu(self.norm2(self.conv2(y)))
        if self.downsample is not None:
            x = self.downsample(x)
        return self.relu(x + y)


class Encoder(nn.Module):
    """core/extractor.py:63-91 with config/stage2.yaml's widths, and a 1x1 head behind it whose channel count the op does not take."""

    def __init__(self, dims=(32, 48, 96)):
        super().__init__()
        self.in_ds = nn.Sequential(nn.Conv2d(3, 32, 5, stride=2, padding=2), nn.GroupNorm(8, 32), nn.ReLU(inplace=True))
        self.res1 = nn.Sequential(Block(32, dims[0]), Block(dims[0], dims[0]))
        self.res2 = nn.Sequential(Block(dims[0], dims[1], stride=2), Block(dims[1], dims[1]))
        self.res3 = nn.Sequential(Block(dims[1], dims[2], stride=2), Block(dims[2], dims[2]))
        self.head = nn.Sequential(nn.Conv2d(dims[2], 32, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(32, 4, 1))

    def forward(self, x):
        return self.head(self.res3(self.res2(self.res1(self.in_ds(x)))))


def _classes(seq):
    return [type(m) for m in seq]


def _same_state(a, before):
    after = a.state_dict()
    return list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)


def test_convert_takes_the_shortcut_convolutions_and_nothing_else():
    torch.manual_seed(5)
    net = Encoder()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    assert C1.convert(net) == 2                                                        # res2[0] and res3[0]; res1[0] is 32 -> 32: no shortcut layer
    for blk, stride in ((net.res2[0], (2, 2)), (net.res3[0], (2, 2))):
        assert _classes(blk.downsample) == [C1.FusedConv1x1, nn.GroupNorm] and blk.downsample[0].stride == stride
        assert blk.downsample[1] is blk.norm3
        assert type(blk.conv1) is nn.Conv2d and type(blk.conv2) is nn.Conv2d           # attribute convolutions of a block: left alone
    assert [n for n, m in net.named_modules() if isinstance(m, C1.FusedConv1x1)] == ["res2.0.downsample.0", "res3.0.downsample.0"]
    for blk in (net.res1[0], net.res1[1], net.res2[1], net.res3[1]):
        assert blk.downsample is None
    assert _classes(net.in_ds) == [nn.Conv2d, nn.GroupNorm, nn.ReLU] and _classes(net.head) == [nn.Conv2d, nn.ReLU, nn.Conv2d]
    assert _same_state(net, before)
    assert C1.convert(net) == 0                                                        # idempotent
    Encoder().load_state_dict(net.state_dict())                                        # and the keys load into the plain modules
    wide = Encoder(dims=(64, 96, 128))                                                 # the default widths: res1[0] has a shortcut too, stride 1
    assert C1.convert(wide) == 3 and type(wide.res1[0].downsample[0]) is C1.FusedConv1x1 and wide.res1[0].downsample[0].stride == (1, 1)
    dec = nn.Sequential(Block(192, 96), Block(96, 96))                                 # GSRegresser.decoder3
    assert C1.convert(dec) == 1 and type(dec[0].downsample[0]) is C1.FusedConv1x1


def test_convert_composes_with_groupnorm_and_conv3x3_in_any_order():
    a, b = Encoder(), Encoder()
    assert C1.convert(a) == 2 and GN.convert(a) > 0 and C3.convert(a) == 0
    assert C3.convert(b) == 0 and GN.convert(b) > 0 and C1.convert(b) == 2
    for x, y in zip(a.modules(), b.modules()):
        assert type(x) is type(y)
    assert _classes(a.res2[0].downsample) == [C1.FusedConv1x1, GN.FusedGroupNorm]
    assert list(a.state_dict()) == list(b.state_dict()) == list(Encoder().state_dict())


def test_convert_leaves_everything_else_alone():
    def untouched(m):
        want = [type(x) for x in m.modules()]
        assert C1.convert(m) == 0 and [type(x) for x in m.modules()] == want

    class Holder(nn.Module):
        def __init__(self):
            super().__init__()
            self.proj = nn.Conv2d(32, 48, 1)

    untouched(Holder())                                                                 # an attribute convolution, no Sequential
    untouched(nn.ModuleList([nn.Conv2d(32, 48, 1)]))
    untouched(nn.Conv2d(32, 48, 1))                                                     # a bare layer is in no Sequential either
    untouched(nn.Sequential(nn.Conv2d(32, 4, 1)))                                       # C_out no multiple of 16 (the heads' tails)
    untouched(nn.Sequential(nn.Conv2d(32, 40, 1)))
    untouched(nn.Sequential(nn.Conv2d(32, 144, 1)))                                     # C_out > 128
    untouched(nn.Sequential(nn.Conv2d(3, 32, 1)))                                       # C_in no multiple of 4
    untouched(nn.Sequential(nn.Conv2d(260, 32, 1)))                                     # C_in > 256
    untouched(nn.Sequential(nn.Conv2d(32, 48, 1, bias=False)))
    untouched(nn.Sequential(nn.Conv2d(32, 48, 1, stride=3)))
    untouched(nn.Sequential(nn.Conv2d(32, 48, 1, stride=(1, 2))))
    untouched(nn.Sequential(nn.Conv2d(32, 48, 1, padding=1)))
    untouched(nn.Sequential(nn.Conv2d(32, 48, 1, padding="same")))                      # a padding given as a string
    untouched(nn.Sequential(nn.Conv2d(32, 48, 1, groups=2)))
    untouched(nn.Sequential(nn.Conv2d(32, 48, 1, padding=1, padding_mode="reflect")))
    untouched(nn.Sequential(nn.Conv2d(32, 48, 3, padding=1)))
    untouched(nn.Sequential(nn.Conv2d(32, 48, (1, 3), padding=(0, 1))))

    class MyConv(nn.Conv2d):
        pass

    untouched(nn.Sequential(MyConv(32, 48, 1)))                                         # a subclass
    seq = nn.Sequential(nn.Conv2d(256, 128, 1, stride=2), nn.Conv2d(4, 16, 1, dilation=1))   # both ends of the supported set
    assert C1.convert(seq) == 2 and _classes(seq) == [C1.FusedConv1x1, C1.FusedConv1x1]


def test_the_cpu_forward_and_backward_are_torchs_bit_for_bit():
    """On CPU tensors every converted forward is the pass-through: output and all gradients equal the unconverted tree's bits."""
    torch.manual_seed(6)
    plain = Encoder()
    fused = copy.deepcopy(plain)
    assert C1.convert(fused) == 2
    x, g = torch.randn(2, 3, 32, 36), torch.randn(2, 4, 4, 5)
    assert list(A.calls) == SIXTEEN                                                     # converting creates no counter, counting does
    res = []
    for net in (plain, fused):
        xin = x.clone().requires_grad_(True)
        out = net(xin)
        out.backward(g)
        res.append([out, xin.grad] + [p.grad for p in net.parameters()])
    assert len(res[0]) == 2 + len(list(plain.parameters())) and all(torch.equal(a.detach(), b.detach()) for a, b in zip(*res))
    assert (res[1][0] != 0).any() and A.calls["conv1x1"] == 0 and A.calls["conv1x1_passthrough"] == 2
    assert list(A.calls) == SIXTEEN + OURS


def test_the_op_has_no_cpu_path():
    with pytest.raises(RuntimeError, match="GPU"):
        C1.conv1x1(torch.randn(1, 32, 4, 4), torch.randn(48, 32, 1, 1), torch.randn(48), 2)


def test_supported_and_tile():
    assert C1.supported(32, 48, 2) and C1.supported(128, 48) and C1.supported(4, 16, 1) and C1.supported(256, 128, 2)
    assert not C1.supported(32, 48, 3) and not C1.supported(32, 40) and not C1.supported(6, 16) and not C1.supported(260, 16) and not C1.supported(32, 144)
    tp, wp, parts = C1.tile()
    assert tp > 0 and wp > 0 and parts > 0 and C1.tile() == (tp, wp, parts)


def test_the_name_is_by_name_only():
    hook_run.assert_the_names(A)
    assert list(A.calls) == SIXTEEN
    assert "conv1x1" not in A.requested("all") and A.requested("all") == A.FEATURES
    for other in ("groupnorm", "resblock", "stemconv", "gshead", "conv3x3", "all,groupnorm,splat", "resblock,stemconv,gshead,conv3x3"):
        assert "conv1x1" not in A.requested(other)
    A.restore()
    assert list(A.calls) == SIXTEEN
    assert A.requested("conv1x1") == ("conv1x1",)
    assert list(A.calls) == SIXTEEN + OURS and A.calls["conv1x1"] == 0 == A.calls["conv1x1_passthrough"]
    assert A.requested("all,conv1x1") == A.FEATURES + ("conv1x1",)
    assert A.requested("conv1x1,conv3x3,resblock") == ("resblock", "conv3x3", "conv1x1")       # after BY_NAME, whatever the order given
    assert list(A.calls) == SIXTEEN + OURS + ["conv3x3", "conv3x3_passthrough"]                # counters in the order they were first asked for
    with pytest.raises(ValueError):
        A.requested("conv1x1s")
    with pytest.raises(ValueError):
        A.requested("conv1")
    A.restore()
    assert list(A.calls) == SIXTEEN
    # the table: the two constructors, filed under whichever requested name comes first in their rows
    rows = lambda feats: {f: [m + "." + a for m, a, _ in r] for f, r in A._table(feats).items()}
    inits = ["core.extractor.ResidualBlock.__init__", "core.extractor.UnetExtractor.__init__"]
    assert rows(("conv1x1",)) == {"conv1x1": inits}
    assert rows(("groupnorm", "conv1x1")) == {"groupnorm": inits, "conv1x1": []}
    assert rows(("stemconv", "conv1x1")) == {"stemconv": [inits[1]], "conv1x1": [inits[0]]}
    assert rows(("conv3x3",)) == {"conv3x3": ["lib.gs_parm_network.GSRegresser.__init__"]}


def test_a_process_that_never_asks_keeps_todays_sixteen_keys():
    code = ("import sys, json; sys.path.insert(0, %r); import gps_gaussian_amd; from gps_gaussian_amd import accelerate as A, conv1x1\n"
            "a = list(A.calls); A.requested('all'); A.requested('gshead'); b = list(A.calls); A.requested('all,conv3x3'); c = list(A.calls)\n"
            "A.requested('conv1x1,all'); d = list(A.calls)\n"
            "print(json.dumps([a, b, c, d]))" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    a, b, c, d = json.loads(out.stdout.strip().splitlines()[-1])
    assert a == SIXTEEN and b == SIXTEEN and c == SIXTEEN + ["conv3x3", "conv3x3_passthrough"] and d == c + OURS
