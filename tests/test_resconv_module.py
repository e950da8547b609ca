"""CPU: resconv.convert / FusedResConv3x3 as modules -- which layers are converted (22 in a stage-2 depth encoder plus decoders, the stride-2
conv1s untouched), classes and state_dict keys unchanged, idempotence, composition with every other conversion of the package in any order, the
pass-through computing the SAME function as the plain layer bit for bit (a CPU tensor, autocast, bias=False) with the counters moving, the hook's
table of names left alone, and the op refusing CPU tensors.  Stand-in blocks written here; the reference's own classes where a checkout is
present (hook_run.needs_ref)."""
import copy
import itertools

import pytest
import torch
from torch import nn

import gps_gaussian_amd
from gps_gaussian_amd import accelerate as A
from gps_gaussian_amd import conv1x1, conv3x3, groupnorm, gshead, resconv, stemconv, upcat

import hook_run


@pytest.fixture(autouse=True)
def _built():
    gps_gaussian_amd.build()
    before = dict(resconv.calls)
    yield
    resconv.calls.update(before)
    A.restore()          # the by-name counters other converted layers created


class Block(nn.Module):
    """core/extractor.py:6-60, ResidualBlock with norm_fn 'group': the 3x3 convolutions as attributes, the shortcut a Sequential."""

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
    """core/extractor.py:63-91, UnetExtractor."""

    def __init__(self, in_channel, dims):
        super().__init__()
        self.in_ds = nn.Sequential(nn.Conv2d(in_channel, 32, 5, stride=2, padding=2), nn.GroupNorm(8, 32), nn.ReLU(inplace=True))
        self.res1 = nn.Sequential(Block(32, dims[0]), Block(dims[0], dims[0]))
        self.res2 = nn.Sequential(Block(dims[0], dims[1], stride=2), Block(dims[1], dims[1]))
        self.res3 = nn.Sequential(Block(dims[1], dims[2], stride=2), Block(dims[2], dims[2]))

    def forward(self, x):
        x1 = self.res1(self.in_ds(x))
        x2 = self.res2(x1)
        return x1, x2, self.res3(x2)


def _head(dim, cout, act=None):
    layers = [nn.Conv2d(dim, dim, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(dim, cout, 1)]
    return nn.Sequential(*(layers + ([act] if act is not None else [])))


class Regresser(nn.Module):
    """lib/gs_parm_network.py:7-81 with config/stage2.yaml's widths."""
    RGB, DEPTH, DEC, HEAD = (32, 48, 96), (32, 48, 96), (48, 64, 96), 32

    def __init__(self):
        super().__init__()
        r, d, dec = self.RGB, self.DEPTH, self.DEC
        self.depth_encoder = Encoder(1, d)
        self.decoder3 = nn.Sequential(Block(r[2] + d[2], dec[2]), Block(dec[2], dec[2]))
        self.decoder2 = nn.Sequential(Block(r[1] + d[1] + dec[2], dec[1]), Block(dec[1], dec[1]))
        self.decoder1 = nn.Sequential(Block(r[0] + d[0] + dec[1], dec[0]), Block(dec[0], dec[0]))
        self.up = nn.Upsample(scale_factor=2, mode="bilinear")
        self.out_conv = nn.Conv2d(dec[0] + 3 + 1, self.HEAD, 3, padding=1)
        self.out_relu = nn.ReLU(inplace=True)
        self.rot_head = _head(self.HEAD, 4)
        self.scale_head = _head(self.HEAD, 3, nn.Softplus(beta=100))
        self.opacity_head = _head(self.HEAD, 1, nn.Sigmoid())

    def forward(self, img, depth, img_feat):
        i1, i2, i3 = img_feat
        d1, d2, d3 = self.depth_encoder(depth)
        x = self.decoder3(torch.cat([i3, d3], 1))
        x = self.decoder2(torch.cat([self.up(x), torch.cat([i2, d2], 1)], 1))
        x = self.decoder1(torch.cat([self.up(x), torch.cat([i1, d1], 1)], 1))
        x = self.out_relu(self.out_conv(torch.cat([self.up(x), img, depth], 1)))
        return nn.functional.normalize(self.rot_head(x), dim=1), torch.clamp_max(self.scale_head(x), 0.01), self.opacity_head(x)


def _inputs(seed=0, N=1, H=16, W=24):
    g = torch.Generator().manual_seed(seed)
    new = lambda c, s: torch.randn(N, c, H // s, W // s, generator=g)
    return new(3, 1), new(1, 1), [new(c, s) for c, s in zip(Regresser.RGB, (2, 4, 8))]


def _fused_names(m):
    return sorted(n for n, x in m.named_modules() if type(x) is resconv.FusedResConv3x3)


BLOCKS = ["depth_encoder.res1.0", "depth_encoder.res1.1", "depth_encoder.res2.0", "depth_encoder.res2.1", "depth_encoder.res3.0",
          "depth_encoder.res3.1", "decoder3.0", "decoder3.1", "decoder2.0", "decoder2.1", "decoder1.0", "decoder1.1"]
STRIDE2 = ["depth_encoder.res2.0.conv1", "depth_encoder.res3.0.conv1"]
TWENTY_TWO = sorted(n for n in (b + "." + c for b in BLOCKS for c in ("conv1", "conv2")) if n not in STRIDE2)


def test_convert_takes_the_22_stride_1_layers_of_a_stage_2_regresser():
    torch.manual_seed(3)
    m = Regresser()
    plain = copy.deepcopy(m)
    keys = list(m.state_dict())
    holder = nn.ModuleDict({"regresser": m})
    assert len(TWENTY_TWO) == 22
    assert resconv.convert(holder) == 22
    assert _fused_names(m) == TWENTY_TWO
    for name in STRIDE2:                                                             # stride 2: left alone
        conv = m.get_submodule(name)
        assert type(conv) is nn.Conv2d and conv.stride == (2, 2)
    widths = sorted(set((c.in_channels, c.out_channels) for c in m.modules() if type(c) is resconv.FusedResConv3x3))
    assert widths == [(32, 32), (48, 48), (64, 64), (96, 96), (128, 48), (192, 64), (192, 96)]
    assert resconv.convert(holder) == 0 and resconv.convert(m) == 0 and resconv.convert(m.decoder2[0]) == 0        # idempotent
    # nothing else changed class: the shortcut's 1x1, the stem, out_conv, the heads (all in Sequentials or no block members), norms, blocks
    for (n, a), (_, b) in zip(m.named_modules(), plain.named_modules()):
        assert type(a) is type(b) or n in TWENTY_TWO, n
    sd, ref = m.state_dict(), plain.state_dict()
    assert list(sd) == keys == list(ref) and all(torch.equal(sd[k], ref[k]) for k in keys)
    Regresser().load_state_dict(sd)                                                  # and the keys load into the plain modules
    twin = copy.deepcopy(m)
    assert _fused_names(twin) == TWENTY_TWO and resconv.convert(twin) == 0


def test_convert_leaves_everything_else_alone():
    def untouched(m):
        want = [type(x) for x in m.modules()]
        assert resconv.convert(m) == 0 and [type(x) for x in m.modules()] == want

    untouched(nn.Sequential(nn.Conv2d(32, 32, 3, padding=1), nn.ReLU()))             # a Sequential slot (conv3x3.convert's)
    untouched(nn.Conv2d(32, 32, 3, padding=1))

    class Holder(nn.Module):                                                         # conv1 and conv2, but no norms: no residual block
        def __init__(self):
            super().__init__()
            self.conv1, self.conv2 = nn.Conv2d(32, 32, 3, padding=1), nn.Conv2d(32, 32, 3, padding=1)

    untouched(Holder())

    class Named(nn.Sequential):                                                      # block members on an nn.Sequential: left alone
        def __init__(self):
            super().__init__()
            self.conv1, self.norm1 = nn.Conv2d(32, 32, 3, padding=1), nn.GroupNorm(4, 32)
            self.conv2, self.norm2 = nn.Conv2d(32, 32, 3, padding=1), nn.GroupNorm(4, 32)

    untouched(Named())

    class MyConv(nn.Conv2d):
        pass

    def block(conv1, conv2=None, planes=32):
        b = Block(32, planes)
        b.conv1 = conv1
        if conv2 is not None:
            b.conv2 = conv2
        return b

    for conv in (nn.Conv2d(32, 32, 3, padding=1, bias=False), nn.Conv2d(32, 32, 3, padding=1, stride=2), nn.Conv2d(32, 32, 3, padding=2, dilation=2),
                 nn.Conv2d(32, 32, 3, padding=1, groups=2), nn.Conv2d(32, 32, 3, padding=1, padding_mode="reflect"), nn.Conv2d(32, 32, 5, padding=2),
                 nn.Conv2d(32, 32, 3, padding="same"), nn.Conv2d(32, 32, 3, padding=0), nn.Conv2d(6, 32, 3, padding=1), nn.Conv2d(196, 32, 3, padding=1),
                 MyConv(32, 32, 3, padding=1)):
        b = block(conv)
        assert resconv.convert(b) == 1 and type(b.conv1) is type(conv) and type(b.conv2) is resconv.FusedResConv3x3
    for planes in (24, 112):                                                         # C_out no multiple of 16 / above 96
        b = Block(32, planes)
        assert resconv.convert(b) == 0
    b = Block(4, 16)                                                                 # both low ends of the supported set
    b.norm1, b.norm2 = nn.Identity(), nn.BatchNorm2d(16)                             # the members are recognised by name, whatever the norm is
    assert resconv.convert(b) == 2
    shared = Block(32, 32)
    both = nn.ModuleList([shared, shared])                                           # reachable twice: converted once
    assert resconv.convert(both) == 2


_OTHERS = (("groupnorm", groupnorm.convert), ("gn_relu", groupnorm.fuse_sequential_relu), ("conv1x1", conv1x1.convert), ("stemconv", stemconv.convert),
           ("gshead", gshead.convert), ("conv3x3", conv3x3.convert_regresser), ("upcat", upcat.convert))


def _orders():
    """ours first, ours last, ours in the middle of the others reversed, and ours between every neighbouring pair of a rotation"""
    names = [n for n, _ in _OTHERS]
    yield ["resconv"] + names
    yield names + ["resconv"]
    for k in range(1, len(names)):
        rot = names[k:] + names[:k]
        yield rot[:k] + ["resconv"] + rot[k:]
    yield names[::-1][:3] + ["resconv"] + names[::-1][3:]


@pytest.fixture(scope="module")
def _reference_run():
    torch.manual_seed(2)
    plain = Regresser()
    args = _inputs(seed=6)
    with torch.no_grad():
        want = plain(*args)
    return plain, args, want


@pytest.mark.parametrize("order", list(_orders()), ids=lambda o: "-".join(o))
def test_convert_composes_with_every_other_conversion_in_any_order(order, _reference_run):
    plain, args, want = _reference_run
    m = copy.deepcopy(plain)
    keys = list(m.state_dict())
    fns = dict(_OTHERS, resconv=resconv.convert)
    counts = {n: fns[n](m) for n in order}
    assert counts["resconv"] == 22 and _fused_names(m) == TWENTY_TWO
    assert counts["conv1x1"] == 5 and counts["stemconv"] == 1 and counts["gshead"] == 3 and counts["conv3x3"] == 4 and counts["upcat"] == 1
    assert counts["groupnorm"] + counts["gn_relu"] > 0 and all(fns[n](m) == 0 for n in order)
    assert type(m.decoder3[0].downsample[0]) is conv1x1.FusedConv1x1 and type(m.out_conv) is conv3x3.FusedConv3x3
    assert isinstance(m.decoder1[1].norm1, groupnorm.FusedGroupNorm) and type(m.depth_encoder.in_ds[0]) is stemconv.FusedStemConv2d
    assert m.forward.__func__ is upcat.regresser_forward
    assert list(m.state_dict()) == keys
    resconv.calls.update(resconv=0, resconv_passthrough=0)
    with torch.no_grad():
        got = m(*args)
    assert all(torch.equal(g, w) for g, w in zip(got, want))                         # on the CPU every converted layer passes through
    assert resconv.calls == {"resconv": 0, "resconv_passthrough": 22}


def test_both_block_forwards_reach_the_converted_layers():
    """The block's own forward and groupnorm.residual_block_forward call block.conv1(x) and block.conv2(y)."""
    torch.manual_seed(4)
    plain = Block(32, 48)
    b = copy.deepcopy(plain)
    assert resconv.convert(b) == 2
    x = torch.randn(1, 32, 9, 11)
    resconv.calls.update(resconv=0, resconv_passthrough=0)
    want = plain(x.clone())
    assert torch.equal(b(x.clone()), want) and resconv.calls["resconv_passthrough"] == 2
    assert torch.equal(groupnorm.residual_block_forward(b, x.clone()), want) and resconv.calls["resconv_passthrough"] == 4
    assert groupnorm.convert(b) == 3
    assert torch.equal(groupnorm.residual_block_forward(b, x.clone()), want) and resconv.calls == {"resconv": 0, "resconv_passthrough": 6}


def _pair(**kw):
    torch.manual_seed(7)
    plain = nn.Conv2d(32, 48, 3, padding=1, **kw)
    fused = copy.deepcopy(plain)
    fused.__class__ = resconv.FusedResConv3x3
    return plain, fused


def _passes_through(plain, fused, x, grads=True, **autocast):
    n0, p0 = resconv.calls["resconv"], resconv.calls["resconv_passthrough"]
    res = []
    for layer in (plain, fused):
        xin = x.clone().requires_grad_(grads)
        with torch.autocast("cpu", enabled=bool(autocast), **autocast):
            y = layer(xin)
        if grads:
            y.float().square().sum().backward()
        res.append([y.detach()] + ([xin.grad] + [p.grad for p in layer.parameters()] if grads else []))
    assert resconv.calls["resconv"] == n0 and resconv.calls["resconv_passthrough"] == p0 + 1
    for a, b in zip(*res):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    return res[1][0]


def test_the_pass_through_is_the_plain_layer_bit_for_bit():
    x = torch.randn(2, 32, 10, 13, generator=torch.Generator().manual_seed(8))
    plain, fused = _pair()
    assert _passes_through(plain, fused, x).dtype == torch.float32                   # a CPU tensor
    assert _passes_through(plain, fused, x, dtype=torch.bfloat16).dtype == torch.bfloat16   # autocast
    plain, fused = _pair(bias=False)
    _passes_through(plain, fused, x)                                                 # bias=False
    with torch.no_grad():
        _passes_through(plain, fused, x, grads=False)
    plain, fused = _pair(stride=2)
    _passes_through(plain, fused, x)                                                 # a stride-2 layer force-swapped
    assert set(resconv.calls) == {"resconv", "resconv_passthrough"}


def test_the_hooks_names_and_counters_are_untouched():
    keys = list(A.calls)
    m = Regresser()
    assert resconv.convert(m) == 22
    with torch.no_grad():
        m(*_inputs())
    hook_run.assert_the_names(A)
    assert list(A.calls) == keys and "resconv" not in A.calls and "resconv" not in A.NAMES
    assert set(resconv.calls) == {"resconv", "resconv_passthrough"}


def test_the_op_refuses_cpu_tensors():
    x, w, b = torch.randn(1, 32, 4, 4), torch.randn(48, 32, 3, 3), torch.randn(48)
    for args in ((x, w, b), (x.clone().requires_grad_(True), w, b)):
        with pytest.raises(RuntimeError, match="GPU"):
            resconv.conv3x3(*args)


def test_supported_and_tile():
    assert all(resconv.supported(*p) for p in ((32, 32), (48, 48), (64, 64), (96, 96), (128, 48), (192, 64), (192, 96), (4, 16), (100, 80)))
    assert not any(resconv.supported(*p) for p in ((0, 32), (3, 32), (196, 32), (32, 0), (32, 24), (32, 112), (6, 16)))
    th, tw = resconv.tile()
    assert th > 0 and tw > 0 and resconv.tile() == (th, tw)


_REF_BODY = """
    import types, torch
    from torch import nn
    import corr_sampler                                    # the drop-in
    import core.extractor as E
    import lib.gs_parm_network as G
    from gps_gaussian_amd import resconv, groupnorm, accelerate as A
    dims = [32, 48, 96]
    cfg = types.SimpleNamespace(raft=types.SimpleNamespace(encoder_dims=dims),
                                gsnet=types.SimpleNamespace(encoder_dims=dims, decoder_dims=[48, 64, 96], parm_head_dim=32))
    torch.manual_seed(11)
    net = G.GSRegresser(cfg)
    keys = list(net.state_dict())
    torch.manual_seed(12)
    img, depth = torch.randn(1, 3, 32, 32), torch.rand(1, 1, 32, 32)
    enc = E.UnetExtractor(in_channel=3, encoder_dim=dims)
    with torch.no_grad():
        feats = enc(img)
        want = net(img, depth, feats)
    print('ref', 'CONVERTED', resconv.convert(net), resconv.convert(net), resconv.convert(enc))
    fused = sorted(n for n, m in net.named_modules() if type(m) is resconv.FusedResConv3x3)
    print('ref', 'FUSED', len(fused), 'depth_encoder.res2.0.conv1' in fused, 'depth_encoder.res3.0.conv1' in fused, 'decoder3.0.conv1' in fused)
    print('ref', 'STRIDE2', type(net.depth_encoder.res2[0].conv1).__name__, type(net.depth_encoder.res3[0].conv1).__name__)
    print('ref', 'KEYS', list(net.state_dict()) == keys)
    with torch.no_grad():
        got = net(img, depth, feats)
    print('ref', 'SAME', all(torch.equal(a, b) for a, b in zip(got, want)), resconv.calls)
    groupnorm.convert(net)
    for blk in net.modules():
        if isinstance(blk, E.ResidualBlock):
            blk.forward = types.MethodType(groupnorm.residual_block_forward, blk)
    resconv.calls.update(resconv=0, resconv_passthrough=0)
    with torch.no_grad():
        got = net(img, depth, feats)
    print('ref', 'SAME_RB', all(torch.equal(a, b) for a, b in zip(got, want)), resconv.calls)
    print('ref', 'NAMES', 'resconv' in A.NAMES, len(A.calls))
"""


@hook_run.needs_ref
def test_the_references_own_regresser(tmp_path):
    out = hook_run.run(_REF_BODY, None, tmp_path)
    assert "ref CONVERTED 22 0 10" in out                                            # the image encoder in fp32 (stage 1): 10 more
    assert "ref FUSED 22 False False True" in out and "ref STRIDE2 Conv2d Conv2d" in out and "ref KEYS True" in out
    assert "ref SAME True {'resconv': 0, 'resconv_passthrough': 22}" in out
    assert "ref SAME_RB True {'resconv': 0, 'resconv_passthrough': 22}" in out
    assert "ref NAMES False 16" in out
