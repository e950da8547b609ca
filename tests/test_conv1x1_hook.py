"""CPU: GPSGS_ACCELERATE=conv1x1 makes the reference's UNMODIFIED core/extractor.py build `downsample[0]` of every ResidualBlock that has a shortcut
as a FusedConv1x1 -- in the encoders and in the regresser's decoders (lib/gs_parm_network.py builds them from the same class) -- and nothing else;
no other name does; it composes with the other opt-ins of the same constructors.

Each case runs in a fresh interpreter with the integration path, the harness of hook_run.py; they skip where there is no reference
checkout."""
import hook_run as H

# builds UnetExtractor and GSRegresser with config/stage2.yaml's widths, prints for every ResidualBlock whether it has a shortcut and the classes in
# it, every FusedConv1x1 by name, every other module class, the state_dict keys, a digest of the parameters and of a seeded CPU forward, the counters
# and what was rebound
_BODY = """
    import hashlib, types, torch
    from torch import nn
    import corr_sampler                                    # the drop-in: where the hook installs itself
    import core.extractor as E
    import lib.gs_parm_network as G
    import gps_gaussian_amd.accelerate as A
    dims = [32, 48, 96]
    cfg = types.SimpleNamespace(raft=types.SimpleNamespace(encoder_dims=dims),
                                gsnet=types.SimpleNamespace(encoder_dims=dims, decoder_dims=[48, 64, 96], parm_head_dim=32))
    name = lambda m: type(m).__module__.split('.')[-1] + '.' + type(m).__name__
    torch.manual_seed(11)
    enc = E.UnetExtractor(in_channel=3, encoder_dim=dims)
    net = G.GSRegresser(cfg)
    for tag, root in (('enc', enc), ('net', net)):
        for n, m in root.named_modules():
            if isinstance(m, E.ResidualBlock):
                print(tag, 'BLOCK', n, 'none' if m.downsample is None else [name(x) for x in m.downsample])
        print(tag, 'FUSED', sorted(n for n, m in root.named_modules() if name(m) == 'conv1x1.FusedConv1x1'))
        print(tag, 'OTHERS', sorted(set(name(m) for m in root.modules() if name(m) != 'conv1x1.FusedConv1x1')))
        print(tag, 'KEYS', ','.join(root.state_dict().keys()))
        h = hashlib.sha256()
        for v in root.state_dict().values():
            h.update(v.contiguous().numpy().tobytes())
        print(tag, 'PARAMS', h.hexdigest())
    torch.manual_seed(12)
    img, depth = torch.randn(1, 3, 32, 32), torch.rand(1, 1, 32, 32)
    with torch.no_grad():
        feats = enc(img)
        outs = net(img, depth, feats)
    h = hashlib.sha256()
    for o in list(feats) + list(outs):
        h.update(o.contiguous().numpy().tobytes())
    print('all', 'DIGEST', [tuple(o.shape) for o in outs], h.hexdigest())
    print('CALLS', A.calls.get('conv1x1'), A.calls.get('conv1x1_passthrough'))
    print('COUNTERS', len(A.calls), list(A.calls)[16:])
    print('INSTALLED', sorted(A.installed().items()))
"""

_RB, _UN, _FW = "core.extractor.ResidualBlock.__init__", "core.extractor.UnetExtractor.__init__", "core.extractor.ResidualBlock.forward"
_F1 = "conv1x1.FusedConv1x1"
# with these widths: the encoders' res2[0] and res3[0] (res1[0] is 32 -> 32: no shortcut), and the first block of each decoder
_ENC = ["res2.0.downsample.0", "res3.0.downsample.0"]
_NET = ["decoder1.0.downsample.0", "decoder2.0.downsample.0", "decoder3.0.downsample.0", "depth_encoder.res2.0.downsample.0",
        "depth_encoder.res3.0.downsample.0"]


def _blocks(out):
    """(tag, block name) -> the classes in its shortcut ('none' where it has none)"""
    return {tuple(l.split()[0:3:2]): l.split(" ", 3)[3] for l in H.lines(out, "BLOCK")}


def _first(out, tag, what):
    return [l for l in H.lines(out, what) if l.startswith(tag + " ")][0].split(what + " ", 1)[1]


@H.needs_ref
def test_conv1x1_converts_the_shortcut_convolutions_and_nothing_else_does(tmp_path):
    variants = (None, "all", "resblock", "conv1x1", "resblock,stemconv,gshead,conv3x3,conv1x1")
    runs = {v: H.run(_BODY, v, tmp_path) for v in variants}
    plain = _blocks(runs[None])
    with_shortcut = sorted(k for k, v in plain.items() if v != "none")
    assert with_shortcut == sorted([("enc", n.rsplit(".downsample", 1)[0]) for n in _ENC] + [("net", n.rsplit(".downsample", 1)[0]) for n in _NET])
    assert len(plain) == 6 + 6 + 6                                                      # six blocks in each encoder, two in each decoder

    for v in (None, "all", "resblock"):                                                 # no shortcut layer changes, no counter appears
        out = runs[v]
        assert "enc FUSED []" in out and "net FUSED []" in out, v
        assert all(c.startswith("['conv.Conv2d', ") for c in _blocks(out).values() if c != "none"), v
        assert "CALLS None None" in out and "COUNTERS 16 []" in out, v
    assert _blocks(runs["all"]) == plain
    assert "INSTALLED []" in runs[None] and "INSTALLED []" in runs["all"]
    assert "(%r, 'resblock')" % _RB in runs["resblock"] and "conv1x1" not in H.lines(runs["resblock"], "INSTALLED")[0]

    out = runs["conv1x1"]                                                               # conv1x1 alone: the shortcut layers, and only them
    assert "enc FUSED %r" % _ENC in out and "net FUSED %r" % _NET in out
    got = _blocks(out)
    assert sorted(k for k, v in got.items() if v != "none") == with_shortcut            # exactly the blocks that have a downsample
    assert all(v == str([_F1, "normalization.GroupNorm"]) for v in got.values() if v != "none")
    for tag in ("enc", "net"):                                                          # every other module is what it was
        assert _first(out, tag, "OTHERS") == _first(runs[None], tag, "OTHERS")
    assert "INSTALLED %r" % [(_RB, "conv1x1"), (_UN, "conv1x1")] in out
    assert "CALLS 0 7" in out                                                           # a CPU forward: seven pass-throughs, counted
    assert "COUNTERS 18 ['conv1x1', 'conv1x1_passthrough']" in out

    out = runs["resblock,stemconv,gshead,conv3x3,conv1x1"]                              # composes; each row is filed under its first requested name
    assert "enc FUSED %r" % _ENC in out and "net FUSED %r" % _NET in out
    got = _blocks(out)
    assert sorted(k for k, v in got.items() if v != "none") == with_shortcut
    assert all(v == str([_F1, "groupnorm.FusedGroupNorm"]) for v in got.values() if v != "none")       # downsample[1] converts independently
    assert "CALLS 0 7" in out
    assert "COUNTERS 20 ['conv3x3', 'conv3x3_passthrough', 'conv1x1', 'conv1x1_passthrough']" in out
    assert "(%r, 'resblock')" % _RB in out and "(%r, 'resblock')" % _UN in out and "(%r, 'resblock')" % _FW in out
    assert "'conv1x1')" not in H.lines(out, "INSTALLED")[0]
    assert "normalization.GroupNorm" not in _first(out, "net", "OTHERS") and "stemconv.FusedStemConv2d" in _first(out, "enc", "OTHERS")

    # the same layers under the same names, the same parameters and -- on CPU tensors every replaced forward hands on to torch -- the same output
    # bits in every variant
    for tag, n in (("KEYS", 2), ("PARAMS", 2), ("DIGEST", 1)):
        lines = [H.lines(o, tag) for o in runs.values()]
        assert all(l == lines[0] for l in lines) and len(lines[0]) == n, tag
