"""CPU: GPSGS_ACCELERATE=gshead makes the reference's UNMODIFIED lib/gs_parm_network.py build the tails of its three heads as FusedHeadConv, and
nothing else; every other value of the variable leaves the heads exactly as the reference builds them.

Each case runs in a fresh interpreter with the integration path, the harness of hook_run.py; they skip where there is no reference
checkout."""
import hook_run as H

# builds GSRegresser from a small cfg (dims [16, 24, 32], head dim 16), prints the classes of its heads, of the norms and of the stem, the state_dict
# keys, a digest of the parameters and of a seeded CPU forward, the counters and what was rebound
_BODY = """
    import hashlib, types, torch
    from torch import nn
    import corr_sampler                                    # the drop-in: where the hook installs itself
    import core.extractor as E
    import lib.gs_parm_network as G
    import gps_gaussian_amd.accelerate as A
    dims = [16, 24, 32]
    cfg = types.SimpleNamespace(raft=types.SimpleNamespace(encoder_dims=dims),
                                gsnet=types.SimpleNamespace(encoder_dims=dims, decoder_dims=dims, parm_head_dim=16))
    name = lambda m: type(m).__module__.split('.')[-1] + '.' + type(m).__name__
    torch.manual_seed(11)
    net = G.GSRegresser(cfg)
    for head in ('rot_head', 'scale_head', 'opacity_head'):
        print(head, 'HEAD', [name(m) for m in getattr(net, head)])
    print('net', 'NORMS', sorted(set(name(m) for m in net.modules() if isinstance(m, nn.GroupNorm))))
    print('net', 'STEM', [name(m) for m in net.depth_encoder.in_ds])
    print('net', 'FUSED', sum(name(m) == 'gshead.FusedHeadConv' for m in net.modules()), sum(isinstance(m, nn.Conv2d) for m in net.modules()))
    print('net', 'KEYS', ','.join(net.state_dict().keys()))
    h = hashlib.sha256()
    for v in net.state_dict().values():
        h.update(v.contiguous().numpy().tobytes())
    print('net', 'PARAMS', h.hexdigest())
    torch.manual_seed(12)
    img, depth = torch.randn(1, 3, 32, 32), torch.rand(1, 1, 32, 32)
    with torch.no_grad():
        feats = E.UnetExtractor(in_channel=3, encoder_dim=dims)(img)
        outs = net(img, depth, feats)
    h = hashlib.sha256()
    for o in outs:
        h.update(o.contiguous().numpy().tobytes())
    print('net', 'DIGEST', [tuple(o.shape) for o in outs], h.hexdigest())
    print('CALLS', A.calls['gshead'], A.calls['gshead_passthrough'])
    print('INSTALLED', sorted(A.installed().items()))
"""

_INIT = "lib.gs_parm_network.GSRegresser.__init__"
_PLAIN = {"rot_head": "['conv.Conv2d', 'activation.ReLU', 'conv.Conv2d']",
          "scale_head": "['conv.Conv2d', 'activation.ReLU', 'conv.Conv2d', 'activation.Softplus']",
          "opacity_head": "['conv.Conv2d', 'activation.ReLU', 'conv.Conv2d', 'activation.Sigmoid']"}
_FUSED = {"rot_head": "['conv.Conv2d', 'linear.Identity', 'gshead.FusedHeadConv']",
          "scale_head": "['conv.Conv2d', 'linear.Identity', 'gshead.FusedHeadConv', 'linear.Identity']",
          "opacity_head": "['conv.Conv2d', 'linear.Identity', 'gshead.FusedHeadConv', 'linear.Identity']"}


def _heads(out):
    return {l.split()[0]: l.split("HEAD ", 1)[1] for l in H.lines(out, "HEAD")}


@H.needs_ref
def test_gshead_converts_the_heads_and_nothing_else_does(tmp_path):
    runs = {v: H.run(_BODY, v, tmp_path) for v in (None, "all", "groupnorm", "resblock", "stemconv", "gshead", "resblock,stemconv,gshead")}

    for v in (None, "all", "groupnorm", "resblock", "stemconv"):                      # nothing of the heads changes
        out = runs[v]
        assert _heads(out) == _PLAIN, v
        assert H.lines(out, "FUSED")[0].split()[2] == "0" and "CALLS 0 0" in out and _INIT not in out, v
    assert "INSTALLED []" in runs[None] and "INSTALLED []" in runs["all"]

    out = runs["gshead"]                                                               # gshead alone: the three tails, and only them
    assert _heads(out) == _FUSED
    assert "INSTALLED %r" % [(_INIT, "gshead")] in out
    assert "NORMS ['normalization.GroupNorm']" in out                                  # every norm is still nn.GroupNorm
    assert "STEM ['conv.Conv2d', 'normalization.GroupNorm', 'activation.ReLU']" in out    # in_ds[0] is a plain Conv2d
    assert H.lines(out, "FUSED")[0].split()[2] == "3"
    assert "CALLS 0 3" in out                                                          # a CPU forward: three pass-throughs, counted

    out = runs["resblock,stemconv,gshead"]                                             # composes with the encoder's opt-ins
    assert _heads(out) == _FUSED and "CALLS 0 3" in out
    assert "STEM ['stemconv.FusedStemConv2d', 'groupnorm.FusedGroupNormReLU', 'linear.Identity']" in out
    assert "normalization.GroupNorm" not in H.lines(out, "NORMS")[0]
    assert "(%r, 'gshead')" % _INIT in out and "core.extractor.UnetExtractor.__init__" in out and "core.extractor.ResidualBlock.forward" in out

    # the same layers under the same names, the same parameters, the same number of convolutions everywhere; the same output bits wherever every
    # forward was torch's own (the pass-through applies the ReLU and the activation itself)
    for tag in ("KEYS", "PARAMS"):
        lines = [H.lines(o, tag) for o in runs.values()]
        assert all(l == lines[0] for l in lines) and len(lines[0]) == 1, tag
    assert len({H.lines(o, "FUSED")[0].split()[3] for o in runs.values()}) == 1
    assert H.lines(runs["gshead"], "DIGEST") == H.lines(runs[None], "DIGEST") == H.lines(runs["all"], "DIGEST") == H.lines(runs["stemconv"], "DIGEST")
    assert len(H.lines(runs[None], "DIGEST")) == 1
