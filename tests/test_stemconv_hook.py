"""CPU: GPSGS_ACCELERATE=stemconv makes the reference's UNMODIFIED core/extractor.py build its stem convolution as a FusedStemConv2d, and the
constructor wrapper it shares with `groupnorm` / `resblock` does only what was asked.

Each case runs in a fresh interpreter with the integration path, the harness of hook_run.py; they skip where there is no reference
checkout."""
import hook_run as H

# builds UnetExtractor as both encoders do, prints the classes of its stem, of every norm and convolution, and the state_dict keys
_BODY = """
    import torch
    from torch import nn
    import corr_sampler                                    # the drop-in: where the hook installs itself
    import core.extractor as E
    import gps_gaussian_amd.accelerate as A
    torch.manual_seed(11)
    name = lambda m: type(m).__module__.split('.')[-1] + '.' + type(m).__name__
    for tag, cin in (('image', 3), ('depth', 1)):
        unet = E.UnetExtractor(in_channel=cin, encoder_dim=[16, 24, 32])
        print(tag, 'STEM', [name(m) for m in unet.in_ds])
        print(tag, 'NORMS', sorted(set(name(m) for m in unet.modules() if isinstance(m, nn.GroupNorm))))
        print(tag, 'CONVS', sum(type(m) is nn.Conv2d for m in unet.modules()), sum(name(m) == 'stemconv.FusedStemConv2d' for m in unet.modules()))
        print(tag, 'KEYS', ','.join(unet.state_dict().keys()))
        with torch.no_grad():
            unet(torch.randn(1, cin, 32, 32))
    block = E.ResidualBlock(16, 24, norm_fn='group', stride=2)
    print('block', 'NORMS', sorted(set(name(m) for m in block.modules() if isinstance(m, nn.GroupNorm))))
    print('CALLS', A.calls['stemconv'], A.calls['stemconv_passthrough'])
    print('INSTALLED', sorted((k, v) for k, v in A.installed().items() if k.startswith('core.extractor.')))
"""

_UNET, _BLOCK = "core.extractor.UnetExtractor.__init__", "core.extractor.ResidualBlock.__init__"
_PLAIN_STEM = "['conv.Conv2d', 'normalization.GroupNorm', 'activation.ReLU']"


@H.needs_ref
def test_the_shared_wrapper_does_only_what_was_asked(tmp_path):
    unset = H.run(_BODY, None, tmp_path)
    only_all = H.run(_BODY, "all", tmp_path)
    conv = H.run(_BODY, "stemconv", tmp_path)
    norm = H.run(_BODY, "groupnorm", tmp_path)
    res = H.run(_BODY, "resblock", tmp_path)
    both = H.run(_BODY, "resblock,stemconv", tmp_path)

    for out in (unset, only_all):                                    # nothing is converted
        assert len(H.lines(out, "STEM")) == 2 and all(_PLAIN_STEM in l for l in H.lines(out, "STEM"))
        assert all(l.split()[3] == "0" for l in H.lines(out, "CONVS")) and "INSTALLED []" in out and "CALLS 0 0" in out
    # stemconv alone: the convolution, and every norm still an nn.GroupNorm; only the class that has a stem is wrapped
    assert all("['stemconv.FusedStemConv2d', 'normalization.GroupNorm', 'activation.ReLU']" in l for l in H.lines(conv, "STEM"))
    assert all("['normalization.GroupNorm']" in l for l in H.lines(conv, "NORMS")) and len(H.lines(conv, "NORMS")) == 3
    assert "INSTALLED %r" % [(_UNET, "stemconv")] in conv
    assert all(l.split()[3] == "1" for l in H.lines(conv, "CONVS"))      # exactly in_ds[0] of each encoder
    calls = H.lines(conv, "CALLS")[0].split()
    assert calls[1] == "0" and calls[2] == "2"                            # CPU tensors: handed to nn.Conv2d.forward, and counted
    # groupnorm or resblock alone: in_ds[0] stays a plain nn.Conv2d, exactly as before
    assert all("['conv.Conv2d', 'groupnorm.FusedGroupNorm', 'activation.ReLU']" in l for l in H.lines(norm, "STEM"))
    assert all("['conv.Conv2d', 'groupnorm.FusedGroupNormReLU', 'linear.Identity']" in l for l in H.lines(res, "STEM"))
    for out in (norm, res):
        assert all(l.split()[3] == "0" for l in H.lines(out, "CONVS")) and "CALLS 0 0" in out
    assert "INSTALLED %r" % [(_BLOCK, "groupnorm"), (_UNET, "groupnorm")] in norm
    # both
    assert all("['stemconv.FusedStemConv2d', 'groupnorm.FusedGroupNormReLU', 'linear.Identity']" in l for l in H.lines(both, "STEM"))
    assert all("normalization.GroupNorm" not in l for l in H.lines(both, "NORMS"))
    # the same layers under the same names everywhere
    keys = [H.lines(o, "KEYS") for o in (unset, only_all, conv, norm, res, both)]
    assert all(k == keys[0] for k in keys) and len(keys[0]) == 2
    n_convs = [int(l.split()[2]) + int(l.split()[3]) for l in H.lines(unset, "CONVS")]
    for out in (conv, both):
        assert [int(l.split()[2]) + int(l.split()[3]) for l in H.lines(out, "CONVS")] == n_convs
