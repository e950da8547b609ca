"""CPU: GPSGS_ACCELERATE=groupnorm makes the reference's UNMODIFIED core/extractor.py build FusedGroupNorm layers (accelerate.py wraps the two
constructors, the reference's forward bodies run as they are); "all" alone converts nothing.

Each case runs in a fresh interpreter with the integration path, the harness of hook_run.py; they skip where there is no reference
checkout."""
import hook_run as H

# builds the two classes, prints the class names of their GroupNorm layers, the state_dict keys and a digest of a seeded CPU forward
_BODY = """
    import hashlib, torch
    from torch import nn
    import corr_sampler                                    # the drop-in: where the hook installs itself
    import core.extractor as E
    import gps_gaussian_amd.accelerate as A
    torch.manual_seed(11)
    unet = E.UnetExtractor(in_channel=3, encoder_dim=[16, 24, 32])
    block = E.ResidualBlock(16, 24, norm_fn='group', stride=2)      # stride 2: the block builds norm3 for its downsample path
    assert hasattr(block, 'norm3')
    for name, net in (('unet', unet), ('block', block)):
        norms = [type(m).__module__.split('.')[-1] + '.' + type(m).__name__ for m in net.modules() if isinstance(m, nn.GroupNorm)]
        print(name, 'NORMS', len(norms), sorted(set(norms)))
        print(name, 'KEYS', ','.join(net.state_dict().keys()))
    torch.manual_seed(12)
    with torch.no_grad():
        outs = unet(torch.randn(1, 3, 32, 32))
        outs = list(outs) if isinstance(outs, (tuple, list)) else [outs]
        outs.append(block(torch.randn(1, 16, 16, 16)))
    h = hashlib.sha256()
    for o in outs:
        h.update(o.contiguous().numpy().tobytes())
    print('DIGEST', h.hexdigest())
    print('CALLS', A.calls['groupnorm'], A.calls['groupnorm_passthrough'])
    print('INSTALLED', sorted(k for k, v in A.installed().items() if v == 'groupnorm'))
"""


@H.needs_ref
def test_groupnorm_converts_the_extractor_and_all_alone_does_not(tmp_path):
    plain = H.run(_BODY, None, tmp_path)
    fused = H.run(_BODY, "groupnorm", tmp_path)
    only_all = H.run(_BODY, "all", tmp_path)
    both = H.run(_BODY, "all,groupnorm", tmp_path)

    for out in (plain, only_all):
        norms = H.lines(out, "NORMS")
        assert len(norms) == 2 and all("['normalization.GroupNorm']" in l for l in norms), norms
        assert "INSTALLED []" in out and "CALLS 0 0" in out
    for out in (fused, both):
        norms = H.lines(out, "NORMS")
        assert len(norms) == 2 and all("['groupnorm.FusedGroupNorm']" in l for l in norms), norms          # every one, norm3 included
        assert "INSTALLED ['core.extractor.ResidualBlock.__init__', 'core.extractor.UnetExtractor.__init__']" in out
        calls = H.lines(out, "CALLS")[0].split()
        assert calls[1] == "0" and int(calls[2]) > 0        # CPU tensors: every forward was handed to nn.GroupNorm.forward, and counted
    # the same number of GroupNorm layers, the same state_dict keys, the same bits
    assert H.lines(plain, "NORMS")[0].split()[2] == H.lines(fused, "NORMS")[0].split()[2] != "0"
    assert H.lines(plain, "KEYS") == H.lines(fused, "KEYS") == H.lines(only_all, "KEYS") == H.lines(both, "KEYS") and len(H.lines(plain, "KEYS")) == 2
    assert H.lines(plain, "DIGEST") == H.lines(fused, "DIGEST") == H.lines(only_all, "DIGEST") == H.lines(both, "DIGEST") and len(H.lines(plain, "DIGEST")) == 1
