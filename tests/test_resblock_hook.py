"""CPU: GPSGS_ACCELERATE=resblock on the reference's UNMODIFIED core/extractor.py -- the two constructors are wrapped (conversion + the stem's fused
ReLU) and ResidualBlock.forward is rebound to groupnorm.residual_block_forward; `groupnorm` alone installs no forward; a block built with
norm_fn='batch' runs the reference's own forward.  State-dict keys and the digest of a seeded CPU forward are those of the plain run.

Each case runs in a fresh interpreter with the integration path, the harness of hook_run.py; they skip where there is no reference
checkout."""
import pytest

import hook_run as H

_BODY = """
    import hashlib, torch
    from torch import nn
    import corr_sampler                                    # the drop-in: where the hook installs itself
    import core.extractor as E
    import gps_gaussian_amd.accelerate as A
    torch.manual_seed(11)
    unet = E.UnetExtractor(in_channel=3, encoder_dim=[16, 24, 32])
    block = E.ResidualBlock(16, 24, norm_fn='group', stride=2)
    batch = E.ResidualBlock(16, 16, norm_fn='batch').eval()
    for name, net in (('unet', unet), ('block', block)):
        norms = [type(m).__module__.split('.')[-1] + '.' + type(m).__name__ for m in net.modules() if isinstance(m, nn.GroupNorm)]
        print(name, 'NORMS', len(norms), sorted(set(norms)))
        print(name, 'KEYS', ','.join(net.state_dict().keys()))
    print('STEM', [type(m).__name__ for m in unet.in_ds])
    torch.manual_seed(12)
    with torch.no_grad():
        outs = list(unet(torch.randn(1, 3, 32, 32)))
        outs.append(block(torch.randn(1, 16, 16, 16)))
        outs.append(batch(torch.randn(1, 16, 8, 8)))
    h = hashlib.sha256()
    for o in outs:
        h.update(o.contiguous().numpy().tobytes())
    print('DIGEST', h.hexdigest())
    print('CALLS', A.calls['groupnorm'], A.calls['groupnorm_passthrough'], A.calls['resblock'], A.calls['resblock_passthrough'])
    print('INSTALLED', sorted(A.installed().items()))
    print('FORWARD', E.ResidualBlock.forward.__module__)
"""

_INITS = ["core.extractor.ResidualBlock.__init__", "core.extractor.UnetExtractor.__init__"]
_FWD = "core.extractor.ResidualBlock.forward"


@H.needs_ref
def test_resblock_installs_the_forward_and_both_constructors(tmp_path):
    plain = H.run(_BODY, None, tmp_path)
    only_gn = H.run(_BODY, "groupnorm", tmp_path)
    res = H.run(_BODY, "resblock", tmp_path)
    both = H.run(_BODY, "all,groupnorm,resblock", tmp_path)

    assert "INSTALLED []" in plain and "FORWARD core.extractor" in plain and "CALLS 0 0 0 0" in plain
    # groupnorm alone: exactly the two constructors, the reference's forward bodies
    assert "INSTALLED %r" % [(k, "groupnorm") for k in _INITS] in only_gn and "FORWARD core.extractor" in only_gn
    assert "STEM ['Conv2d', 'FusedGroupNorm', 'ReLU']" in only_gn
    assert H.lines(only_gn, "CALLS")[0].split()[3:] == ["0", "0"]
    # resblock alone: the constructors under its own name, and the forward
    assert "INSTALLED %r" % sorted([(k, "resblock") for k in _INITS + [_FWD]]) in res
    # both names: one wrapper per constructor (filed under groupnorm), the forward under resblock
    got = eval(H.lines(both, "INSTALLED")[0].split(" ", 1)[1])
    assert [kv for kv in got if kv[0].startswith("core.extractor.")] == sorted([(k, "groupnorm") for k in _INITS] + [(_FWD, "resblock")])
    for out in (res, both):
        assert "FORWARD gps_gaussian_amd.accelerate" in out
        assert "STEM ['Conv2d', 'FusedGroupNormReLU', 'Identity']" in out
        norms = H.lines(out, "NORMS")
        assert len(norms) == 2 and all("groupnorm.FusedGroupNorm" in l and "normalization.GroupNorm" not in l for l in norms), norms
        calls = [int(v) for v in H.lines(out, "CALLS")[0].split()[1:]]
        # CPU tensors: no kernel ran, every norm was handed on; 6 unet blocks + 1 = 7 blocks on the new forward, the batch-norm block on the reference's
        assert calls[0] == 0 and calls[1] > 0 and calls[2] == 7 and calls[3] == 1
    # the same layers, the same state_dict keys, the same bits
    assert H.lines(plain, "NORMS")[0].split()[2] == H.lines(res, "NORMS")[0].split()[2] != "0"
    assert H.lines(plain, "KEYS") == H.lines(only_gn, "KEYS") == H.lines(res, "KEYS") == H.lines(both, "KEYS") and len(H.lines(plain, "KEYS")) == 2
    assert H.lines(plain, "DIGEST") == H.lines(only_gn, "DIGEST") == H.lines(res, "DIGEST") == H.lines(both, "DIGEST")
    assert len(H.lines(plain, "DIGEST")) == 1
