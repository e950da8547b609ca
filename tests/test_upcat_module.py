"""CPU: upcat.convert / regresser_forward as modules -- which modules are bound, state_dict untouched, idempotence, the pass-through computing the
SAME function as the unconverted stand-in bit for bit (on CPU tensors every site is the pass-through), modules whose `up` is not the plain one, the
hook's table of names left alone, and the op refusing CPU tensors."""
import copy

import pytest
import torch
from torch import nn

import gps_gaussian_amd
from gps_gaussian_amd import accelerate as A
from gps_gaussian_amd import upcat

import hook_run
import upcat_standin as S


@pytest.fixture(autouse=True)
def _counters():
    gps_gaussian_amd.build()
    before = dict(upcat.calls)
    yield
    upcat.calls.update(before)


def _model(up=None, seed=1):
    torch.manual_seed(seed)
    return S.Regresser(up)


def test_convert_binds_the_forward_and_changes_nothing_else():
    m = _model()
    plain = copy.deepcopy(m)
    keys = list(m.state_dict())
    holder = nn.ModuleDict({"regresser": m, "other": nn.Sequential(nn.Conv2d(3, 3, 1), nn.Upsample(scale_factor=2, mode="bilinear"))})
    assert upcat.convert(holder) == 1
    assert upcat.convert(holder) == 0 and upcat.convert(m) == 0                    # idempotent, from the root or from the module itself
    assert m.forward.__func__ is upcat.regresser_forward and m.forward.__self__ is m
    assert "forward" not in holder["other"].__dict__ and type(m) is S.Regresser
    sd, ref = m.state_dict(), plain.state_dict()
    assert list(sd) == keys == list(ref) and all(torch.equal(sd[k], ref[k]) for k in keys)
    assert [type(x) for x in m.modules()] == [type(x) for x in plain.modules()]
    # a module that lacks one member is not a regresser
    short = _model()
    del short.opacity_head
    assert upcat.convert(short) == 0 and "forward" not in short.__dict__
    # a deep copy of a converted module is converted, and bound to itself
    twin = copy.deepcopy(m)
    assert twin.forward.__self__ is twin and upcat.convert(twin) == 0


def test_cpu_forward_and_gradients_are_the_unconverted_ones_bit_for_bit():
    m = _model()
    plain = copy.deepcopy(m)
    assert upcat.convert(m) == 1
    args = S.inputs()
    upcat.calls.update(upcat=0, upcat_passthrough=0)
    got, want = m(*args), plain(*args)
    assert upcat.calls == {"upcat": 0, "upcat_passthrough": 3}
    assert all(torch.equal(g, w) for g, w in zip(got, want)) and [tuple(g.shape) for g in got] == [(2, 4, 16, 24), (2, 3, 16, 24), (2, 1, 16, 24)]
    sum(g.square().sum() for g in got).backward()
    sum(w.square().sum() for w in want).backward()
    for (k, p), (_, q) in zip(m.named_parameters(), plain.named_parameters()):
        assert p.grad is not None and torch.equal(p.grad, q.grad), k


@pytest.mark.parametrize("up", [nn.Upsample(scale_factor=2, mode="nearest"), nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True),
                                nn.Upsample(scale_factor=2, mode="bicubic"), nn.Upsample(size=(3, 3), mode="bilinear")],
                         ids=["nearest", "align_corners", "bicubic", "size"])
def test_an_up_that_is_not_the_plain_one_is_not_the_plain_one(up):
    assert not upcat._plain_up(up) and not upcat._plain_up(nn.Identity())
    assert upcat._plain_up(nn.Upsample(scale_factor=2, mode="bilinear")) and upcat._plain_up(nn.Upsample(scale_factor=(2.0, 2), mode="bilinear", align_corners=False))
    assert not upcat._plain_up(nn.Upsample(scale_factor=3, mode="bilinear")) and not upcat._plain_up(nn.Upsample(scale_factor=(2, 1), mode="bilinear"))


@pytest.mark.parametrize("up", [nn.Upsample(scale_factor=2, mode="nearest"), nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True)],
                         ids=["nearest", "align_corners"])
def test_a_module_with_another_up_still_runs_and_passes_through(up):
    m = _model(up)
    plain = copy.deepcopy(m)
    assert upcat.convert(m) == 1
    args = S.inputs(seed=3)
    upcat.calls.update(upcat=0, upcat_passthrough=0)
    assert all(torch.equal(g, w) for g, w in zip(m(*args), plain(*args)))
    assert upcat.calls == {"upcat": 0, "upcat_passthrough": 3}


def test_a_scale_of_three_still_runs_and_passes_through():
    torch.manual_seed(5)
    m = S.Regresser(nn.Upsample(scale_factor=3, mode="bilinear"), stride=3)
    plain = copy.deepcopy(m)
    assert upcat.convert(m) == 1
    args = S.inputs(N=1, H=27, W=54, seed=4, stride=3)
    upcat.calls.update(upcat=0, upcat_passthrough=0)
    got, want = m(*args), plain(*args)
    assert all(torch.equal(g, w) for g, w in zip(got, want)) and tuple(got[0].shape) == (1, 4, 27, 54)
    assert upcat.calls == {"upcat": 0, "upcat_passthrough": 3}


@pytest.mark.parametrize("ours_first", [True, False], ids=["upcat-first", "upcat-last"])
def test_convert_composes_with_the_conversions_that_change_submodule_classes(ours_first):
    from gps_gaussian_amd import conv1x1, conv3x3, groupnorm, gshead
    torch.manual_seed(2)
    m = S.Regresser(head=32)
    plain = copy.deepcopy(m)
    keys = list(m.state_dict())
    others = (gshead.convert, conv3x3.convert_regresser, conv1x1.convert, groupnorm.convert)
    try:
        if ours_first:
            assert upcat.convert(m) == 1
        n = [f(m) for f in (others if ours_first else others[::-1])]
        if not ours_first:
            assert upcat.convert(m) == 1
        assert sum(n) >= 7                                       # three head tails, out_conv + out_relu, three head tops
        assert type(m.out_conv) is conv3x3.FusedConv3x3 and type(m.out_relu) is nn.Identity and type(m.rot_head[0]) is conv3x3.FusedConv3x3
        assert m.forward.__func__ is upcat.regresser_forward and upcat.convert(m) == 0 and list(m.state_dict()) == keys
        args = S.inputs(seed=6)
        upcat.calls.update(upcat=0, upcat_passthrough=0)
        assert all(torch.equal(g, w) for g, w in zip(m(*args), plain(*args)))
        assert upcat.calls == {"upcat": 0, "upcat_passthrough": 3}
    finally:
        A.restore()          # the by-name counters the converted layers created


def test_the_hooks_names_and_counters_are_untouched():
    keys = list(A.calls)
    m = _model()
    upcat.convert(m)
    m(*S.inputs())
    hook_run.assert_the_names(A)
    assert list(A.calls) == keys and "upcat" not in A.calls and "upcat" not in A.NAMES
    assert set(upcat.calls) == {"upcat", "upcat_passthrough"}


def test_the_op_refuses_cpu_tensors():
    a, s = torch.randn(1, 2, 3, 4), torch.randn(1, 1, 6, 8)
    for args in ((a,), (a, s), (a.requires_grad_(True), s)):
        with pytest.raises(RuntimeError, match="upsample2x_cat inputs must live on a GPU"):
            upcat.upsample2x_cat(*args)
