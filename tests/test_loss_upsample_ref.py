"""CPU: the references the edge tests of the convex upsampling and the L1 + SSIM loss stand on (tests/edge_ref.py), checked against each other.

  * oracle/corr_oracle.py's upsampling, forward and hand-written backward, against fp64 torch autograd of the reference's own formula;
  * oracle/loss_oracle.py's SSIM value and hand-derived gradient (the M1 / M2 / M3 maps the kernel also uses) against fp64 autograd of the eager
    restatement: this is what makes the oracle's gradient independent of the kernel's derivation.  The two differ in the last fp32 bit of the
    window's normalisation, which moves the value by ~7e-8 and the gradient by ~6e-7 of its largest element: the bounds are 2e-7 and 2e-6;
  * the premises of the exact GPU tests, in numpy fp32 and in the fp64 oracle."""
import numpy as np
import pytest
import torch

import edge_ref as E
from oracle import loss_oracle as LO


@pytest.mark.parametrize("shape", E.UP_SHAPES, ids=E.sid)
@pytest.mark.parametrize("kind", ["random", "spike"])
def test_upsample_oracle_matches_fp64_autograd(shape, kind):
    c = E.up_case(shape, kind)
    a = E.upsample_autograd(c["flow"], c["mask"], c["gout"], shape[-1], torch.float64)
    for k in ("out", "gflow", "gmask"):
        assert a[k].shape == c["ref"][k].shape
        d = float((a[k] - c["ref"][k]).abs().max())
        assert d <= 1e-12, (k, d)


@pytest.mark.parametrize("shape", E.LOSS_SHAPES, ids=E.sid)
def test_ssim_oracle_matches_fp64_autograd(shape):
    c = E.loss_case(shape)
    assert c["floor_value"] <= 2e-7, c["floor_value"]
    assert c["floor_grad"] <= 2e-6, c["floor_grad"]
    assert abs(c["l1"] - float((c["pred"].double() - c["gt"].double()).abs().mean())) <= 1e-15


@pytest.mark.parametrize("name", E.DEGENERATE)
def test_ssim_oracle_matches_fp64_autograd_on_degenerate_pairs(name):
    c = E.degenerate_case(name)
    if name == "two_constants":
        # Constant images a, b under a window whose taps sum to S = 1 + d: sigma1^2 + sigma2^2 = (a^2 + b^2)(S - S^2), 2 sigma12 = 2ab (S - S^2), so
        # the map moves by about ((a - b)^2 / C2) d = (0.0625 / 9e-4) d.  One fp32 ulp in each 1-D factor of the window (|d| <= 2 x 1.2e-7) is 1.7e-5:
        # here, and only here, the last bit of the window's normalisation is visible in the fifth digit of SSIM.
        assert c["floor_value"] <= 2e-5 and c["floor_grad"] <= 2e-4
    else:
        assert c["floor_value"] <= 2e-7   # the gradient is zero up to fp64 rounding (of 1 / N-sized terms that cancel), and SSIM is 1
        assert abs(c["ssim"] - 1.0) <= 1e-12 and abs(c["ssim64"] - 1.0) <= 1e-12
        assert float(c["grad"].abs().max()) <= 1e-12 and float(c["grad64"].abs().max()) <= 1e-12


def test_exp_of_minus_200_is_zero_in_fp32():
    assert np.exp(np.float32(-200.0)) == 0 and np.exp(np.float32(-200.0)).dtype == np.float32
    e = np.exp(np.array([0.0] + [-200.0] * 8, np.float32))
    assert (e / e.sum() == np.array([1.0] + [0.0] * 8, np.float32)).all()


@pytest.mark.parametrize("shape", E.UP_SHAPES + [(1, 2, 3, 65, 2)], ids=E.sid)
def test_onehot_expectation_is_integer_and_below_2_24(shape):
    consts = range(9) if shape == (1, 2, 3, 65, 2) else [None]
    for const in consts:
        c = E.onehot_case(shape, const)
        assert c["worst"] < 2 ** 24          # every partial sum, in any order, is an integer that fp32 holds exactly
        for k in ("flow", "gout", "out", "gflow"):
            assert torch.equal(c[k], c[k].round()) and float(c[k].abs().max()) < 2 ** 24
        if const is None and shape[3] >= 9:
            assert sorted(np.unique(c["k"])) == list(range(9))
        # the integer routing is the fp64 oracle's answer for this mask
        r = E.upsample_oracle(c["flow"].numpy(), c["mask"].numpy(), c["gout"].numpy(), shape[-1])
        assert float((r["out"] - c["out"].double()).abs().max()) <= 1e-9 and float((r["gflow"] - c["gflow"].double()).abs().max()) <= 1e-9
        assert float(r["gmask"].abs().max()) <= 1e-60


@pytest.mark.parametrize("shape", [E.UP_SHAPES[1], E.UP_SHAPES[4]], ids=E.sid)
def test_softmax_shift_is_exact_in_fp32(shape):
    c = E.shift_case(shape)
    for m in (c["mask"], c["moved"]):
        assert torch.equal(m * 8, (m * 8).round()) and float(m.abs().max()) <= 4100
    f = shape[-1]
    a, b = (m.view(shape[0], 9, f, f, shape[2], shape[3]) for m in (c["mask"], c["moved"]))
    assert torch.equal(a - a.max(dim=1, keepdim=True).values, b - b.max(dim=1, keepdim=True).values)
    assert len(torch.unique((b - a)[:, 0])) == (3 if a[:, 0].numel() >= 3 else 1)


@pytest.mark.parametrize("shift", E.SHIFTS, ids=lambda s: "%d_%d" % s)
def test_oracle_gradient_moves_with_the_block(shift):
    """The zero margin is wide enough: in fp64 the SSIM gradient of the moved pair IS the rolled gradient of the first, and it is zero where
    the roll wraps around."""
    hw = E.shift_hw(*shift)
    s0, g0 = LO.ssim(*E.shifted_pair(hw, 0, 0), with_grad=True)
    s1, g1 = LO.ssim(*E.shifted_pair(hw, *shift), with_grad=True)
    assert np.abs(g1 - np.roll(g0, shift, axis=(-2, -1))).max() <= 1e-15
    assert abs(s0 - s1) <= 1e-15
    B, (y0, x0), m = E.SHIFT_BLOCK, E.SHIFT_AT, E.SHIFT_MARGIN
    outside = np.ones(g0.shape, bool)
    outside[..., y0 - m:y0 + B + m, x0 - m:x0 + B + m] = False
    assert np.abs(g0[outside]).max() == 0.0 and np.abs(g0).max() > 0
    assert E.shift_hw(4, 20) == E.shift_hw(32, 64) == E.shift_hw(17, 23) == (96, 128) and E.shift_hw(43, 75) == (105, 137)
