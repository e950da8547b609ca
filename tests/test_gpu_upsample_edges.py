"""GPU (-m gpu): the convex upsampling (csrc/corr_pyramid.hip: k_up_fwd, k_up_bwd_cells, k_up_bwd_flow) at the edges of its kernels.

k_up_bwd_cells gives a workgroup 64 coarse columns and splits the f^2 fine pixels of a cell over four wave groups; the shapes (tests/edge_ref.py
UP_SHAPES) put W on both sides of one and of two such tiles, f^2 at 1 (three idle groups), 4, 9 (an uneven split), 16 and 64, C at 1 and 2 and
H at 1, 2, 3.  Exact tests first -- a one-hot softmax makes the op a pure routing of small integers, so an indexing slip cannot hide behind a
tolerance -- then random inputs against the fp64 oracle under the criterion of tests/test_gpu_groupnorm.py: err = max |t - t64| / max |t64|,
fused <= max(2 x eager fp32 on the CPU, 1e-6).  Every tolerance case prints its errors (tests/edge_ref.py report)."""
import pytest
import torch

import edge_ref as E
import gps_gaussian_amd  # noqa: F401
from gps_gaussian_amd import corr as K

pytestmark = pytest.mark.gpu
FLOOR = 1e-6


def _run(flow, mask, gout, f, want=(True, True)):
    """-> dict(out, gflow, gmask) of the fused op; a gradient that is not asked for is None."""
    fl = flow.cuda().requires_grad_(want[0])
    mk = mask.cuda().requires_grad_(want[1])
    out = K.upsample_flow(fl, mk, f)
    out.backward(gout.cuda())
    torch.cuda.synchronize()
    return dict(out=out.detach(), gflow=fl.grad, gmask=mk.grad)


def _assert_onehot(c, got):
    assert torch.equal(E.bits(got["out"]), E.bits(c["out"])), "forward routing"
    assert torch.equal(E.bits(got["gflow"]), E.bits(c["gflow"])), "grad_flow routing"
    assert got["gmask"].shape == c["mask"].shape and bool((got["gmask"] == 0).all()), "grad_mask of a one-hot softmax"


@pytest.mark.parametrize("shape", E.UP_SHAPES, ids=E.sid)
def test_onehot_routing_is_exact(shape):
    """A. Logit 0 at one tap, -200 at the other eight: fp32 softmax is exactly one-hot, flow and grad_out are integers in [-8, 8]."""
    c = E.onehot_case(shape)
    _assert_onehot(c, _run(c["flow"], c["mask"], c["gout"], shape[-1]))


@pytest.mark.parametrize("tap", range(9))
def test_onehot_routing_one_tap_for_the_whole_tensor(tap):
    shape = (1, 2, 3, 65, 2)
    c = E.onehot_case(shape, tap)
    _assert_onehot(c, _run(c["flow"], c["mask"], c["gout"], shape[-1]))


@pytest.mark.parametrize("shape", E.UP_SHAPES, ids=E.sid)
def test_random_inputs_within_twice_eager_fp32(shape):
    """B and F. randn flow, 3 randn logits, randn grad_out against the fp64 oracle; a second run gives the same bits."""
    c = E.up_case(shape)
    got = _run(c["flow"], c["mask"], c["gout"], shape[-1])
    for q in ("out", "gflow", "gmask"):
        assert got[q].dtype == torch.float32 and got[q].shape == c["ref"][q].shape
        E.check("upsample_random", E.sid(shape), q, got[q], c["eager"][q], c["ref"][q], FLOOR)
    again = _run(c["flow"], c["mask"], c["gout"], shape[-1])
    for q in ("out", "gflow", "gmask"):
        assert E.same_bits(got[q], again[q]), q


@pytest.mark.parametrize("shape", [(2, 2, 3, 63, 2), (2, 1, 3, 65, 3)], ids=E.sid)
def test_one_gradient_only_gives_the_same_bits(shape):
    """C. k_up_bwd_cells with S == nullptr (no flow gradient) and with gmask == nullptr."""
    c = E.up_case(shape)
    both = _run(c["flow"], c["mask"], c["gout"], shape[-1])
    only_flow = _run(c["flow"], c["mask"], c["gout"], shape[-1], want=(True, False))
    only_mask = _run(c["flow"], c["mask"], c["gout"], shape[-1], want=(False, True))
    assert only_flow["gmask"] is None and only_mask["gflow"] is None
    assert E.same_bits(only_flow["gflow"], both["gflow"]) and E.same_bits(only_mask["gmask"], both["gmask"])
    assert E.same_bits(only_flow["out"], both["out"]) and E.same_bits(only_mask["out"], both["out"])


@pytest.mark.parametrize("shape", [(2, 2, 3, 63, 2), (1, 2, 2, 130, 8)], ids=E.sid)
def test_softmax_is_blind_to_a_shift_of_all_nine_logits(shape):
    """D. Logits on a 1/8 grid in [-4, 4]; 0 or +-4096 added to the nine taps of a fine pixel is exact in fp32 and cancels in `logit - max`."""
    c = E.shift_case(shape)
    a = _run(c["flow"], c["mask"], c["gout"], shape[-1])
    b = _run(c["flow"], c["moved"], c["gout"], shape[-1])
    for q in ("out", "gflow", "gmask"):
        assert E.same_bits(a[q], b[q]), q


@pytest.mark.parametrize("shape", [(2, 1, 3, 65, 3)], ids=E.sid)
def test_one_logit_80_above_the_rest(shape):
    """D. exp(-80) is still a normal fp32 number: nothing overflows, nothing is flushed that the fp64 oracle keeps."""
    c = E.up_case(shape, "spike")
    got = _run(c["flow"], c["mask"], c["gout"], shape[-1])
    for q in ("out", "gflow", "gmask"):
        E.check("upsample_spike80", E.sid(shape), q, got[q], c["eager"][q], c["ref"][q], FLOOR)


def test_channel_stride_of_grad_out():
    """E. C = 2 with an all-zero second grad_out channel against C = 1 on the first channel alone: the same bits in grad_mask and grad_flow[:, 0]
    (a wrong channel stride in k_up_bwd_cells would read the first channel twice, or the next sample)."""
    shape = (2, 2, 3, 63, 2)
    c = E.up_case(shape)
    g2 = c["gout"].clone()
    g2[:, 1] = 0.0
    two = _run(c["flow"], c["mask"], g2, shape[-1])
    one = _run(c["flow"][:, :1].contiguous(), c["mask"], c["gout"][:, :1].contiguous(), shape[-1])
    assert E.same_bits(two["gmask"], one["gmask"])
    assert E.same_bits(two["gflow"][:, 0], one["gflow"][:, 0])
    assert bool((two["gflow"][:, 1] == 0).all())
    assert E.same_bits(two["out"][:, 0], one["out"][:, 0])
