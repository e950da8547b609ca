"""GPU (-m gpu): the residual-block 3x3 matrix-core convolution (csrc/resconv.hip; resconv.conv3x3 / FusedResConv3x3) against F.conv2d and its
autograd in fp64 on the CPU, starting from the same fp32 inputs.  The fp64 CPU reference is the only reference: no ATen convolution on the GPU
serves as one or runs a backward in this file; only the pass-through cases run ATen's forward there, and they compare the converted module with the
plain one, which is the same ATen call twice.

The cases, their inputs and the derived bounds are resconv_cases.py's (test_resconv_bounds.py shows on the CPU that the bounds are not vacuous)."""
import copy

import pytest
import torch
from torch import nn

import gps_gaussian_amd  # noqa: F401
from gps_gaussian_amd import resconv as RC

import convop_run as R
import resconv_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _counters():
    before = dict(RC.calls)
    yield
    RC.calls.update(before)


def _run(c):
    return R.run_case(RC.conv3x3, c)


@pytest.mark.parametrize("name", K.names())
def test_forward_and_backward_within_the_bounds(name):
    c = K.case(name)
    R.check(dict(test="fp32", case=name, dims=list(c["dims"])), "fused", _run(c), c["ref"], c["bounds"])


def test_the_weight_gradient_cases_sit_on_the_partition_and_group_edges():
    """The three wgrad_* planes are what the library's own counts make them: pixel tiles = the partition cap, one more, one past a reduction group."""
    cap, group = K.weight_counts()
    tiles = lambda name: K.cases()[name][3] // K.WTILE[0] * (K.cases()[name][4] // K.WTILE[1])
    assert cap > group > 1 and (tiles("wgrad_cap"), tiles("wgrad_cap+1"), tiles("wgrad_group+1")) == (cap, cap + 1, group + 1)


@pytest.mark.parametrize("which", ["192_96", "8_16"])
def test_small_integers_give_the_exact_answer(which):
    TH, TW = RC.tile()
    N, Ci, Co, H, W = (2, 192, 96, 2 * TH + 1, TW + 1) if which == "192_96" else (2, 8, 16, 9, 11)
    R.exact_integers("resconv_" + which, RC.conv3x3, ((N, Ci, H, W), (Co, Ci, 3, 3), (Co,), (N, Co, H, W)), padding=1)


def test_two_runs_give_the_same_bits():
    R.two_runs(_run, [(name, K.case(name)) for name in ("tile_2T+1_T-1", "pair_192_96", "wgrad_cap+1")])


@pytest.mark.parametrize("name", ["pair_128_48", "cin_68"])
def test_requires_grad_handling(name, monkeypatch):
    R.requires_grad_matrix(monkeypatch, RC, "rc_backward", RC.conv3x3, K.case(name))


def test_cpu_tensors_and_unsupported_widths_are_an_error():
    with pytest.raises(RuntimeError):
        RC.conv3x3(torch.zeros(1, 4, 3, 3), torch.zeros(16, 4, 3, 3), torch.zeros(16))
    dev = "cuda"
    for ci, co in ((6, 16), (196, 16), (4, 24), (4, 112)):
        with pytest.raises(RuntimeError):
            RC.conv3x3(torch.zeros(1, ci, 3, 3, device=dev), torch.zeros(co, ci, 3, 3, device=dev), torch.zeros(co, device=dev))
    with pytest.raises(RuntimeError):
        RC.conv3x3(torch.zeros(1, 4, 3, 3, device=dev).half(), torch.zeros(16, 4, 3, 3, device=dev), torch.zeros(16, device=dev))
    with pytest.raises(RuntimeError):
        RC.conv3x3(torch.zeros(1, 4, 3, 3, device=dev), torch.zeros(16, 4, 3, 3, device=dev), None)


class Block(nn.Module):
    """core/extractor.py:6-60, ResidualBlock with norm_fn 'group' and no shortcut layer."""

    def __init__(self, planes):
        super().__init__()
        self.conv1, self.conv2 = nn.Conv2d(planes, planes, 3, padding=1), nn.Conv2d(planes, planes, 3, padding=1)
        self.norm1, self.norm2 = nn.GroupNorm(planes // 8, planes), nn.GroupNorm(planes // 8, planes)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        y = self.relu(self.norm1(self.conv1(x)))
        y = self.relu(self.norm2(self.conv2(y)))
        return self.relu(x + y)


def _kept_shape(graph):
    """[N, 32, H, W] that the routing rule keeps for a 32 -> 32 layer that records a graph: four forward workgroups per compute unit."""
    TH, TW = RC.tile()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    shape = (2, 32, TH * -(-cus // 2), TW * 4)
    assert RC.keeps(shape[0], 32, 32, shape[2], shape[3], graph, cus)
    return shape


def test_a_converted_block_runs_the_fused_op():
    torch.manual_seed(21)
    blk = Block(32).cuda()
    plain = copy.deepcopy(blk)
    assert RC.convert(blk) == 2 and type(blk.conv1) is RC.FusedResConv3x3 and type(blk.conv2) is RC.FusedResConv3x3
    x = torch.randn(*_kept_shape(True), device="cuda")
    n0, p0 = RC.calls["resconv"], RC.calls["resconv_passthrough"]
    out = blk(x)
    out.square().sum().backward()
    assert (RC.calls["resconv"], RC.calls["resconv_passthrough"]) == (n0 + 2, p0)
    # the same block with the op called by hand: the fused op's bits, forward and gradients
    y = torch.relu_(plain.norm1(RC.conv3x3(x, plain.conv1.weight, plain.conv1.bias)))
    y = torch.relu_(plain.norm2(RC.conv3x3(y, plain.conv2.weight, plain.conv2.bias)))
    want = torch.relu(x + y)
    want.square().sum().backward()
    assert torch.equal(out, want)
    for (k, p), (_, q) in zip(blk.named_parameters(), plain.named_parameters()):
        assert p.grad is not None and torch.equal(p.grad, q.grad), k
    # and it is a convolution: against the plain block (ATen's forward), loosely
    with torch.no_grad():
        assert torch.allclose(out, plain(x), rtol=1e-3, atol=1e-3)


def test_what_the_op_does_not_take_goes_through_torch():
    torch.manual_seed(4)
    plain = nn.Conv2d(32, 48, 3, padding=1).cuda()
    fused = copy.deepcopy(plain)
    fused.__class__ = RC.FusedResConv3x3
    x = torch.randn(2, 32, 20, 22, device="cuda")
    both = R.passthrough_pair(RC.calls, "resconv")

    def forced(m):
        f = copy.deepcopy(m)
        f.__class__ = RC.FusedResConv3x3
        return f

    both(plain, fused, x.to(memory_format=torch.channels_last))                                  # channels-last input
    both(copy.deepcopy(plain).half(), copy.deepcopy(fused).half(), x.half())                      # fp16 input outside autocast
    both(plain, fused, x, dtype=torch.float16)                                                    # fp16 autocast
    both(plain, fused, x, dtype=torch.bfloat16)                                                   # bf16 autocast
    wide = torch.randn(2, 32, 20, 44, device="cuda")
    both(plain, fused, wide[:, :, :, ::2])                                                        # a strided view
    both(plain, fused, wide[:, :, :, :22])                                                        # ... and one with contiguous rows
    nb = nn.Conv2d(32, 48, 3, padding=1, bias=False).cuda()
    both(nb, forced(nb), x)                                                                       # no bias
    s2 = nn.Conv2d(32, 48, 3, stride=2, padding=1).cuda()
    both(s2, forced(s2), x)                                                                       # stride 2
    c40 = nn.Conv2d(32, 40, 3, padding=1).cuda()
    both(c40, forced(c40), x)                                                                     # C_out = 40
    both(plain, fused, x[:0])                                                                     # an empty batch
    both(plain, fused, x)                                                                         # what the measured rule routes away: C_out 48
    with torch.no_grad():
        both(plain, fused, x)                                                                     # ... and a forward alone of a small plane
