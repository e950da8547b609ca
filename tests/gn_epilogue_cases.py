"""Shared by the GroupNorm-epilogue tests (CPU and GPU): the cases, their seeded inputs, the fp64 reference with its guard band, and the stand-in
residual block.  Everything here is computed once per case (lru_cache) and never modified by a test.

A case draws, from a generator seeded with crc32("epi_" + name): x, w, b, res ~ randn (in that order), then dout ~ randn; w[0] is made negative and
w[C // 2] an exact zero.  The fp64 reference is  z = group_norm(x),  a = relu(z),  s = res + a,  out = relu(s)  (relu form: out = a).

GUARD BAND.  out, dx and dres of an element are not comparable between two precisions where a ReLU's argument may have either sign: elements whose
fp64 z -- or, in the residual form, s -- lies within BAND = 1e-5 of zero are left out of those three comparisons.  fp32 places z within a few 1e-7
of its fp64 value at these magnitudes, so the band is wide by a factor of some tens; the share it removes is capped at SHARE_CAP = 1e-3 per case
(a standard normal z has density 0.4 at zero: 2e-5 x 0.4 = 8e-6 expected, twice that with the second kink; the largest over these seeds is 3.1e-5)."""
import functools
import zlib

import torch
import torch.nn.functional as F
from torch import nn

import gps_gaussian_amd  # noqa: F401
from gps_gaussian_amd import _capi

EPS = 1e-5
BAND = 1e-5
SHARE_CAP = 1e-3

NAMES = ["row_K-1", "row_K+1", "row_2K+1", "plane_K-1", "plane_K+1", "plane_2K+1", "misaligned_105", "ragged_15", "one_element_planes", "ref_32ch_G8",
         "ref_96ch_G12"]
FP16_NAMES = ["row_K-1", "row_K+1", "row_2K+1", "plane_K+1", "misaligned_105", "ragged_15", "ref_32ch_G8", "ref_96ch_G12"]   # as tests/test_gpu_groupnorm.py
SHORT_ROWS = ["misaligned_105", "ragged_15", "one_element_planes"]     # rows under 1,024 elements
FORMS = ["relu", "relu_add_relu"]


def K():
    return int(_capi.lib().gn_chunk_elems())


def _shape_for_row(L):
    """[2, 2 cpg, 1, L / cpg] with G = 2: a row of exactly L elements."""
    for cpg in (4, 3, 5, 7, 2, 1):
        if L % cpg == 0:
            return (2, 2 * cpg, 1, L // cpg), 2
    raise AssertionError(L)


@functools.lru_cache(maxsize=None)
def cases():
    k = K()
    c = {}
    for name, L in (("row_K-1", k - 1), ("row_K+1", k + 1), ("row_2K+1", 2 * k + 1)):
        c[name] = _shape_for_row(L)
    for name, HW in (("plane_K-1", k - 1), ("plane_K+1", k + 1), ("plane_2K+1", 2 * k + 1)):
        c[name] = ((2, 4, 1, HW), 2)
    c["misaligned_105"] = ((2, 6, 5, 7), 2)
    c["ragged_15"] = ((1, 32, 3, 5), 8)
    c["one_element_planes"] = ((3, 8, 1, 1), 1)
    c["ref_32ch_G8"] = ((2, 32, 64, 64), 8)
    c["ref_96ch_G12"] = ((4, 96, 16, 16), 12)
    assert sorted(c) == sorted(NAMES)
    return c


@functools.lru_cache(maxsize=None)
def inputs(name, half=False):
    shape, G = cases()[name]
    gen = torch.Generator().manual_seed(zlib.crc32(("epi_" + name).encode()))
    x = torch.randn(shape, generator=gen)
    w = torch.randn(shape[1], generator=gen)
    b = torch.randn(shape[1], generator=gen)
    res = torch.randn(shape, generator=gen)
    dout = torch.randn(shape, generator=gen)
    w[0] = -abs(w[0]) - 0.1
    w[shape[1] // 2] = 0.0
    if half:
        x = x.half()
    return dict(name=name, shape=shape, G=G, half=half, x=x, w=w, b=b, res=res, dout=dout)


@functools.lru_cache(maxsize=None)
def ref64(name, form, half=False):
    """fp64 on the CPU (from the fp16 values of x where half): out, dx, dgamma, dbeta, dres (None in the relu form) and `keep`, the elements outside
    the guard band."""
    c = inputs(name, half)
    x = c["x"].double().requires_grad_(True)
    w = c["w"].double().requires_grad_(True)
    b = c["b"].double().requires_grad_(True)
    res = c["res"].double().requires_grad_(True)
    z = F.group_norm(x, c["G"], w, b, EPS)
    keep = z.detach().abs() >= BAND
    out = F.relu(z)
    if form == "relu_add_relu":
        s = res + out
        keep &= s.detach().abs() >= BAND
        out = F.relu(s)
    out.backward(c["dout"].double())
    return dict(out=out.detach(), dx=x.grad, dgamma=w.grad, dbeta=b.grad, dres=res.grad if form == "relu_add_relu" else None, keep=keep,
                excluded_share=float((~keep).double().mean()))


class StandInBlock(nn.Module):
    """conv -> GN -> ReLU -> conv -> GN -> ReLU, a 1x1-conv + GN downsample, add, ReLU (written for these tests; in-place ReLUs like the networks
    this package serves)."""

    def __init__(self, in_planes=16, planes=16):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, planes, 3, padding=1)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1)
        self.relu = nn.ReLU(inplace=True)
        self.norm1 = nn.GroupNorm(2, planes)
        self.norm2 = nn.GroupNorm(2, planes)
        self.norm3 = nn.GroupNorm(4, planes)
        self.downsample = nn.Sequential(nn.Conv2d(in_planes, planes, 1), self.norm3)

    def forward(self, x):
        y = self.relu(self.norm1(self.conv1(x)))
        y = self.relu(self.norm2(self.conv2(y)))
        if self.downsample is not None:
            x = self.downsample(x)
        return self.relu(x + y)


class StandIn(nn.Module):
    """A Sequential(conv, GN, ReLU) stem and one StandInBlock.  `fused_forward` routes the block through groupnorm.residual_block_forward."""

    def __init__(self):
        super().__init__()
        self.stem = nn.Sequential(nn.Conv2d(3, 16, 5, padding=2), nn.GroupNorm(2, 16), nn.ReLU(inplace=True))
        self.block = StandInBlock()
        self.fused_forward = False

    def forward(self, x):
        x = self.stem(x)
        if self.fused_forward:
            from gps_gaussian_amd import groupnorm
            return groupnorm.residual_block_forward(self.block, x)
        return self.block(x)


def stand_in():
    """Seeded: the network, an input [2, 3, 40, 36] (rows of 8 x 1440 = 11,520 elements: two chunks, the second ragged) and an output gradient."""
    torch.manual_seed(33)
    net = StandIn()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.GroupNorm):
                m.weight.normal_()
                m.bias.normal_()
    return net, torch.randn(2, 3, 40, 36), torch.randn(2, 16, 40, 36)
