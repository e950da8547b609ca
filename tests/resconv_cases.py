"""What the residual-block 3x3 convolution's GPU test (test_gpu_resconv.py) and the CPU test of its bounds (test_resconv_bounds.py) share: the case
table with the reason for each shape, the seeded inputs, and the derived bounds.  With u = 2^-24 and g(n) = n u / (1 - n u), elementwise and for any
summation order:
    y        |y - y64| <= g(9 C_in + 1) (sum |w||x| + |b|)
    dx       <= g(9 C_out) sum |w||dy|
    dw, db   <= g(N H W) sum |dy||x|,  g(N H W) sum |dy|
the sums of absolute values coming from the same fp64 convolution (and its autograd) applied to |x|, |w|, |b|, |dy| (convop_run.ref64)."""
import functools

import torch

from gps_gaussian_amd import _capi, resconv

import convop_run as R
from convop_run import gamma

PAIRS = ((32, 32), (48, 48), (64, 64), (96, 96), (128, 48), (192, 64), (192, 96))     # stage 2's (C_in, C_out)
TILE_TAGS = ("T-1", "T", "T+1", "2T+1_T-1", "1_2T+1")
COUT_EDGES = (16, 32, 48, 64, 80, 96)
CIN_EDGES = (4, 32, 36, 64, 68, 100, 192)
WTILE = (4, 32)                                                                       # the pixel tile of the weight gradient (include/gpsgs.h)


def weight_counts():
    """(cap, group) at (C_in, C_out) = (4, 16): the largest number of pixel partitions and the reduction's group size, read off rc_scratch_bytes
    for planes of t = 1, 2, ... weight tiles as convop_run.group_size does."""
    M = 16 * (9 * 4 + 1)
    rows = lambda t: _capi.lib().rc_scratch_bytes(1, 4, 16, WTILE[0], WTILE[1] * t) // (4 * M)
    group = R.group_size(rows, 4096)
    cap = next(t for t in range(1, 4097) if rows(t + 1) == rows(t))                  # rows(t) = parts + ceil(parts / group) grows with t up to the cap
    assert rows(cap) == cap + -(-cap // group) and rows(4096) == rows(cap)
    return cap, group


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (N, C_in, C_out, H, W)"""
    TH, TW = resconv.tile()
    c = {}
    planes = ((TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 1, TW - 1), (1, 2 * TW + 1))
    for tag, hw in zip(TILE_TAGS, planes):
        c["tile_%s" % tag] = (2, 48, 48) + hw                   # around the forward's tile; 48: a full and a half block of output channels
    c["one_pixel"] = (1, 4, 16, 1, 1)                           # every tap but the centre is padding
    c["ragged_37x41"] = (1, 52, 48, 37, 41)                     # rows start off 16-byte boundaries
    for co in COUT_EDGES:
        c["cout_%d" % co] = (2, 36, co, 9, TW + 3)              # every block boundary of the output side (32, 64, 96) and the half blocks
    for ci in CIN_EDGES:
        c["cin_%d" % ci] = (2, ci, 48, 9, TW + 3)               # ... of the input side: dx's blocks of 32, dw's blocks of 64, the chunks of 4
    for ci, co in PAIRS:
        c["pair_%d_%d" % (ci, co)] = (2, ci, co, 17, TW + 1)
    cap, group = weight_counts()
    for tag, t in (("cap", cap), ("cap+1", cap + 1), ("group+1", group + 1)):
        c["wgrad_%s" % tag] = (1, 4, 16, WTILE[0], WTILE[1] * t)   # the weight gradient's pixel tiles: = the partitions, one more, one past a group
    return c


def names():
    return ["tile_%s" % t for t in TILE_TAGS] + ["one_pixel", "ragged_37x41"] + ["cout_%d" % c for c in COUT_EDGES] + ["cin_%d" % c for c in CIN_EDGES] + \
        ["pair_%d_%d" % p for p in PAIRS] + ["wgrad_cap", "wgrad_cap+1", "wgrad_group+1"]


def bounds(ref, N, Ci, Co, H, W):
    return dict(y=gamma(9 * Ci + 1) * ref["abs_y"], dx=gamma(9 * Co) * ref["abs_dx"], dw=gamma(N * H * W) * ref["abs_dw"],
                db=gamma(N * H * W) * ref["abs_db"])


def inputs(gen, N, Ci, Co, H, W):
    """Seeded normal x, w (x 0.2), b, dy; one exact-zero filter and one negative one."""
    x = torch.randn((N, Ci, H, W), generator=gen)
    w = torch.randn((Co, Ci, 3, 3), generator=gen) * 0.2
    b = torch.randn((Co,), generator=gen)
    w[Co // 2] = 0.0
    w[0] = -w[0].abs() - 1.0 / 16
    dy = torch.randn((N, Co, H, W), generator=gen)
    return dict(x=x, w=w, b=b, dy=dy, conv=dict(padding=1))


case = R.case_cache(cases, inputs, bounds)
