"""GPU (-m gpu): the 1-D correlation sampler (k_cs_fwd, k_cs_bwd, k_cs_bwd4) and the fused multi-level lookup (k_lookup_fwd, k_lookup_bwd), both
in csrc/corr_sampler.hip, at their edges.  References: the C twin, value for value (A, B, D, E, F); the fp64 hat function
within the derived bound 4 * 2^-24 * S (A, B; both in tests/corr_edge_ref.py, tied to each other and to the reference's grid_sample path by
tests/test_corr_lookup_ref.py); and exact statements that owe nothing to either (C, G).  Coordinates: tests/corr_edge_ref.py special_coords --
exact integers, one ulp either side, negative, half or wholly outside the row, far away.  Every shape is tiny; the file runs in a few seconds."""
import numpy as np
import pytest
import torch

import corr_edge_ref as R
import gps_gaussian_amd  # noqa: F401
from gps_gaussian_amd import _capi
from gps_gaussian_amd import corr as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.float16]
DT_IDS = ["fp32", "fp16"]


def _half(dtype):
    return dtype is torch.float16


def _as(t, dtype):
    """What the kernels give for the twin's fp32 result `t`: itself, or rounded once to fp16."""
    return t.to(dtype)


def gpu_sampler(vol, coords, gout, r, dtype):
    """corr.forward / corr.backward on the GPU -> (out, grad_volume) on the CPU."""
    v, c = vol.to(DEV, dtype), coords.to(DEV)
    out, = K.forward(v, c, r)
    gv, = K.backward(v, c, gout.to(DEV, dtype), r)
    assert out.dtype == dtype and gv.dtype == dtype and gv.shape == v.shape
    return out.cpu(), gv.cpu()


def gpu_lookup(pyr, coords, gout, r, dtype):
    """_LookupPyramid forward and backward on the GPU -> (out, [grad per level]) on the CPU."""
    vs = [p.to(DEV, dtype).requires_grad_(True) for p in pyr]
    out = K._LookupPyramid.apply(coords.to(DEV), r, *vs)
    out.backward(gout.to(DEV, dtype))
    assert out.dtype == dtype and all(v.grad is not None and v.grad.shape == v.shape and v.grad.dtype == dtype for v in vs)
    return out.detach().cpu(), [v.grad.cpu() for v in vs]


def _pyramid(N, H1, W1, W2, levels, seed, half):
    return [R.randn((N, H1, W1, w), (seed, l), half) for l, w in enumerate(R.widths(W2, levels))]


# ---- A. sampler against the twin, value for value, and against the hat function ---------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("r", R.SAMPLER_R)
def test_sampler_matches_the_twin_at_special_coordinates(r, dtype):
    worst_f = worst_b = 0.0
    for W2 in R.SAMPLER_W2:
        c = R.coords_grid(W2, r, 2, 2)
        N, _, H1, W1 = c.shape
        vol = R.randn((N, H1, W1, W2), ("A", W2, r), _half(dtype))
        gout = R.randn((N, 2 * r + 1, H1, W1), ("A-g", W2, r), _half(dtype))
        out, gv = gpu_sampler(vol, c, gout, r, dtype)
        assert R.same_values(out, _as(R.twin_forward(vol, c, r), dtype)), (W2, r)
        assert R.same_values(gv, _as(R.twin_backward(c, gout, W2, r), dtype)), (W2, r)
        if not _half(dtype):
            rf = R.bound_ratio(out, R.hat_lookup([vol], c, r), R.hat_magnitude([vol], c, r))
            (gref,), (gmag,) = R.hat_backward([W2], c, gout, r)
            rb = R.bound_ratio(gv, gref, gmag)
            assert rf <= 1.0 and rb <= 1.0, (W2, r, rf, rb)
            worst_f, worst_b = max(worst_f, rf), max(worst_b, rb)
    if not _half(dtype):
        R.report(dict(test="sampler_vs_hat", family="gpu sampler, r=%d" % r, forward_over_bound=worst_f, backward_over_bound=worst_b))


# ---- B. fused lookup against the twin per level ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("levels", R.LOOKUP_LEVELS)
def test_lookup_matches_the_twin_per_level(levels, dtype):
    worst_f = worst_b = 0.0
    for W2 in R.LOOKUP_W2:
        for r in R.LOOKUP_R:
            rd = 2 * r + 1
            c = R.coords_grid(W2, r, 2, 2)
            N, _, H1, W1 = c.shape
            wl = R.widths(W2, levels)
            pyr = _pyramid(N, H1, W1, W2, levels, ("B", W2, r), _half(dtype))
            gout = R.randn((N, levels * rd, H1, W1), ("B-g", W2, r, levels), _half(dtype))
            out, grads = gpu_lookup(pyr, c, gout, r, dtype)
            assert out.shape == (N, levels * rd, H1, W1)
            assert R.same_values(out, _as(R.twin_lookup(pyr, c, r), dtype)), (W2, r)
            want = R.twin_lookup_backward(wl, c, gout, r)
            for l, w in enumerate(wl):
                assert grads[l].shape == (N, H1, W1, w)
                assert R.same_values(grads[l], _as(want[l], dtype)), (W2, r, l)
                if w == 0:          # a level of width 0: all-zero channels, an empty gradient
                    assert grads[l].numel() == 0 and not bool(out[:, l * rd:(l + 1) * rd].any())
            if not _half(dtype):
                rf = R.bound_ratio(out, R.hat_lookup(pyr, c, r), R.hat_magnitude(pyr, c, r))
                grefs, gmags = R.hat_backward(wl, c, gout, r)
                rb = max(R.bound_ratio(g, gr, gm) for g, gr, gm in zip(grads, grefs, gmags))
                assert rf <= 1.0 and rb <= 1.0, (W2, r, rf, rb)
                worst_f, worst_b = max(worst_f, rf), max(worst_b, rb)
    if not _half(dtype):
        R.report(dict(test="lookup_vs_hat", family="gpu lookup, %d levels" % levels, forward_over_bound=worst_f, backward_over_bound=worst_b))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("levels", R.LOOKUP_LEVELS)
def test_lookup_channel_layout(levels, dtype):
    """Channel l*(2r+1)+k is tap k of level l: with V_l[..., j] = 100 (l + 1) + j and coordinates that are integers at every level and keep every
    window inside its row, out[n, l*(2r+1)+k, y, x] = 100 (l + 1) + c / 2^l - r + k, exactly (integers below 2^11)."""
    W2, r, N, H1 = 64, 1, 2, 3
    rd = 2 * r + 1
    cvals = torch.arange(8, 49, 8, dtype=torch.float32)              # c / 8 in 1..6: inside [r, 8 - 1 - r] at level 3
    c = cvals.repeat(N * H1).reshape(N, 1, H1, -1)
    W1 = c.shape[-1]
    pyr = [(100.0 * (l + 1) + torch.arange(w, dtype=torch.float32)).expand(N, H1, W1, w).contiguous() for l, w in enumerate(R.widths(W2, levels))]
    gout = torch.zeros(N, levels * rd, H1, W1)
    out, _ = gpu_lookup(pyr, c, gout, r, dtype)
    for l in range(levels):
        for k in range(rd):
            want = (100.0 * (l + 1) + c[:, 0] / 2 ** l - r + k).to(dtype)
            assert R.same_bits(out[:, l * rd + k], want), (l, k)
    # and the backward reads grad_out at the same channel: a one-hot channel (l0, k0) reaches level l0 alone, at column c / 2^l0 - r + k0
    for l0 in range(levels):
        for k0 in (0, rd - 1):
            gout = torch.zeros(N, levels * rd, H1, W1)
            gout[:, l0 * rd + k0] = 1.0
            _, grads = gpu_lookup(pyr, c, gout, r, dtype)
            for l, g in enumerate(grads):
                want = torch.zeros_like(g)
                if l == l0:
                    want.scatter_(-1, (c[:, 0] / 2 ** l - r + k0).long()[..., None], 1.0)
                assert torch.equal(g, want), (l0, k0, l)


# ---- C. exact statements that owe nothing to the twin -------------------------------------------------------------------------
def _gather(vol, ci, r):
    """out[n,k,y,x] = vol[n,y,x,ci - r + k] where that column exists, else +0 (ci: integer coordinates [N,H1,W1], int64)."""
    W2 = vol.shape[-1]
    cols = ci[..., None] - r + torch.arange(2 * r + 1)                     # [N,H1,W1,rd]
    ok = (cols >= 0) & (cols < W2)
    if W2 == 0:
        return torch.zeros(cols.shape, dtype=vol.dtype).permute(0, 3, 1, 2)
    g = torch.gather(vol, -1, cols.clamp(0, W2 - 1))
    return torch.where(ok, g, torch.zeros_like(g)).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_integer_coordinates_are_a_pure_gather(dtype):
    for W2, r in ((1, 0), (1, 2), (4, 1), (7, 4), (8, 7), (17, 2)):
        ints = torch.arange(-r - 2, W2 + r + 3)
        ci = ints.repeat(4).reshape(2, 2, -1)
        c = ci.float()[:, None]
        vol = R.randn(ci.shape + (W2,), ("C1", W2, r), _half(dtype))
        assert bool((vol != 0).all())
        out, _ = gpu_sampler(vol, c, torch.zeros(2, 2 * r + 1, 2, ci.shape[-1]), r, dtype)
        assert R.same_bits(out, _gather(vol, ci, r).to(dtype)), (W2, r)
    # fused lookup: multiples of 8 are integers at all four levels
    W2, levels, r = 17, 4, 2
    rd = 2 * r + 1
    ci = (8 * torch.arange(-3, 6)).repeat(4).reshape(2, 2, -1)
    pyr = _pyramid(2, 2, ci.shape[-1], W2, levels, "C1-l", _half(dtype))
    out, _ = gpu_lookup(pyr, ci.float()[:, None], torch.zeros(2, levels * rd, 2, ci.shape[-1]), r, dtype)
    for l in range(levels):
        assert R.same_bits(out[:, l * rd:(l + 1) * rd], _gather(pyr[l], ci // 2 ** l, r).to(dtype)), l


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_one_hot_row_gives_exactly_the_two_weights(dtype):
    """A row that is 1 at column j0 and 0 elsewhere: tap k is max(0, 1 - |c - r + k - j0|), i.e. 1 - dx and dx in the two taps that see the column
    and 0 in the others -- exact for coordinates that are multiples of 1/8 (the hat function in fp64 is exact there, and so is its cast)."""
    for W2, r in ((1, 1), (5, 2), (8, 4), (9, 0)):
        N, H1, W1 = 2, 2, 40
        c = R.eighths((N, 1, H1, W1), -r - 2, W2 + r + 2, ("C2", W2, r))
        j0 = torch.from_numpy(np.random.default_rng(R._seed("C2-j", W2, r)).integers(0, W2, (N, H1, W1, 1)))
        vol = torch.zeros(N, H1, W1, W2).scatter_(-1, j0, 1.0)
        want = R.hat_lookup([vol], c, r)
        dx = (c - c.floor()).double()[:, 0]
        assert bool(((want == 0) | (want == 1) | (want == dx[:, None]) | (want == 1 - dx[:, None])).all())
        out, _ = gpu_sampler(vol, c, torch.zeros(N, 2 * r + 1, H1, W1), r, dtype)
        assert torch.equal(out.double(), want), (W2, r)
    # the fused lookup: level l sees c / 2^l, multiples of 1/64 -- still exact (weights are multiples of 1/64 in [0, 1]: representable in fp16)
    W2, levels, r = 9, 4, 1
    N, H1, W1 = 2, 2, 40
    c = R.eighths((N, 1, H1, W1), -r - 2, W2 + r + 2, "C2-l")
    pyr = []
    for l, w in enumerate(R.widths(W2, levels)):
        j0 = torch.from_numpy(np.random.default_rng(R._seed("C2-lj", l)).integers(0, w, (N, H1, W1, 1)))
        pyr.append(torch.zeros(N, H1, W1, w).scatter_(-1, j0, 1.0))
    out, _ = gpu_lookup(pyr, c, torch.zeros(N, levels * (2 * r + 1), H1, W1), r, dtype)
    assert torch.equal(out.double(), R.hat_lookup(pyr, c, r))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_one_hot_grad_out_at_an_integer_lands_in_one_column(dtype):
    """grad_out non-zero in ONE tap k0 per (n, y, x), integer coordinate c: grad_volume[n,y,x,:] is that value at column c - r + k0 (if the row has
    it) and zero elsewhere -- this pins both ends of the backward's tap range, i == 0 (k0 = 0) and i == rd - 1 / i == rd (dx == 0)."""
    for W2, r in ((1, 0), (4, 1), (8, 4), (9, 2), (12, 7)):
        rd = 2 * r + 1
        ints = torch.arange(-r - 1, W2 + r + 2)
        ci = ints.repeat_interleave(rd).reshape(1, 1, -1).expand(2, 2, -1).contiguous()      # every (c, k0) pair
        W1 = ci.shape[-1]
        k0 = torch.arange(rd).repeat(ints.numel()).reshape(1, 1, -1).expand(2, 2, -1)
        val = R.randn((2, 2, W1), ("C3", W2, r), _half(dtype))
        gout = torch.zeros(2, rd, 2, W1).scatter_(1, k0[:, None], val[:, None])
        col = ci - r + k0
        want = torch.zeros(2, 2, W1, W2)
        ok = (col >= 0) & (col < W2)
        want.scatter_(-1, col.clamp(0, W2 - 1)[..., None], torch.where(ok, val, torch.zeros_like(val))[..., None])
        _, gv = gpu_sampler(torch.zeros(2, 2, W1, W2), ci.float()[:, None], gout, r, dtype)
        assert torch.equal(gv, want.to(dtype)), (W2, r)
        _, (g0,) = gpu_lookup([torch.zeros(2, 2, W1, W2)], ci.float()[:, None], gout, r, dtype)
        assert torch.equal(g0, want.to(dtype)), (W2, r)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_one_hot_grad_out_gives_exactly_the_two_weights(dtype):
    """grad_out 1 in ONE tap k0 per (n, y, x) and coordinates that are multiples of 1/8: grad_volume[n,y,x,j] = max(0, 1 - |c - r + k0 - j|), i.e.
    1 - dx at column floor(c) - r + k0 and dx at the next (tap index i == rd for k0 == rd - 1), exactly -- the hat function's autograd in fp64."""
    for W2, r in ((1, 1), (4, 0), (8, 4), (9, 2), (12, 7)):
        rd = 2 * r + 1
        N, H1, W1 = 2, 2, 8 * rd
        c = R.eighths((N, 1, H1, W1), -r - 2, W2 + r + 2, ("C5", W2, r))
        k0 = torch.arange(rd).repeat(N * H1 * W1 // rd).reshape(N, 1, H1, W1)
        gout = torch.zeros(N, rd, H1, W1).scatter_(1, k0, 1.0)
        (want,), _ = R.hat_backward([W2], c, gout, r)
        _, gv = gpu_sampler(torch.zeros(N, H1, W1, W2), c, gout, r, dtype)
        assert torch.equal(gv.double(), want), (W2, r)
    # fused lookup, every level: c / 2^l are multiples of 1/64
    W2, levels, r = 17, 4, 2
    rd = 2 * r + 1
    N, H1, W1 = 2, 2, 8 * rd * levels
    c = R.eighths((N, 1, H1, W1), -r - 2, W2 + r + 2, "C5-l")
    ch = torch.arange(levels * rd).repeat(N * H1 * W1 // (levels * rd)).reshape(N, 1, H1, W1)
    gout = torch.zeros(N, levels * rd, H1, W1).scatter_(1, ch, 1.0)
    wl = R.widths(W2, levels)
    want, _ = R.hat_backward(wl, c, gout, r)
    _, grads = gpu_lookup([torch.zeros(N, H1, W1, w) for w in wl], c, gout, r, dtype)
    for l in range(levels):
        assert torch.equal(grads[l].double(), want[l]), l
        assert bool(want[l].any())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("s", [3, -3, 8, -5])
def test_sampler_moves_with_the_volume(s, dtype):
    """(V moved by s columns, coords + s) has the bits of (V, coords), forward and -- on the columns both rows hold -- backward: coordinates that
    are multiples of 1/8, V zero within |s| columns of either end so that the move loses nothing."""
    for W2, r in ((24, 4), (20, 1), (17, 0)):
        N, H1, W1 = 2, 2, 48
        c = R.eighths((N, 1, H1, W1), -r - 2, W2 + r + 2, ("C4", W2, r))
        vol = R.randn((N, H1, W1, W2), ("C4", W2, r), _half(dtype))
        vol[..., :abs(s)] = 0
        vol[..., W2 - abs(s):] = 0
        gout = R.randn((N, 2 * r + 1, H1, W1), ("C4-g", W2, r), _half(dtype))
        out, gv = gpu_sampler(vol, c, gout, r, dtype)
        out_s, gv_s = gpu_sampler(R.shift_volume(vol, s), c + s, gout, r, dtype)
        assert R.same_bits(out, out_s), (W2, r)
        lo, hi = max(s, 0), min(W2, W2 + s)
        assert R.same_bits(gv_s[..., lo:hi], gv[..., lo - s:hi - s]), (W2, r)
        assert bool(out.any()) and bool(gv.any())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("s", [8, -8])
def test_lookup_moves_with_the_pyramid(s, dtype):
    """The same through the fused lookup: s = +-8 is an integer move at all four levels (level l moves by s / 2^l)."""
    W2, levels, r = 64, 4, 2
    N, H1, W1 = 2, 2, 48
    c = R.eighths((N, 1, H1, W1), -r - 2, W2 + r + 2, "C4-l")
    pyr = _pyramid(N, H1, W1, W2, levels, "C4-l", _half(dtype))
    for l, v in enumerate(pyr):
        m = abs(s) >> l
        v[..., :m] = 0
        v[..., v.shape[-1] - m:] = 0
    gout = R.randn((N, levels * (2 * r + 1), H1, W1), "C4-lg", _half(dtype))
    out, grads = gpu_lookup(pyr, c, gout, r, dtype)
    out_s, grads_s = gpu_lookup([R.shift_volume(v, s // 2 ** l) for l, v in enumerate(pyr)], c + s, gout, r, dtype)
    assert R.same_bits(out, out_s)
    for l, (g, gs) in enumerate(zip(grads, grads_s)):
        sl, w = s // 2 ** l, g.shape[-1]
        lo, hi = max(sl, 0), min(w, w + sl)
        assert R.same_bits(gs[..., lo:hi], g[..., lo - sl:hi - sl]), l
        assert bool(g.any())


# ---- D. block tails -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("nhw", R.TAIL_NHW, ids=lambda s: "x".join(map(str, s)))
def test_block_tails(nhw, dtype):
    """N*H1*W1 = 255, 256, 257, 513 threads of the forwards; W2 = 4: as many quads of k_cs_bwd4; W2 = 1, 7: k_cs_bwd and k_lookup_bwd end inside a
    block (7 * 257 = 1799 = 7 * 256 + 7)."""
    N, H1, W1 = nhw
    r, levels = 2, 4
    rd = 2 * r + 1
    for W2 in R.TAIL_W2:
        sc = R.special_coords(W2, r, "D")
        c = sc.repeat(-(-N * H1 * W1 // sc.numel()))[:N * H1 * W1].reshape(N, 1, H1, W1)
        vol = R.randn((N, H1, W1, W2), ("D", W2, nhw), _half(dtype))
        gout = R.randn((N, rd, H1, W1), ("D-g", W2, nhw), _half(dtype))
        out, gv = gpu_sampler(vol, c, gout, r, dtype)
        assert R.same_values(out, _as(R.twin_forward(vol, c, r), dtype)), W2
        assert R.same_values(gv, _as(R.twin_backward(c, gout, W2, r), dtype)), W2
        pyr = _pyramid(N, H1, W1, W2, levels, ("D-l", W2, nhw), _half(dtype))
        gl = R.randn((N, levels * rd, H1, W1), ("D-lg", W2, nhw), _half(dtype))
        out, grads = gpu_lookup(pyr, c, gl, r, dtype)
        assert R.same_values(out, _as(R.twin_lookup(pyr, c, r), dtype)), W2
        for l, (g, want) in enumerate(zip(grads, R.twin_lookup_backward(R.widths(W2, levels), c, gl, r))):
            assert R.same_values(g, _as(want, dtype)), (W2, l)


# ---- D2. one level of the fused lookup IS the sampler ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("r", [0, 4])
@pytest.mark.parametrize("W2", [8, 7])
def test_one_level_lookup_is_the_sampler(W2, r, dtype):
    """cs_lookup_* with levels = 1 and cs_forward / cs_backward on the same volume, coordinates and grad_out give the same bits: the four kernels
    share one sampling core (sample_row, tap_grad).  W2 = 8 takes k_cs_bwd4, W2 = 7 the scalar k_cs_bwd; 260 rows = one full block and a tail."""
    N, H1, W1 = 1, 2, 130
    sc = R.special_coords(W2, r, "D2")
    c = sc.repeat(-(-N * H1 * W1 // sc.numel()))[:N * H1 * W1].reshape(N, 1, H1, W1)
    vol = R.randn((N, H1, W1, W2), ("D2", W2, r), _half(dtype))
    gout = R.randn((N, 2 * r + 1, H1, W1), ("D2-g", W2, r), _half(dtype))
    out_s, gv_s = gpu_sampler(vol, c, gout, r, dtype)
    out_l, (gv_l,) = gpu_lookup([vol], c, gout, r, dtype)
    assert R.same_bits(out_l, out_s)
    assert R.same_bits(gv_l, gv_s)
    assert bool(out_s.any()) and bool(gv_s.any())


# ---- E. zero fill and bounds, through the C-ABI -----------------------------------------------------------------------------------
SENTINEL = 777.0


class Guarded:
    """A tensor of `shape` inside a larger allocation: `lead` sentinel elements before it (64: 16-byte aligned; 65: not), 64 after it, its own bytes
    pre-filled with 0xFF (a NaN in either dtype).  The kernels write into torch.empty memory: whatever they leave unwritten shows as that NaN."""

    def __init__(self, shape, dtype, lead=R.FILL_GUARD):
        self.n = int(np.prod(shape))
        self.lead = lead
        self.flat = torch.full((lead + self.n + R.FILL_GUARD,), SENTINEL, dtype=dtype, device=DEV)
        self.inner = self.flat[lead:lead + self.n]
        if self.n:
            self.inner.view(torch.uint8).fill_(0xFF)
        self.shape = tuple(shape)
        self.ptr = self.inner.data_ptr() if self.n else None

    def check(self, want, what):
        flat = self.flat.cpu()
        assert bool((flat[:self.lead] == SENTINEL).all()) and bool((flat[self.lead + self.n:] == SENTINEL).all()), "%s: written outside the tensor" % (what,)
        got = flat[self.lead:self.lead + self.n].reshape(self.shape)
        assert not bool(torch.isnan(got).any()), "%s: elements left unwritten" % (what,)
        assert R.same_values(got, want), what


def _ptr(t):
    return t.data_ptr() if t.numel() else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _levels_arg(ptrs):
    import ctypes as C
    return (C.c_void_p * 4)(*(list(ptrs) + [None] * (4 - len(ptrs))))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("W2", R.FILL_W2)
def test_capi_every_element_is_written_and_nothing_else(W2, dtype):
    lib = _capi.lib()
    dt = K._DT[dtype]
    N, H1, W1 = R.FILL_NHW
    r, levels = R.FILL_R, R.FILL_LEVELS
    rd = 2 * r + 1
    sc = R.special_coords(W2, r, "E")
    c = sc[torch.from_numpy(np.random.default_rng(R._seed("E", W2)).permutation(sc.numel())[:N * H1 * W1])].reshape(N, 1, H1, W1)
    cd = c.to(DEV).contiguous()
    wl = R.widths(W2, levels)
    # sampler
    vol = R.randn((N, H1, W1, W2), ("E", W2), _half(dtype))
    gout = R.randn((N, rd, H1, W1), ("E-g", W2), _half(dtype))
    vd, gd = vol.to(DEV, dtype), gout.to(DEV, dtype)
    out = Guarded((N, rd, H1, W1), dtype)
    assert lib.cs_forward(vd.data_ptr(), cd.data_ptr(), out.ptr, N, H1, W1, W2, r, dt, _stream()) == 0
    out.check(_as(R.twin_forward(vol, c, r), dtype), "cs_forward")
    for lead in (64, 65):       # 64: 16-byte aligned -- k_cs_bwd4 where W2 % 4 == 0; 65: misaligned -- k_cs_bwd for every W2
        gv = Guarded((N, H1, W1, W2), dtype, lead)
        assert (gv.ptr % 16 == 0) == (lead == 64)
        assert lib.cs_backward(cd.data_ptr(), gd.data_ptr(), gv.ptr, N, H1, W1, W2, r, dt, _stream()) == 0
        gv.check(_as(R.twin_backward(c, gout, W2, r), dtype), "cs_backward lead %d" % lead)
    # fused lookup: W2 = 4 and 5 have a level of width 0, which travels as NULL
    pyr = _pyramid(N, H1, W1, W2, levels, ("E-l", W2), _half(dtype))
    gl = R.randn((N, levels * rd, H1, W1), ("E-lg", W2), _half(dtype))
    pd, gld = [p.to(DEV, dtype) for p in pyr], gl.to(DEV, dtype)
    out = Guarded((N, levels * rd, H1, W1), dtype)
    assert lib.cs_lookup_forward(_levels_arg([_ptr(p) for p in pd]), cd.data_ptr(), out.ptr, N, H1, W1, W2, levels, r, dt, _stream()) == 0
    out.check(_as(R.twin_lookup(pyr, c, r), dtype), "cs_lookup_forward")
    gps = [Guarded((N, H1, W1, w), dtype) for w in wl]
    assert lib.cs_lookup_backward(cd.data_ptr(), gld.data_ptr(), _levels_arg([g.ptr for g in gps]), N, H1, W1, W2, levels, r, dt, _stream()) == 0
    for l, (g, want) in enumerate(zip(gps, R.twin_lookup_backward(wl, c, gl, r))):
        g.check(_as(want, dtype), "cs_lookup_backward level %d" % l)


def test_capi_null_pointers_of_empty_levels_are_accepted():
    """W2 = 1 with four levels: levels 1..3 have no element and travel as NULL (the refusing side: tests/test_capi_corr_lookup.py)."""
    lib = _capi.lib()
    N, H1, W1, W2, levels, r = 1, 2, 9, 1, 4, 1
    rd = 2 * r + 1
    c = R.special_coords(W2, r, "E0")[:N * H1 * W1].reshape(N, 1, H1, W1)
    v0 = R.randn((N, H1, W1, W2), "E0")
    gl = R.randn((N, levels * rd, H1, W1), "E0-g")
    cd, vd, gld = c.to(DEV), v0.to(DEV), gl.to(DEV)
    out = Guarded((N, levels * rd, H1, W1), torch.float32)
    assert lib.cs_lookup_forward(_levels_arg([vd.data_ptr(), None, None, None]), cd.data_ptr(), out.ptr, N, H1, W1, W2, levels, r, 0, _stream()) == 0
    empty = [torch.zeros(N, H1, W1, 0)] * 3
    out.check(R.twin_lookup([v0] + empty, c, r), "cs_lookup_forward")
    g0 = Guarded((N, H1, W1, W2), torch.float32)
    assert lib.cs_lookup_backward(cd.data_ptr(), gld.data_ptr(), _levels_arg([g0.ptr, None, None, None]), N, H1, W1, W2, levels, r, 0, _stream()) == 0
    g0.check(R.twin_lookup_backward([1, 0, 0, 0], c, gl, r)[0], "cs_lookup_backward")


# ---- F. misaligned grad_volume ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_capi_misaligned_gradient_takes_the_scalar_kernel_and_gives_the_same_values(dtype):
    """W2 = 8: an aligned grad_volume runs k_cs_bwd4, the same buffer one element further runs k_cs_bwd; both give the same bits."""
    lib = _capi.lib()
    N, H1, W2, r = 2, 2, 8, 4
    c = R.coords_grid(W2, r, N, H1, "F")
    W1 = c.shape[-1]
    gout = R.randn((N, 2 * r + 1, H1, W1), "F", _half(dtype))
    cd, gd = c.to(DEV), gout.to(DEV, dtype)
    n = N * H1 * W1 * W2
    res = []
    for off in (0, 1):
        buf = torch.full((n + 8,), SENTINEL, dtype=dtype, device=DEV)
        view = buf[off:off + n]
        assert (view.data_ptr() % 16 == 0) == (off == 0)
        assert lib.cs_backward(cd.data_ptr(), gd.data_ptr(), view.data_ptr(), N, H1, W1, W2, r, K._DT[dtype], _stream()) == 0
        host = buf.cpu()
        assert bool((host[:off] == SENTINEL).all()) and bool((host[off + n:] == SENTINEL).all())
        res.append(host[off:off + n].reshape(N, H1, W1, W2).clone())
    assert R.same_bits(res[0], res[1])
    assert R.same_values(res[1], _as(R.twin_backward(c, gout, W2, r), dtype))


# ---- G. the Python layer ------------------------------------------------------------------------------------------------------------
def _g_case(dtype):
    N, H1, W1, W2, r = 2, 3, 10, 9, 2
    c = R.eighths((N, 1, H1, W1), -r - 2, W2 + r + 2, "G").to(DEV)     # multiples of 1/8 below 16: representable in fp16
    vol = R.randn((N, H1, W1, W2), "G", _half(dtype)).to(DEV, dtype)
    gout = R.randn((N, 2 * r + 1, H1, W1), "G-g").to(DEV)                # fp32, not fp16-representable
    return N, H1, W1, W2, r, c, vol, gout


def _coords_forms(c):
    N, _, H1, W1 = c.shape
    two = torch.cat([c, torch.full_like(c, 1e4)], 1)                     # [N,2,H,W]: channel 0 is the coordinate
    wide = torch.full((N, 3, H1, 2 * W1), -55.0, device=c.device)
    wide[:, 1:2, :, ::2] = c
    forms = {"two-channel": two, "fp64": c.double(), "fp16": c.half(), "strided": wide[:, 1:2, :, ::2]}
    assert not forms["strided"].is_contiguous() and torch.equal(forms["fp16"].float(), c)
    return forms


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_python_layer_normalises_its_arguments(dtype):
    N, H1, W1, W2, r, c, vol, gout = _g_case(dtype)
    out, = K.forward(vol, c, r)
    gplain = gout.to(dtype)
    gv, = K.backward(vol, c, gplain, r)
    for name, form in _coords_forms(c).items():
        o, = K.forward(vol, form, r)
        g, = K.backward(vol, form, gplain, r)
        assert R.same_bits(o, out) and R.same_bits(g, gv), name
    # a permuted, non-contiguous volume
    vperm = vol.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    assert not vperm.is_contiguous() and torch.equal(vperm, vol)
    o, = K.forward(vperm, c, r)
    g, = K.backward(vperm, c, gplain, r)
    assert R.same_bits(o, out) and R.same_bits(g, gv)
    # grad_output: non-contiguous; fp32 under the volume's dtype (cast once, as the plain call's gradient was)
    gstr = gplain.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not gstr.is_contiguous()
    g, = K.backward(vol, c, gstr, r)
    assert R.same_bits(g, gv)
    g, = K.backward(vol, c, gout, r)
    assert g.dtype == dtype and R.same_bits(g, gv)
    # the autograd wrapper
    v = vol.clone().requires_grad_(True)
    o = K.CorrSampler.apply(v, _coords_forms(c)["two-channel"], r)
    o.backward(gstr)
    assert R.same_bits(o.detach(), out) and R.same_bits(v.grad, gv)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_python_layer_of_the_fused_lookup_normalises_its_arguments(dtype):
    """CorrBlockFast1D.__call__ with the reference's [N,2,H,W] coords (and the other forms) against _LookupPyramid on contiguous fp32 [N,1,H,W]."""
    N, D, H1, W1, W2, r = 2, 8, 3, 10, 9, 2
    f1 = R.randn((N, D, H1, W1), "G-f1", True).to(DEV, dtype).requires_grad_(True)
    f2 = R.randn((N, D, H1, W2), "G-f2", True).to(DEV, dtype)
    blk = K.CorrBlockFast1D(f1, f2, num_levels=4, radius=r)
    c = R.eighths((N, 1, H1, W1), -r - 2, W2 + r + 2, "G").to(DEV)
    gout = R.randn((N, 4 * (2 * r + 1), H1, W1), "G-lg").to(DEV)
    assert [v.shape[-1] for v in blk.volumes] == [9, 4, 2, 1]
    live = [v for v in blk.volumes]
    out = K._LookupPyramid.apply(c, r, *live)
    grads = torch.autograd.grad(out, live, gout.to(dtype), retain_graph=True)
    for name, form in _coords_forms(c).items():
        o = blk(form)
        assert R.same_bits(o.detach(), out.detach()), name
        gstr = gout.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)       # fp32 and non-contiguous under either dtype
        gs = torch.autograd.grad(o, live, gstr, retain_graph=True)
        for l, (a, b) in enumerate(zip(gs, grads)):
            assert a.dtype == dtype and R.same_bits(a, b), (name, l)


def test_python_layer_misuse_raises_runtime_error():
    N, H1, W1, W2, r, c, vol, gout = _g_case(torch.float32)
    pyr = [torch.zeros(N, H1, W1, W2 >> l, device=DEV) for l in range(4)]
    bad = [
        lambda: K.forward(vol, c[:, 0], r),                                              # coords: wrong rank
        lambda: K.forward(vol, c[:, :, :, :-1], r),                                      # coords: wrong width
        lambda: K.forward(vol, c[:1], r),                                                # coords: wrong batch
        lambda: K.forward(vol, c[:, :0], r),                                             # coords: no channel
        lambda: K.backward(vol, c[:, :, :-1], gout, r),
        lambda: K.backward(vol, c, gout[:, :-1], r),                                     # grad_output: wrong tap count
        lambda: K.backward(vol, c, gout[:, :, :, :-1], r),                               # grad_output: wrong width
        lambda: K.backward(vol, c, gout[0], r),                                          # grad_output: wrong rank
        lambda: K.forward(vol, c, -1),                                                   # radius < 0
        lambda: K.backward(vol, c, gout, -1),
        lambda: K._LookupPyramid.apply(c, -1, *pyr),
        lambda: K._LookupPyramid.apply(c[:, 0], r, *pyr),
        lambda: K._LookupPyramid.apply(c, r, pyr[0], torch.zeros(N, H1, W1, (W2 >> 1) + 1, device=DEV)),         # a level of wrong width
        lambda: K._LookupPyramid.apply(c, r, pyr[0], pyr[1].half()),                     # ... of wrong dtype
        lambda: K._LookupPyramid.apply(c, r, pyr[0], torch.zeros(N, H1, W2 >> 1, W1, device=DEV).permute(0, 1, 3, 2)),   # ... non-contiguous
        lambda: K._LookupPyramid.apply(c, r, *(pyr + [torch.zeros(N, H1, W1, 0, device=DEV)])),                  # five levels
        lambda: K._LookupPyramid.apply(c, r),                                            # none
        lambda: K._ptr_array(pyr + [None]),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(RuntimeError):
            f()
            pytest.fail("case %d raised nothing" % i)
    # a gradient of the wrong shape never reaches the kernel: autograd refuses it
    v = vol.clone().requires_grad_(True)
    o = K._LookupPyramid.apply(c, r, v)
    with pytest.raises(RuntimeError):
        o.backward(gout[:, :-1])
