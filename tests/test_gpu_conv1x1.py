"""GPU (-m gpu): the 1x1 matrix-core convolution (csrc/conv1x1.hip; conv1x1.conv1x1 / FusedConv1x1) against F.conv2d and its autograd in fp64 on
the CPU, starting from the same fp32 inputs.  The edge shapes come from c1_tile -- the forward's pixel tile TP, the weight gradient's pixel tile WP
and the cap PARTS on its partial sums -- and from c1_scratch_bytes (the reduction's group size), not from numbers written down here.

The bounds are derived, not measured, and hold for any summation order.  With u = 2^-24 and g(n) = n u / (1 - n u), elementwise:
    y        |y - y64| <= g(C_in + 1) (sum |w||x| + |b|)
    dx       <= g(C_out) sum |w||dy|
    dw, db   <= g(P) sum |dy||x|,  g(P) sum |dy|,   P = N H_out W_out
the sums of absolute values come from the same fp64 convolution (and its autograd) applied to |x|, |w|, |b|, |dy|.

ATen's convolution runs on the GPU in two tests only: the pass-through cases (forward; the converted module against the plain one, the same ATen
call twice) and the block test, whose unconverted block is what the converted one is compared with."""
import copy
import functools
import zlib

import pytest
import torch
from torch import nn

import gps_gaussian_amd  # noqa: F401
from gps_gaussian_amd import _capi, accelerate as A
from gps_gaussian_amd import conv1x1 as C1

import convop_run as R
from convop_run import KEYS, gamma

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _counters():
    A.counters("conv1x1")
    yield
    A.restore()      # the process's counter keys are what they were


_tile = C1.tile


@functools.lru_cache(maxsize=None)
def _group():
    """The reduction's group size G, read off c1_scratch_bytes: 4 M (parts + groups) bytes for the M = C_out (C_in + 1) sums of [1,4,1,t WP] -> 16."""
    _, WP, PARTS = _tile()
    return R.group_size(lambda t: _capi.lib().c1_scratch_bytes(1, 4, 16, 1, t * WP, 1) // (4 * 16 * (4 + 1)), PARTS)


def _factor(n):
    """(h, w) with h w = n, as square as it goes."""
    h = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
    return h, n // h


@functools.lru_cache(maxsize=None)
def _cases():
    """name -> (N, C_in, C_out, H, W, stride)"""
    TP, WP, PARTS = _tile()
    G = _group()
    c = {"one_pixel_s1": (1, 4, 16, 1, 1, 1), "one_pixel_s2": (1, 4, 16, 1, 1, 2)}
    for tag, n in (("TP-1", TP - 1), ("TP", TP), ("TP+1", TP + 1)):
        c["tile_%s" % tag] = (1, 128, 48) + _factor(n) + (1,)
    c["odd_plane_s2"] = (3, 32, 48, 5, 7, 2)                       # smaller than a tile, over several images
    c["even_plane_s2"] = (2, 48, 96, 6, 8, 2)                      # the last row and column are never sampled
    c["cin192_64"] = (1, 192, 64, 9, 11, 1)
    c["cin192_96"] = (1, 192, 96, 9, 11, 1)
    c["limits_256_128"] = (1, 256, 128, 3, 5, 1)
    c["parts+1"] = (1, 4, 16, 1, WP * PARTS + 1, 1)                # PARTS + 1 weight-gradient tiles: workgroup 0 walks two
    c["group+1"] = (1, 4, 16, 1, WP * G + 1, 1)                    # G + 1 partial sums: two groups in the reduction
    c["two_tiles_odd_s2"] = (2, 32, 48, 37, 41, 2)                 # 19 x 21 = 399 output pixels: two forward tiles, odd rows (scalar quad stores)
    c["two_tiles_even_s2"] = (1, 48, 96, 34, 36, 2)                # 17 x 18 = 306: two tiles, even rows (paired quad stores)
    c["cin20_tail"] = (2, 20, 32, 7, 9, 1)                         # C_in = 16 + 4: the last chunk of channels is a quarter full
    return c


CASES = ["one_pixel_s1", "one_pixel_s2", "tile_TP-1", "tile_TP", "tile_TP+1", "odd_plane_s2", "even_plane_s2", "cin192_64", "cin192_96",
         "limits_256_128", "parts+1", "group+1", "two_tiles_odd_s2", "two_tiles_even_s2", "cin20_tail"]


def _bounds(ref, N, Ci, Co, H, W, s):
    P = ref["y"].numel() // Co                                     # N H_out W_out
    return dict(y=gamma(Ci + 1) * ref["abs_y"], dx=gamma(Co) * ref["abs_dx"], dw=gamma(P) * ref["abs_dw"], db=gamma(P) * ref["abs_db"])


def _out_hw(H, W, s):
    return (H - 1) // s + 1, (W - 1) // s + 1


def _inputs(gen, N, Ci, Co, H, W, s):
    x = torch.randn((N, Ci, H, W), generator=gen)
    w = torch.randn((Co, Ci, 1, 1), generator=gen) * 0.2
    b = torch.randn((Co,), generator=gen)
    w[Co // 2] = 0.0                    # one exact-zero filter
    dy = torch.randn((N, Co) + _out_hw(H, W, s), generator=gen)
    return dict(x=x, w=w, b=b, dy=dy, conv=dict(stride=s))


_case = R.case_cache(_cases, _inputs, _bounds)


def _op(stride):
    return lambda x, w, b: C1.conv1x1(x, w, b, stride)


def _run(c):
    return R.run_case(_op(c["conv"]["stride"]), c)


def _check(test, name, got, c, who="fused"):
    R.check(dict(test=test, case=name, dims=list(c["dims"]), who=who), "ratio", got, c["ref"], c["bounds"])


def _unsampled(H, W, s):
    """[H, W] bool: the positions of a plane a stride-s 1x1 convolution never reads."""
    m = torch.ones(H, W, dtype=torch.bool)
    m[::s, ::s] = False
    return m


def _assert_plus_zero_where_unsampled(dx, H, W, s):
    """dx is +0.0 -- the bit pattern, not just == 0 -- at every position the forward did not sample.  -> how many such positions."""
    m = _unsampled(H, W, s)
    bits = dx.detach().cpu().contiguous().view(torch.int32)[:, :, m]
    assert int((bits != 0).sum()) == 0
    return bits.numel()


@pytest.mark.parametrize("name", CASES)
def test_forward_and_backward_within_the_bounds(name):
    c = _case(name)
    N, Ci, Co, H, W, s = c["dims"]
    got = _run(c)
    _check("fp32", name, got, c)
    if s == 2:
        _assert_plus_zero_where_unsampled(got["dx"], H, W, s)


def test_the_input_gradient_of_an_even_plane_is_plus_zero_where_nothing_was_sampled():
    """[2,48,6,8] -> 96, stride 2: rows 0, 2, 4 and columns 0, 2, 4, 6 are sampled; row 5 and column 7 never are.  dx goes in holding NaN bit
    patterns wherever torch.empty leaves them, and comes back with +0.0 at 36 of the 48 positions of each of its 96 planes."""
    c = _case("even_plane_s2")
    N, Ci, Co, H, W, s = c["dims"]
    assert (N, Ci, H, W, s) == (2, 48, 6, 8, 2)
    got = _run(c)
    assert _assert_plus_zero_where_unsampled(got["dx"], H, W, s) == N * Ci * (H * W - 3 * 4) == 3456
    m = _unsampled(H, W, s)
    assert bool(m[5].all()) and bool(m[:, 7].all()) and int((~m).sum()) == 12
    sampled = got["dx"].cpu()[:, :, ~m]
    assert int((sampled != 0).sum()) == sampled.numel()            # and the sampled positions carry the gradient
    # the same through the C-ABI with dx pre-filled: every element is written
    x, w, dy = (c[k].cuda() for k in ("x", "w", "dy"))
    dx = torch.full_like(x, float("nan"))
    from gps_gaussian_amd._ops import call, ptr
    call("c1_backward", x.device, ptr(x), ptr(w), ptr(dy), N, Ci, Co, H, W, s, ptr(dx), None, None, None)
    torch.cuda.synchronize()
    assert torch.equal(dx, got["dx"])


@pytest.mark.parametrize("which", ["cin128_s1_tile+1", "cin48_s2_two_tiles", "cin32_s2_odd"])
def test_small_integers_give_the_exact_answer(which):
    TP = _tile()[0]
    N, Ci, Co, H, W, s = {"cin128_s1_tile+1": (2, 128, 48) + _factor(TP + 1) + (1,), "cin48_s2_two_tiles": (1, 48, 96, 34, 36, 2),
                          "cin32_s2_odd": (3, 32, 64, 5, 7, 2)}[which]
    got, _ = R.exact_integers(which, _op(s), ((N, Ci, H, W), (Co, Ci, 1, 1), (Co,), (N, Co) + _out_hw(H, W, s)), stride=s)
    if s == 2:
        _assert_plus_zero_where_unsampled(got["dx"], H, W, s)


def test_two_runs_give_the_same_bits():
    R.two_runs(_run, [(name, _case(name)) for name in ("two_tiles_odd_s2", "cin192_96", "group+1")])


@pytest.mark.parametrize("name", ["cin192_64", "two_tiles_even_s2"])
def test_requires_grad_handling(name, monkeypatch):
    c = _case(name)
    R.requires_grad_matrix(monkeypatch, C1, "c1_backward", _op(c["conv"]["stride"]), c)


@pytest.mark.parametrize("name", ["odd_plane_s2", "cin192_96"])
def test_a_strided_or_misaligned_dy_gives_the_same_bits(name):
    c = _case(name)
    s = c["conv"]["stride"]
    full = _run(c)
    dy = c["dy"].cuda()

    def backward_with(g):
        xg, wg, bg = (c[k].cuda().requires_grad_(True) for k in ("x", "w", "b"))
        C1.conv1x1(xg, wg, bg, s).backward(g)
        torch.cuda.synchronize()
        return dict(dx=xg.grad, dw=wg.grad, db=bg.grad)

    # channels-last strides, a transposed view, and a view that starts one element into a larger buffer (4-byte aligned only)
    cl = dy.contiguous(memory_format=torch.channels_last)
    tr = dy.transpose(2, 3).contiguous().transpose(2, 3)
    buf = torch.empty(dy.numel() + 1, device="cuda")
    off = buf[1:].view(dy.shape)
    off.copy_(dy)
    assert not tr.is_contiguous() and off.data_ptr() % 16 != 0
    for g in (cl, tr, off):
        got = backward_with(g)
        for k in ("dx", "dw", "db"):
            assert torch.equal(got[k], full[k]), k


def test_cpu_tensors_and_unsupported_configurations_are_an_error():
    with pytest.raises(RuntimeError, match="GPU"):
        C1.conv1x1(torch.zeros(1, 4, 3, 3), torch.zeros(16, 4, 1, 1), torch.zeros(16))
    z = lambda *s: torch.zeros(*s, device="cuda")
    for args in ((z(1, 6, 3, 3), z(16, 6, 1, 1), z(16)), (z(1, 8, 3, 3), z(24, 8, 1, 1), z(24)), (z(1, 8, 3, 3), z(16, 8, 1, 1), z(16), 3),
                 (z(1, 8, 3, 3), z(16, 8, 3, 3), z(16)), (z(1, 8, 3, 3).half(), z(16, 8, 1, 1), z(16)), (z(1, 8, 3, 3), z(16, 8, 1, 1), None)):
        with pytest.raises(RuntimeError):
            C1.conv1x1(*args)


class Block(nn.Module):
    """core/extractor.py's ResidualBlock with norm_fn 'group': the shortcut is Sequential(Conv2d(in_planes, planes, 1, stride), norm3)."""

    def __init__(self, in_planes, planes, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, planes, 3, padding=1, stride=stride)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1)
        self.relu = nn.ReLU(inplace=True)
        self.norm1, self.norm2, self.norm3 = (nn.GroupNorm(planes // 8, planes) for _ in range(3))
        self.downsample = nn.Sequential(nn.Conv2d(in_planes, planes, 1, stride=stride), self.norm3)

    def forward(self, x):
        y = self.relu(self.norm1(self.conv1(x)))
        y = self.relu(self.norm2(self.conv2(y)))
        return self.relu(self.downsample(x) + y)


@pytest.mark.parametrize("dims", [(2, 32, 48, 21, 27, 2), (1, 48, 96, 12, 23, 2)], ids=["res2_s2", "res3_s2"])
def test_a_converted_block_against_the_unconverted_block(dims):
    """Both blocks run forward and backward on the GPU from the same parameters and input.  What goes into and comes out of the shortcut's 1x1 layer
    is taken with hooks -- its input, its output, the gradient that reaches it, the input gradient it hands back -- and both layers are held to the
    bounds at the top against fp64 from THEIR OWN captured input and gradient (the gradient reaching the layer has been through a ReLU mask and a
    GroupNorm that saw the other layer's rounding).  The converted block reached the fused op once and never passed through."""
    N, Ci, Co, H, W, s = dims
    torch.manual_seed(zlib.crc32(repr(dims).encode()))
    plain = Block(Ci, Co, s).cuda()
    fused = copy.deepcopy(plain)
    assert C1.convert(fused) == 1 and type(fused.downsample[0]) is C1.FusedConv1x1 and type(plain.downsample[0]) is nn.Conv2d
    x = torch.randn(N, Ci, H, W, device="cuda")
    g = torch.randn((N, Co) + _out_hw(H, W, s), device="cuda")
    res = {}
    for who, net in (("aten", plain), ("fused", fused)):
        cap = {}
        layer = net.downsample[0]
        h1 = layer.register_forward_hook(lambda m, i, o, cap=cap: cap.update(x=i[0].detach(), y=o.detach()))
        h2 = layer.register_full_backward_hook(lambda m, gi, go, cap=cap: cap.update(dx=gi[0].detach(), dy=go[0].detach()))
        n0, p0 = A.calls["conv1x1"], A.calls["conv1x1_passthrough"]
        xin = x.clone().requires_grad_(True)
        out = net(xin)
        out.backward(g)
        torch.cuda.synchronize()
        h1.remove()
        h2.remove()
        assert (A.calls["conv1x1"] - n0, A.calls["conv1x1_passthrough"] - p0) == ((1, 0) if who == "fused" else (0, 0))
        assert torch.equal(cap["x"], x)
        w, b = layer.weight.detach().cpu(), layer.bias.detach().cpu()
        ref = R.ref64(x, w, b, cap["dy"], stride=s)
        c = dict(dims=dims, ref=ref, bounds=_bounds(ref, *dims))
        _check("block", "x".join(map(str, dims)), dict(y=cap["y"], dx=cap["dx"], dw=layer.weight.grad, db=layer.bias.grad), c, who=who)
        res[who] = (out.detach(), xin.grad)
    for a, b in zip(res["aten"], res["fused"]):
        assert a.shape == b.shape and torch.isfinite(b).all()


def test_a_stride_1_input_with_fewer_workgroups_than_compute_units_is_atens():
    """The one row of profiles/conv1x1_shapes.md on which the fused op lost: stride 1 with fewer workgroups of the forward than the device has
    compute units (decoder3[0] on one stereo pair).  One workgroup per compute unit is the fused op's, and so is stride 2 at any size."""
    TP = _tile()[0]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    torch.manual_seed(8)
    plain = nn.Conv2d(4, 16, 1).cuda()
    fused = copy.deepcopy(plain)
    fused.__class__ = C1.FusedConv1x1
    few, enough = torch.randn(1, 4, cus - 1, TP, device="cuda"), torch.randn(1, 4, cus, TP, device="cuda")

    def counts(fn):
        n0, p0 = A.calls["conv1x1"], A.calls["conv1x1_passthrough"]
        out = fn()
        return out, A.calls["conv1x1"] - n0, A.calls["conv1x1_passthrough"] - p0

    y, n, p = counts(lambda: fused(few))
    assert (n, p) == (0, 1) and torch.equal(y, plain(few))
    y, n, p = counts(lambda: fused(enough))
    assert (n, p) == (1, 0) and torch.equal(y, C1.conv1x1(enough, plain.weight, plain.bias))
    y, n, p = counts(lambda: fused(torch.randn(2, 4, (cus + 1) // 2, TP, device="cuda")))           # the images of a batch count together
    assert (n, p) == (1, 0)
    s2 = nn.Conv2d(4, 16, 1, stride=2).cuda()
    s2.__class__ = C1.FusedConv1x1
    assert counts(lambda: s2(few[:, :, :3, :5].contiguous()))[1:] == (1, 0)


def test_what_the_op_does_not_take_goes_through_torch():
    torch.manual_seed(4)
    plain = nn.Sequential(nn.Conv2d(32, 48, 1, stride=2)).cuda()
    fused = copy.deepcopy(plain)
    assert C1.convert(fused) == 1 and type(fused[0]) is C1.FusedConv1x1
    plain, fused = plain[0], fused[0]
    x = torch.randn(2, 32, 20, 22, device="cuda")

    both = R.passthrough_pair(A.calls, "conv1x1")

    def forced(m):
        f = copy.deepcopy(m)
        assert C1.convert(nn.Sequential(f)) == 0
        f.__class__ = C1.FusedConv1x1
        return f

    both(plain, fused, x, dtype=torch.float16)                                                    # fp16 autocast
    both(plain, fused, x, dtype=torch.bfloat16)                                                   # bf16 autocast
    both(copy.deepcopy(plain).half(), copy.deepcopy(fused).half(), x.half())                      # fp16 input outside autocast
    both(plain, fused, x.to(memory_format=torch.channels_last))                                   # channels-last input
    nb = nn.Conv2d(32, 48, 1, bias=False).cuda()
    both(nb, forced(nb), x)                                                                       # no bias
    k3 = nn.Conv2d(32, 48, 3, padding=1).cuda()
    both(k3, forced(k3), x)                                                                       # kernel 3
    g2 = nn.Conv2d(32, 48, 1, groups=2).cuda()
    both(g2, forced(g2), x)                                                                       # groups = 2
    c144 = nn.Conv2d(32, 144, 1).cuda()
    both(c144, forced(c144), x)                                                                   # C_out = 144
    both(plain, fused, x[:0])                                                                     # an empty batch
    n0, p0 = A.calls["conv1x1"], A.calls["conv1x1_passthrough"]
    y = fused(x)
    assert y.dtype == torch.float32 and y.shape == (2, 48, 10, 11) and (A.calls["conv1x1"], A.calls["conv1x1_passthrough"]) == (n0 + 1, p0)
    assert torch.equal(y, C1.conv1x1(x, plain.weight, plain.bias, 2))                             # and the ordinary call is the fused one
