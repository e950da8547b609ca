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
import json
import zlib

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import gps_gaussian_amd  # noqa: F401
from gps_gaussian_amd import _capi, accelerate as A
from gps_gaussian_amd import conv1x1 as C1

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
KEYS = ("y", "dx", "dw", "db")


@pytest.fixture(scope="module", autouse=True)
def _counters():
    A.counters("conv1x1")
    yield
    A.restore()      # the process's counter keys are what they were


def _gamma(n):
    return n * U / (1.0 - n * U)


@functools.lru_cache(maxsize=None)
def _tile():
    import ctypes as C
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    assert _capi.lib().c1_tile(C.byref(a), C.byref(b), C.byref(c)) == 0
    return a.value, b.value, c.value


@functools.lru_cache(maxsize=None)
def _group():
    """The reduction's group size G, read off c1_scratch_bytes: scratch = 4 M (parts + groups) with groups = ceil(parts / G), so the first tile
    count whose scratch holds two group sums is G + 1."""
    _, WP, PARTS = _tile()
    M = 16 * (4 + 1)
    for t in range(1, PARTS + 1):
        extra = _capi.lib().c1_scratch_bytes(1, 4, 16, 1, t * WP, 1) // (4 * M) - t
        assert extra in (1, 2)
        if extra == 2:
            return t - 1
    raise AssertionError("no group boundary below the cap on the partial sums")


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


def _ref64(x, w, b, dy, stride):
    """The fp64 convolution with its gradients, and the same sums over absolute values (what the bounds are made of)."""
    out = {}
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    y = F.conv2d(x64, w64, b64, stride=stride)
    y.backward(dy.double())
    out.update(y=y.detach(), dx=x64.grad, dw=w64.grad, db=b64.grad)
    xa, wa, ba = (t.double().abs().requires_grad_(True) for t in (x, w, b))
    ya = F.conv2d(xa, wa, ba, stride=stride)
    ya.backward(dy.double().abs())
    out.update(abs_y=ya.detach(), abs_dx=xa.grad, abs_dw=wa.grad, abs_db=ba.grad)
    return out


def _bounds(ref, Ci, Co):
    P = ref["y"].numel() // Co                                     # N H_out W_out
    return dict(y=_gamma(Ci + 1) * ref["abs_y"], dx=_gamma(Co) * ref["abs_dx"], dw=_gamma(P) * ref["abs_dw"], db=_gamma(P) * ref["abs_db"])


def _out_hw(H, W, s):
    return (H - 1) // s + 1, (W - 1) // s + 1


def _inputs(name, N, Ci, Co, H, W, s):
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    x = torch.randn((N, Ci, H, W), generator=gen)
    w = torch.randn((Co, Ci, 1, 1), generator=gen) * 0.2
    b = torch.randn((Co,), generator=gen)
    w[Co // 2] = 0.0                    # one exact-zero filter
    dy = torch.randn((N, Co) + _out_hw(H, W, s), generator=gen)
    ref = _ref64(x, w, b, dy, s)
    return dict(dims=(N, Ci, Co, H, W, s), stride=s, x=x, w=w, b=b, dy=dy, ref=ref, bounds=_bounds(ref, Ci, Co))


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs, the fp64 reference and the bounds of one case: computed once, shared by every test that needs them, never modified."""
    return _inputs(name, *_cases()[name])


def _run(x, w, b, dy, stride, backward=True):
    xg, wg, bg = (t.cuda().requires_grad_(backward) for t in (x, w, b))
    y = C1.conv1x1(xg, wg, bg, stride)
    if backward:
        y.backward(dy.cuda())
    torch.cuda.synchronize()
    return dict(y=y.detach(), dx=xg.grad, dw=wg.grad, db=bg.grad)


def _ratio(t, t64, bound):
    """The worst error / bound; an error of zero is inside any bound (also a bound of zero), an error above a zero bound is infinite."""
    d = (t.detach().double().cpu() - t64).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / bound.clamp_min(1e-300))
    return float(r.max())


def _check(test, name, got, c, who="fused"):
    rec = dict(test=test, case=name, dims=list(c["dims"]), who=who, ratio={})
    for k in KEYS:
        assert got[k].shape == c["ref"][k].shape and got[k].dtype == torch.float32, k
        rec["ratio"][k] = _ratio(got[k], c["ref"][k], c["bounds"][k])
    print(json.dumps(rec))
    for k in KEYS:
        assert torch.isfinite(got[k]).all(), k
        assert rec["ratio"][k] <= 1.0, "%s %s %s: error / bound = %.3f" % (who, name, k, rec["ratio"][k])


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
    got = _run(c["x"], c["w"], c["b"], c["dy"], s)
    _check("fp32", name, got, c)
    if s == 2:
        _assert_plus_zero_where_unsampled(got["dx"], H, W, s)


def test_the_input_gradient_of_an_even_plane_is_plus_zero_where_nothing_was_sampled():
    """[2,48,6,8] -> 96, stride 2: rows 0, 2, 4 and columns 0, 2, 4, 6 are sampled; row 5 and column 7 never are.  dx goes in holding NaN bit
    patterns wherever torch.empty leaves them, and comes back with +0.0 at 36 of the 48 positions of each of its 96 planes."""
    c = _case("even_plane_s2")
    N, Ci, Co, H, W, s = c["dims"]
    assert (N, Ci, H, W, s) == (2, 48, 6, 8, 2)
    got = _run(c["x"], c["w"], c["b"], c["dy"], s)
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


def _ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


@pytest.mark.parametrize("which", ["cin128_s1_tile+1", "cin48_s2_two_tiles", "cin32_s2_odd"])
def test_small_integers_give_the_exact_answer(which):
    """x in [-3, 3], w, b, dy in [-2, 2]: every product and partial sum is an integer far below 2^24, so y, dx, dw, db must EQUAL the fp64 result."""
    TP = _tile()[0]
    N, Ci, Co, H, W, s = {"cin128_s1_tile+1": (2, 128, 48) + _factor(TP + 1) + (1,), "cin48_s2_two_tiles": (1, 48, 96, 34, 36, 2),
                          "cin32_s2_odd": (3, 32, 64, 5, 7, 2)}[which]
    gen = torch.Generator().manual_seed(zlib.crc32(which.encode()))
    x, w, b = _ints((N, Ci, H, W), -3, 3, gen), _ints((Co, Ci, 1, 1), -2, 2, gen), _ints((Co,), -2, 2, gen)
    dy = _ints((N, Co) + _out_hw(H, W, s), -2, 2, gen)
    ref = _ref64(x, w, b, dy, s)
    got = _run(x, w, b, dy, s)
    for k in KEYS:
        assert torch.equal(got[k].double().cpu(), ref[k]), k
    if s == 2:
        _assert_plus_zero_where_unsampled(got["dx"], H, W, s)


def test_two_runs_give_the_same_bits():
    for name in ("two_tiles_odd_s2", "cin192_96", "group+1"):
        c = _case(name)
        a = _run(c["x"], c["w"], c["b"], c["dy"], c["stride"])
        b = _run(c["x"], c["w"], c["b"], c["dy"], c["stride"])
        for k in KEYS:
            assert torch.equal(a[k], b[k]), (name, k)


@pytest.mark.parametrize("name", ["cin192_64", "two_tiles_even_s2"])
def test_requires_grad_handling(name):
    c = _case(name)
    s = c["stride"]
    full = _run(c["x"], c["w"], c["b"], c["dy"], s)
    x, w, b, dy = (c[k].cuda() for k in ("x", "w", "b", "dy"))
    # a frozen input: no input gradient, the same parameter gradients
    wg, bg = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = C1.conv1x1(x, wg, bg, s)
    y.backward(dy)
    assert x.grad is None and torch.equal(y.detach(), full["y"]) and torch.equal(wg.grad, full["dw"]) and torch.equal(bg.grad, full["db"])
    # frozen parameters: only the input gradient
    xg = x.clone().requires_grad_(True)
    C1.conv1x1(xg, w, b, s).backward(dy)
    assert w.grad is None and b.grad is None and torch.equal(xg.grad, full["dx"])
    # the bias only, then the weight only
    bg = b.clone().requires_grad_(True)
    C1.conv1x1(x, w, bg, s).backward(dy)
    assert w.grad is None and x.grad is None and torch.equal(bg.grad, full["db"])
    wg = w.clone().requires_grad_(True)
    C1.conv1x1(x, wg, b, s).backward(dy)
    assert b.grad is None and torch.equal(wg.grad, full["dw"])
    with torch.no_grad():
        y0 = C1.conv1x1(x, wg, bg, s)
    assert y0.grad_fn is None and torch.equal(y0, full["y"])
    # gradients in the parameters' dtypes and shapes
    wd = w.double().requires_grad_(True)
    C1.conv1x1(x, wd, b, s).backward(dy)
    assert wd.grad.dtype == torch.float64 and wd.grad.shape == w.shape and torch.equal(wd.grad.float(), full["dw"])


@pytest.mark.parametrize("name", ["odd_plane_s2", "cin192_96"])
def test_a_strided_or_misaligned_dy_gives_the_same_bits(name):
    c = _case(name)
    s = c["stride"]
    full = _run(c["x"], c["w"], c["b"], c["dy"], s)
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
        ref = _ref64(x.cpu(), w, b, cap["dy"].cpu(), s)
        c = dict(dims=dims, ref=ref, bounds=_bounds(ref, Ci, Co))
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

    def both(a, b, inp, **ac):
        n0, p0 = A.calls["conv1x1"], A.calls["conv1x1_passthrough"]
        with torch.autocast("cuda", enabled=bool(ac), **ac):
            ya, yb = a(inp), b(inp)
        assert A.calls["conv1x1"] == n0 and A.calls["conv1x1_passthrough"] == p0 + 1
        assert ya.dtype == yb.dtype and ya.shape == yb.shape and ya.stride() == yb.stride() and torch.equal(ya, yb)

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
