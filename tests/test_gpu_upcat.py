"""GPU (-m gpu): the decoder glue (csrc/upcat.hip; upcat.upsample2x_cat, upcat.convert) against the fp64 restatement of upcat_ref.py, on the inputs
test_upcat_ref.py shows every single-error mutant of that restatement to fail on.  The edge shapes come from uc_tile (upcat_ref.cases), not from
numbers written down here.

THE BOUNDS, from the evaluation order the header of csrc/upcat.hip states, with u = 2^-24, element by element:
    forward    every tap pair is fmaf(0.75, near, 0.25 * far): the multiplication by 0.25 is exact, the fmaf rounds once -- one rounding along x, one
               along y, so every one of the four taps of an output passes TWO roundings:  |out - out64| <= K_FWD u sum_i w_i |a_i|,  K_FWD = 2.
    backward   every axis is fmaf(0.75, d1 + d2, 0.25 * (d0 + d3)): each sum rounds once (the two are side by side, not in a chain), the
               multiplication by 0.25 is exact, the fmaf rounds once -- two roundings along x, two along y, so every one of the sixteen taps passes
               FOUR:  |da - da64| <= K_BWD u sum_i w_i |dout_i|,  K_BWD = 4, the sum over the taps with a border element's folded tap counted.
(With |delta| <= u / (1 + u) per rounding, (1 + delta)^2 - 1 <= 2u holds exactly; (1 + delta)^4 - 1 <= 4u holds to first order, the second-order
term is 2 u^2, a 1e-7-th of the bound.)  The skip channels of out and the skips' gradients carry no arithmetic: equal bit for bit.

An output axis has an even length, so the sizes next to a tile edge are TH -+ 2 and 2 TH + 2 rows, TW -+ 2 and 2 TW + 2 columns (w odd) and TW -+ 4,
2 TW + 4 columns (w even, the 16-byte path)."""
import copy
import functools

import numpy as np
import pytest
import torch

import gps_gaussian_amd  # noqa: F401
from gps_gaussian_amd import upcat

import upcat_ref as R
import upcat_standin as S

pytestmark = pytest.mark.gpu

CASES = sorted(R.cases(16, 256))
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _counters():
    before = dict(upcat.calls)
    yield
    upcat.calls.update(before)


@functools.lru_cache(maxsize=None)
def _case(name, integers=False):
    """The inputs and the fp64 reference of a case: computed once, shared, never written to."""
    c = R.make_case(name, *upcat.tile(), integers=integers)
    Ca = c["a"].shape[1]
    return c, R.forward(c["a"], c["skips"]), R.forward_bound(c["a"]), R.backward(c["dout"], Ca), R.backward_bound(c["dout"], Ca)


def _run(c, a_grad=True, skip_grad=True):
    """-> out, a.grad (None without a_grad), the skips' gradients, all as NumPy arrays."""
    a = torch.from_numpy(c["a"]).to(DEV).requires_grad_(a_grad)
    skips = [torch.from_numpy(s).to(DEV).requires_grad_(skip_grad) for s in c["skips"]]
    out = upcat.upsample2x_cat(a, *skips)
    if a_grad or (skip_grad and skips):
        out.backward(torch.from_numpy(c["dout"]).to(DEV))
    torch.cuda.synchronize()
    return out.detach().cpu().numpy(), (a.grad.cpu().numpy() if a_grad else None), [s.grad.cpu().numpy() if skip_grad else None for s in skips]


def test_the_case_table_is_the_one_the_cpu_tests_hold_the_mutants_to():
    assert sorted(R.cases(*upcat.tile())) == CASES


@pytest.mark.parametrize("name", CASES)
def test_forward_and_backward_are_inside_the_bounds(name):
    c, out64, ob, da64, db = _case(name)
    N, Ca, h, w = c["a"].shape
    out, da, ds = _run(c)
    assert out.shape == out64.shape and out.dtype == np.float32 and da.shape == c["a"].shape
    qf, qb = R.worst_ratio(out[:, :Ca], out64[:, :Ca], ob), R.worst_ratio(da, da64, db)
    print(name, "forward: %.3f of the bound, da: %.3f of the bound" % (qf, qb))
    assert qf <= 1.0, qf
    assert qb <= 1.0, qb
    c0 = Ca
    for s, g in zip(c["skips"], ds):
        assert (out[:, c0:c0 + s.shape[1]].view(np.uint32) == s.view(np.uint32)).all()                   # bit for bit
        assert (g.view(np.uint32) == c["dout"][:, c0:c0 + s.shape[1]].view(np.uint32)).all()
        c0 += s.shape[1]
    assert c0 == out.shape[1]
    # the first and last outputs of an axis are the first and last inputs
    assert (out[:, :Ca, 0, 0] == c["a"][:, :, 0, 0]).all() and (out[:, :Ca, -1, -1] == c["a"][:, :, -1, -1]).all()


@pytest.mark.parametrize("name", CASES)
def test_whole_numbers_come_out_exact(name):
    c, out64, _, da64, _ = _case(name, integers=True)
    out, da, _ = _run(c)
    assert (out.astype(np.float64) == out64).all() and (da.astype(np.float64) == da64).all()


@pytest.mark.parametrize("name", ["reference-shaped", "4x6-three-skips", "cols-above-two-tiles", "rows-above-two-tiles"])
def test_two_runs_give_the_same_bits(name):
    c = _case(name)[0]
    (o1, g1, _), (o2, g2, _) = _run(c), _run(c)
    assert (o1.view(np.uint32) == o2.view(np.uint32)).all() and (g1.view(np.uint32) == g2.view(np.uint32)).all()


def test_without_a_gradient_for_a_no_backward_kernel_is_launched(monkeypatch):
    launched = []
    real = upcat.call
    monkeypatch.setattr(upcat, "call", lambda name, *a: (launched.append(name), real(name, *a))[1])
    c = _case("4x6-three-skips")[0]
    Ca = c["a"].shape[1]
    out, da, ds = _run(c, a_grad=False)
    assert launched == ["uc_forward"] and da is None
    c0 = Ca
    for s, g in zip(c["skips"], ds):
        assert (g.view(np.uint32) == c["dout"][:, c0:c0 + s.shape[1]].view(np.uint32)).all()
        c0 += s.shape[1]
    del launched[:]
    out2, da2, ds2 = _run(c, skip_grad=False)
    assert launched == ["uc_forward", "uc_backward"] and ds2 == [None] * 3 and (out2 == out).all()
    assert R.worst_ratio(da2, _case("4x6-three-skips")[3], _case("4x6-three-skips")[4]) <= 1.0


def test_misaligned_views_and_wrong_arguments():
    """A view that starts off a 16-byte boundary is copied to an aligned tensor by the op; what the op does not take is an error in its name."""
    c, out64, ob, _, _ = _case("4x6-three-skips")
    Ca = c["a"].shape[1]
    flat = torch.zeros(c["a"].size + 1, device=DEV)
    flat[1:] = torch.from_numpy(c["a"]).to(DEV).reshape(-1)
    a = flat[1:].view(*c["a"].shape)
    assert a.data_ptr() % 16 == 4
    skips = [torch.from_numpy(s).to(DEV) for s in c["skips"]]
    out = upcat.upsample2x_cat(a, *skips).cpu().numpy()
    assert R.worst_ratio(out[:, :Ca], out64[:, :Ca], ob) <= 1.0 and (out[:, Ca:] == out64[:, Ca:]).all()
    good = torch.from_numpy(c["a"]).to(DEV)
    for bad in ((good.half(),) + tuple(skips), (good, skips[0].double()), (good[0],), (good, skips[0][:, :, :-1]), (good, skips[0][:1]),
                (good.transpose(2, 3),), (good, skips[0], skips[0], skips[0], skips[0]), (good, skips[0].cpu())):
        with pytest.raises(RuntimeError, match="gps_gaussian_amd: upsample2x_cat"):
            upcat.upsample2x_cat(*bad)


@pytest.mark.parametrize("name", ["4x6-three-skips", "3x3-odd-w", "cols-above-tile-vec"])
def test_pointers_four_bytes_off_through_the_c_abi_give_the_same_bits(name):
    """The op hands the kernels 16-byte aligned tensors; the C-ABI takes 4-byte aligned ones and then runs the 4-byte paths of both kernels (the
    backward's is reached no other way).  Same arithmetic, so the same bits as the aligned call."""
    import ctypes
    from gps_gaussian_amd._ops import call, ptr
    c = _case(name)[0]
    N, Ca, h, w = c["a"].shape
    counts = [s.shape[1] for s in c["skips"]]
    out, da, _ = _run(c)

    def off4(x):     # a copy of x that starts 4 bytes behind a 16-byte boundary, with a guard element behind it
        flat = torch.full((x.size + 2,), 7.0, device=DEV)
        flat[1:-1] = torch.from_numpy(x).to(DEV).reshape(-1)
        assert flat.data_ptr() % 16 == 0
        return flat, flat[1:-1]

    dev = torch.device(DEV)
    (_, a), skips, (_, dout) = off4(c["a"]), [off4(s)[1] for s in c["skips"]], off4(c["dout"])
    oflat, o = off4(np.zeros_like(out))
    gflat, g = off4(np.zeros_like(da))
    ptrs = (ctypes.c_void_p * len(skips))(*[ptr(s) for s in skips]) if skips else None
    cnt = (ctypes.c_int * len(counts))(*counts) if counts else None
    call("uc_forward", dev, ptr(a), ptrs, cnt, len(counts), N, Ca, h, w, ptr(o))
    call("uc_backward", dev, ptr(dout), cnt, len(counts), N, Ca, h, w, ptr(g))
    torch.cuda.synchronize()
    assert (o.cpu().numpy().view(np.uint32) == out.reshape(-1).view(np.uint32)).all()
    assert (g.cpu().numpy().view(np.uint32) == da.reshape(-1).view(np.uint32)).all()
    for flat in (oflat, gflat):      # nothing was written in front of or behind the tensors
        assert float(flat[0]) == 7.0 and float(flat[-1]) == 7.0


def _standin_run(model, args, dtype, dev=DEV):
    model = copy.deepcopy(model).to(device=dev, dtype=dtype)
    img, depth, feat = args
    outs = model(img.to(dev, dtype), depth.to(dev, dtype), [f.to(dev, dtype) for f in feat])
    w = [torch.linspace(0.5, 1.5, o.numel(), device=dev, dtype=dtype).view_as(o) for o in outs]     # a fixed, non-uniform loss
    sum((o * v).sum() for o, v in zip(outs, w)).backward()
    if dev != "cpu":
        torch.cuda.synchronize()
    return [o.detach().double().cpu() for o in outs], {k: p.grad.double().cpu() for k, p in model.named_parameters()}


def test_a_converted_stand_in_runs_its_three_sites_fused():
    """The converted stand-in against its own unconverted ATen forward and backward, both in fp32, both measured against the same module in fp64
    (ATen, on the CPU).  Per tensor T (each output, each parameter's gradient):
        max |fused - T64| <= 4 max |aten32 - T64| + 8 u max |T64|
    Why 4: at a glue site the fused op is within 2 u (forward) and 4 u (backward) of the exact taps, ATen's kernel -- interpolation weights computed
    per pixel, two products and a sum per axis -- within a comparable handful of u; from there on both errors pass through the SAME layers, so the two
    ends differ by the ratio of two rounding realisations of the same size, for whose maxima over a tensor a factor of 4 is loose.  The floor of
    8 u max|T| is for a tensor on which ATen's fp32 result happens to be (almost) exact."""
    torch.manual_seed(7)
    plain = S.Regresser()
    fused = copy.deepcopy(plain)
    assert upcat.convert(fused) == 1
    args = S.inputs(N=2, H=24, W=40, seed=11)
    o64, g64 = _standin_run(plain, args, torch.float64, "cpu")
    upcat.calls.update(upcat=0, upcat_passthrough=0)
    o32, g32 = _standin_run(plain, args, torch.float32)
    assert upcat.calls == {"upcat": 0, "upcat_passthrough": 0}
    of, gf = _standin_run(fused, args, torch.float32)
    assert upcat.calls == {"upcat": 3, "upcat_passthrough": 0}
    assert set(gf) == set(g64) and len(of) == 3

    def check(tag, f, a, r):
        ef, ea, scale = float((f - r).abs().max()), float((a - r).abs().max()), float(r.abs().max())
        print("%s: fused %.3e, aten %.3e, scale %.3e" % (tag, ef, ea, scale))
        assert torch.isfinite(f).all() and ef <= 4 * ea + 8 * R.U32 * scale, tag

    for i in range(3):
        check("output %d" % i, of[i], o32[i], o64[i])
    for k in sorted(g64):
        check(k, gf[k], g32[k], g64[k])
    # one site alone: fp64 tensors, autocast and a strided view are not the op's -- the module's own `up` and torch.cat compute them
    m = fused.to(DEV)
    a, k = torch.randn(1, 2, 3, 4, device=DEV), torch.randn(1, 1, 6, 8, device=DEV)
    upcat.calls.update(upcat=0, upcat_passthrough=0)
    assert torch.equal(upcat._glue(m, a.double(), k.double()), torch.cat([m.up(a.double()), k.double()], 1))
    with torch.autocast("cuda", dtype=torch.float16):
        assert torch.equal(upcat._glue(m, a, k), torch.cat([m.up(a), k], 1))
    wide = torch.randn(1, 2, 3, 8, device=DEV)[..., ::2]
    assert torch.equal(upcat._glue(m, wide, k), torch.cat([m.up(wide), k], 1))
    assert upcat.calls == {"upcat": 0, "upcat_passthrough": 3}
    assert upcat._glue(m, a, k).shape == (1, 3, 6, 8) and upcat.calls["upcat"] == 1
