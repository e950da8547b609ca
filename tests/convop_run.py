"""What the GPU tests of the convolution families share (test_gpu_stemconv.py, test_gpu_conv3x3.py, test_gpu_conv1x1.py; test_gpu_gshead.py, whose
reference and inputs are gshead_ref.py's, takes check and two_runs): the rounding unit and g(n), seeded inputs, the fp64 reference with its sums
over absolute values, a per-name case cache, the run on the GPU, the printed record with its assertions, and the bodies of the three tests every
family has.  A family's file keeps what is its own: the case table with the reason for each shape, the bound formula, the inputs, its own tests.

A case is a dict: dims, x, w, b, dy (fp32 CPU tensors; dy fp16 where the family says so), conv (the keywords that state the op to ref64: stride,
padding, relu), ref (ref64's result) and bounds (one tensor per key of KEYS).  An op is a callable (x, w, b) -> y on GPU tensors."""
import functools
import itertools
import json
import zlib

import torch
import torch.nn.functional as F

U = 2.0 ** -24
KEYS = ("y", "dx", "dw", "db")


def gamma(n):
    return n * U / (1.0 - n * U)


def ratio(t, t64, bound):
    """The worst error / bound; an error of zero is inside any bound (also a bound of zero), an error above a zero bound is infinite."""
    d = (t.detach().double().cpu() - t64).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / bound.clamp_min(1e-300))
    return float(r.max())


def seeded(name, salt=0):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) + salt)


def ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def group_size(rows, cap):
    """The group size G of a weight gradient's reduction, read off its *_scratch_bytes: rows(t) is the number of partial and group sums the scratch
    of t tiles holds, t + ceil(t / G) up to the cap on the partial sums, so the first t whose scratch holds two group sums is G + 1."""
    for t in range(1, cap + 1):
        extra = rows(t) - t
        assert extra in (1, 2)
        if extra == 2:
            return t - 1
    raise AssertionError("no group boundary below the cap on the partial sums")


def ref64(x, w, b, dy, stride=1, padding=0, relu=False):
    """The fp64 convolution (+ ReLU) with its gradients, the pre-activation z, and the same sums over absolute values (what the bounds are made of):
    the absolute run takes |dy| masked by the REFERENCE's mask."""
    out = {}
    x64, w64, b64 = (t.double().cpu().requires_grad_(True) for t in (x, w, b))
    z = F.conv2d(x64, w64, b64, stride=stride, padding=padding)
    y = torch.relu(z) if relu else z
    mask = (z.detach() > 0).double() if relu else torch.ones_like(z.detach())
    y.backward(dy.double().cpu())
    out.update(z=z.detach(), y=y.detach(), dx=x64.grad, dw=w64.grad, db=b64.grad)
    xa, wa, ba = (t.double().cpu().abs().requires_grad_(True) for t in (x, w, b))
    za = F.conv2d(xa, wa, ba, stride=stride, padding=padding)
    za.backward(dy.double().cpu().abs() * mask)
    out.update(abs_y=za.detach(), abs_dx=xa.grad, abs_dw=wa.grad, abs_db=ba.grad)
    return out


def case_cache(table, inputs, bounds):
    """-> case(name, *variant): the case `name` of table() -- inputs(gen, *dims, *variant) -> dict(x, w, b, dy, conv) from a generator seeded with
    the name (and the variant), the fp64 reference, bounds(ref, *dims, *variant) -- computed once per process, shared by every test that needs it,
    never modified."""
    @functools.lru_cache(maxsize=None)
    def case(name, *variant):
        dims = table()[name]
        c = dict(dims=dims, **inputs(seeded(name, sum(int(v) for v in variant)), *dims, *variant))
        c["ref"] = ref64(c["x"], c["w"], c["b"], c["dy"], **c["conv"])
        c["bounds"] = bounds(c["ref"], *dims, *variant)
        return c
    return case


def run(op, tensors, dy, backward=True):
    """op(x, w, b) on the GPU -> y, dx, dw, db (as computed, dtypes included); backward=False: y alone."""
    xg, wg, bg = (t.cuda().requires_grad_(backward) for t in tensors)
    y = op(xg, wg, bg)
    if backward:
        y.backward(dy.cuda().to(y.dtype))
    torch.cuda.synchronize()
    return dict(y=y.detach(), dx=xg.grad, dw=wg.grad, db=bg.grad)


def run_case(op, c, backward=True):
    return run(op, (c["x"], c["w"], c["b"]), c["dy"], backward)


def emit(rec):
    print(json.dumps(rec))


def check(rec, into, got, ref, bounds, keys=KEYS, dtype=torch.float32, ratio=ratio, more=None, emit=emit):
    """Emits the record -- the fields of `rec`, the worst error / bound per key under `into`, then `more` -- and asserts per key: the reference's
    shape, `dtype` (None: any), finite, error / bound <= 1.  Tensors or NumPy arrays, with the `ratio` that goes with them.  -> the record"""
    rec = dict(rec, **{into: {}})
    for k in keys:
        assert got[k].shape == ref[k].shape and dtype in (None, torch.as_tensor(got[k]).dtype), k
        rec[into][k] = ratio(got[k], ref[k], bounds[k])
    rec.update(more or {})
    emit(rec)
    for k in keys:
        assert torch.isfinite(torch.as_tensor(got[k])).all(), k
        assert rec[into][k] <= 1.0, "%s %s %s: error / bound = %.3f" % (rec.get("who", into), rec.get("case"), k, rec[into][k])
    return rec


def rel_err(t, t64):
    return float((t.detach().double().cpu() - t64).abs().max() / t64.abs().max().clamp_min(1e-300))


def passthrough_pair(calls, name):
    """-> both(a, b, inp, **autocast): the plain layer a and the converted layer b give the same tensor (dtype, shape, strides, bits) for inp,
    and b counted one pass-through and no fused call."""
    def both(a, b, inp, **ac):
        n0, p0 = calls[name], calls[name + "_passthrough"]
        with torch.autocast("cuda", enabled=bool(ac), **ac):
            ya, yb = a(inp), b(inp)
        assert calls[name] == n0 and calls[name + "_passthrough"] == p0 + 1
        assert ya.dtype == yb.dtype and ya.shape == yb.shape and ya.stride() == yb.stride() and torch.equal(ya, yb)
    return both


def _same(a, b):
    return torch.equal(torch.as_tensor(a), torch.as_tensor(b))


def two_runs(run_one, cases, keys=KEYS):
    """Two runs of each (name, case) give the same bits."""
    for name, c in cases:
        a, b = run_one(c), run_one(c)
        for k in keys:
            assert _same(a[k], b[k]), (name, k)


def exact_integers(name, op, shapes, **conv):
    """x in [-3, 3], w, b, dy in [-2, 2] of the four `shapes`, seeded with `name`: every product and partial sum is an integer far below 2^24, so
    y, dx, dw, db must EQUAL the fp64 result.  -> (got, ref)"""
    gen = seeded(name)
    x, w, b, dy = (ints(s, -r, r, gen) for s, r in zip(shapes, (3, 2, 2, 2)))
    ref = ref64(x, w, b, dy, **conv)
    got = run(op, (x, w, b), dy)
    for k in KEYS:
        assert torch.equal(got[k].double().cpu(), ref[k]), k
    return got, ref


def requires_grad_matrix(monkeypatch, module, backward, op, c, double_weight=True):
    """Every subset of (x, w, b) requiring a gradient: exactly those gradients come back, with the bits of the run that asked for all three, and
    the kernel was asked for exactly what is needed -- dx only where x wants it, dw, db and their scratch (written both or neither) only where a
    parameter does, no backward call at all where nothing does.  `backward` is the entry point `module` reaches through its `call`."""
    full = run_case(op, c)
    seen = []
    real = module.call

    def spy(name, dev, *args):
        if name == backward:
            seen.append(tuple(a is not None for a in args[-4:]))       # dx, dw, dbias, scratch
        return real(name, dev, *args)

    monkeypatch.setattr(module, "call", spy)
    x, w, b, dy = (c[k].cuda() for k in ("x", "w", "b", "dy"))
    for needs in itertools.product((True, False), repeat=3):
        leaves = [t.clone().requires_grad_(r) for t, r in zip((x, w, b), needs)]
        n = len(seen)
        y = op(*leaves)
        assert torch.equal(y.detach(), full["y"]), needs
        if any(needs):
            y.backward(dy)
            assert seen[n:] == [(needs[0],) + (needs[1] or needs[2],) * 3], needs
        else:
            assert y.grad_fn is None and seen[n:] == []
        for leaf, r, k in zip(leaves, needs, ("dx", "dw", "db")):
            assert (leaf.grad is not None) == r and (not r or torch.equal(leaf.grad, full[k])), (needs, k)
    with torch.no_grad():                                              # parameters that require grad, no graph
        y0 = op(x, w.clone().requires_grad_(True), b.clone().requires_grad_(True))
    assert y0.grad_fn is None and torch.equal(y0, full["y"])
    if double_weight:                                                  # gradients in the parameters' dtypes and shapes
        wd = w.double().requires_grad_(True)
        op(x, wd, b).backward(dy)
        assert wd.grad.dtype == torch.float64 and wd.grad.shape == w.shape and torch.equal(wd.grad.float(), full["dw"])
