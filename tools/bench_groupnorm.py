#!/usr/bin/env python
"""Per-shape timing of GroupNorm: the ATen path (nn.GroupNorm) against this package's chip-wide kernels (groupnorm.FusedGroupNorm), in ONE process.

Shapes: the GroupNorm layers a 1024^2 stereo pair meets in the feature extractor and the refinement network configured by config/stage2.yaml (the
table below is settings; nothing of the reference is read), at N = 2 and N = 8, in fp32 and with an fp16 input under fp16 autocast (where the
ATen path pays a cast kernel the fused op does not).  For each: forward alone (no_grad) and forward + backward, hipEvent brackets on random data,
the two paths ALTERNATING call by call after a warm-up of both; median and quartiles over --iters calls.  Every timed call is enqueued behind a
matrix product of about a millisecond, so the host has finished enqueueing before the first event fires: the bracket holds the GPU time of the
call's kernels and the gaps between them -- what a GPU-bound network iteration pays -- not the Python time of either path.

Prints one JSON line (all numbers) and a markdown table (profiles/groupnorm_shapes.md is that table).  Needs a GPU: there is no fallback.

    timeout 600 python tools/bench_groupnorm.py [--iters 30] [--warmup 5] [--batches 2,8]

--epilogue times the layer TOGETHER with what follows it in the reference's extractor, in its two forms -- relu_(norm(x)) and
relu(res + relu_(norm(x))) -- on three paths, alternating call by call: ATen eager; FusedGroupNorm followed by ATen's relu_ (+ add + relu), which is
what the `groupnorm` conversion alone runs; and the fused epilogue (FusedGroupNorm.forward_relu: one node, no elementwise kernel).  Same shapes,
spin-ahead and quartiles.  The table (profiles/groupnorm_epilogue.md) also goes to --md FILE; the process exits 1 if on any row the fused median
is above the median of FusedGroupNorm + ATen's elementwise ops.

    timeout 900 python tools/bench_groupnorm.py --epilogue [--md FILE]
"""
import argparse
import copy
import json
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (C, H, W, G) at 1024^2 input
SHAPES = [(32, 512, 512, 8), (32, 512, 512, 4), (48, 256, 256, 6), (96, 128, 128, 12), (64, 256, 256, 8), (48, 512, 512, 6)]


def _quartiles(v):
    v = sorted(v)
    q = lambda f: v[min(len(v) - 1, int(round(f * (len(v) - 1))))]
    return dict(median=q(0.5), q1=q(0.25), q3=q(0.75))


COPY_TBS = 6.29   # a device-to-device copy on this card, TB/s of bytes read + written (profiles/groupnorm_shapes.md)


def epilogue(args):
    import torch
    from torch import nn

    import gps_gaussian_amd  # noqa: F401
    from gps_gaussian_amd import accelerate, groupnorm

    assert torch.cuda.is_available(), "bench_groupnorm.py needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    blk = torch.randn(4096, 4096, device=dev)
    blk_out = torch.empty_like(blk)
    rows = []
    for N in [int(b) for b in args.batches.split(",")]:
        for Cn, H, W, G in SHAPES:
            for half in (False, True):
                aten = nn.GroupNorm(G, Cn).to(dev)
                with torch.no_grad():
                    aten.weight.normal_()
                    aten.bias.normal_()
                fused = copy.deepcopy(aten)
                groupnorm.convert(fused)
                x = torch.randn(N, Cn, H, W, device=dev)
                if half:
                    x = x.half()
                dy = torch.randn(N, Cn, H, W, device=dev)
                xg = x.clone().requires_grad_(True)
                res = torch.randn(N, Cn, H, W, device=dev)
                resg = res.clone().requires_grad_(True)

                def op(tag, xin, r):
                    if tag == "fused":
                        return fused.forward_relu(xin, r)
                    y = torch.relu_((aten if tag == "aten" else fused)(xin))
                    return y if r is None else torch.relu(r + y)

                def fwd(tag, residual):
                    with torch.no_grad(), torch.autocast("cuda", torch.float16, enabled=half):
                        return op(tag, x, res if residual else None)

                def fwdbwd(tag, residual):
                    xg.grad = resg.grad = None
                    m = aten if tag == "aten" else fused
                    m.weight.grad = m.bias.grad = None
                    with torch.autocast("cuda", torch.float16, enabled=half):
                        y = op(tag, xg, resg if residual else None)
                    y.backward(dy)

                for residual in (False, True):
                    rec = dict(N=N, C=Cn, H=H, W=W, G=G, x_dtype="fp16 (autocast)" if half else "fp32", form="relu_add_relu" if residual else "relu")
                    for mode, fn in (("fwd", fwd), ("fwd_bwd", fwdbwd)):
                        before = accelerate.calls["groupnorm"]
                        times = {"aten": [], "parent": [], "fused": []}
                        for it in range(args.warmup + args.iters):
                            for tag in times:
                                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                                torch.mm(blk, blk, out=blk_out)   # keeps the GPU busy while the host enqueues what follows
                                e0.record()
                                fn(tag, residual)
                                e1.record()
                                e1.synchronize()
                                if it >= args.warmup:
                                    times[tag].append(e0.elapsed_time(e1) * 1e3)   # microseconds
                        assert accelerate.calls["groupnorm"] - before == 2 * (args.warmup + args.iters)   # both converted paths ran the kernels
                        q = {tag: _quartiles(v) for tag, v in times.items()}
                        rec[mode] = dict(aten_us=q["aten"], parent_us=q["parent"], fused_us=q["fused"],
                                         vs_aten=q["aten"]["median"] / q["fused"]["median"], vs_parent=q["parent"]["median"] / q["fused"]["median"])
                    rows.append(rec)
                del x, dy, xg, res, resg, aten, fused
                torch.cuda.empty_cache()

    print(json.dumps(dict(tool="bench_groupnorm --epilogue", device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, rows=rows)))
    cell = lambda d: "%.0f (%.0f–%.0f)" % (d["median"], d["q1"], d["q3"])
    md = ["| shape | G | x | form | fwd ATen µs (q1–q3) | fwd GN + ATen relu/add µs | fwd fused µs | × ATen | × GN + ATen | fwd+bwd ATen µs | fwd+bwd GN + ATen relu/add µs "
          "| fwd+bwd fused µs | × ATen | × GN + ATen |", "|" + "---|" * 14]
    losing = []
    for r in rows:
        f, b = r["fwd"], r["fwd_bwd"]
        md.append("| [%d,%d,%d,%d] | %d | %s | %s | %s | %s | %s | %.2f | %.2f | %s | %s | %s | %.2f | %.2f |" % (
            r["N"], r["C"], r["H"], r["W"], r["G"], r["x_dtype"], r["form"], cell(f["aten_us"]), cell(f["parent_us"]), cell(f["fused_us"]), f["vs_aten"],
            f["vs_parent"], cell(b["aten_us"]), cell(b["parent_us"]), cell(b["fused_us"]), b["vs_aten"], b["vs_parent"]))
        for mode in ("fwd", "fwd_bwd"):
            if r[mode]["fused_us"]["median"] > r[mode]["parent_us"]["median"]:
                losing.append("[%d,%d,%d,%d] G=%d %s %s %s" % (r["N"], r["C"], r["H"], r["W"], r["G"], r["x_dtype"], r["form"], mode))
    for r in rows:   # the residual forward of the largest fp32 activation: x twice, the residual once, the output once
        if (r["N"], r["C"], r["H"], r["G"], r["x_dtype"], r["form"]) == (2, 32, 512, 8, "fp32", "relu_add_relu"):
            nbytes = 4 * 4 * r["N"] * r["C"] * r["H"] * r["W"]
            us = r["fwd"]["fused_us"]["median"]
            md += ["", "[2,32,512,512] G=8 fp32 residual forward: 4 passes = %.1f MB in %.0f µs = %.2f TB/s, %.0f %% of the %.2f TB/s of a copy." % (
                nbytes / 1e6, us, nbytes / us / 1e6, 100.0 * nbytes / us / 1e6 / COPY_TBS, COPY_TBS)]
    md += ["", "Rows on which the fused median is above GN + ATen relu/add: %s" % (", ".join(losing) if losing else "none")]
    print()
    print("\n".join(md))
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(md) + "\n")
    return 1 if losing else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", default="2,8")
    ap.add_argument("--timeout", type=int, default=900, help="the process ends itself after this many seconds")
    ap.add_argument("--epilogue", action="store_true", help="time norm + ReLU and norm + ReLU + residual add + ReLU on three paths (see above)")
    ap.add_argument("--md", default=None, help="--epilogue: also write the markdown table to this file")
    args = ap.parse_args()
    signal.alarm(args.timeout)
    if args.epilogue:
        sys.exit(epilogue(args))

    import torch
    from torch import nn

    import gps_gaussian_amd  # noqa: F401
    from gps_gaussian_amd import accelerate, groupnorm

    assert torch.cuda.is_available(), "bench_groupnorm.py needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    blk = torch.randn(4096, 4096, device=dev)
    blk_out = torch.empty_like(blk)
    rows = []
    for N in [int(b) for b in args.batches.split(",")]:
        for Cn, H, W, G in SHAPES:
            for half in (False, True):
                aten = nn.GroupNorm(G, Cn).to(dev)
                with torch.no_grad():
                    aten.weight.normal_()
                    aten.bias.normal_()
                fused = copy.deepcopy(aten)
                groupnorm.convert(fused)
                x = torch.randn(N, Cn, H, W, device=dev)
                if half:
                    x = x.half()
                dy = torch.randn(N, Cn, H, W, device=dev)
                xg = x.clone().requires_grad_(True)

                def fwd(m):
                    with torch.no_grad(), torch.autocast("cuda", torch.float16, enabled=half):
                        return m(x)

                def fwdbwd(m):
                    xg.grad = None
                    m.weight.grad = m.bias.grad = None
                    with torch.autocast("cuda", torch.float16, enabled=half):
                        y = m(xg)
                    y.backward(dy)

                rec = dict(N=N, C=Cn, H=H, W=W, G=G, x_dtype="fp16 (autocast)" if half else "fp32")
                for mode, fn in (("fwd", fwd), ("fwd_bwd", fwdbwd)):
                    before = accelerate.calls["groupnorm"]
                    times = {"aten": [], "fused": []}
                    for it in range(args.warmup + args.iters):
                        for tag, m in (("aten", aten), ("fused", fused)):
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            torch.mm(blk, blk, out=blk_out)   # keeps the GPU busy while the host enqueues what follows
                            e0.record()
                            fn(m)
                            e1.record()
                            e1.synchronize()
                            if it >= args.warmup:
                                times[tag].append(e0.elapsed_time(e1) * 1e3)   # microseconds
                    assert accelerate.calls["groupnorm"] - before == args.warmup + args.iters   # the fused path really ran the kernels
                    a, f = _quartiles(times["aten"]), _quartiles(times["fused"])
                    rec[mode] = dict(aten_us=a, fused_us=f, ratio=a["median"] / f["median"])
                rows.append(rec)
                del x, dy, xg, aten, fused
                torch.cuda.empty_cache()

    print(json.dumps(dict(tool="bench_groupnorm", device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, rows=rows)))
    print()
    print("| shape | G | x | fwd ATen µs (q1–q3) | fwd fused µs (q1–q3) | × | fwd+bwd ATen µs (q1–q3) | fwd+bwd fused µs (q1–q3) | × |")
    print("|---|---|---|---|---|---|---|---|---|")
    cell = lambda d: "%.0f (%.0f–%.0f)" % (d["median"], d["q1"], d["q3"])
    for r in rows:
        print("| [%d,%d,%d,%d] | %d | %s | %s | %s | %.2f | %s | %s | %.2f |" % (
            r["N"], r["C"], r["H"], r["W"], r["G"], r["x_dtype"], cell(r["fwd"]["aten_us"]), cell(r["fwd"]["fused_us"]), r["fwd"]["ratio"],
            cell(r["fwd_bwd"]["aten_us"]), cell(r["fwd_bwd"]["fused_us"]), r["fwd_bwd"]["ratio"]))


if __name__ == "__main__":
    main()
