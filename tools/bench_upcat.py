#!/usr/bin/env python
"""Per-site timing of the regresser's decoder glue (lib/gs_parm_network.py:56-67) -- ATen's nn.Upsample(scale_factor=2, mode="bilinear") and the
reference's two-stage torch.cat against upcat.upsample2x_cat (the streaming kernels of csrc/upcat.hip).

Sites: the three of GSRegresser.forward with config/stage2.yaml's widths and a 1024^2 stereo pair -- S3 [N,96,128,128] + 2 x 48 channels, S2
[N,64,256,256] + 2 x 32, S1 [N,48,512,512] + the image (3) and the depth (1) -- each at N = 2 (one stereo pair) and N = 8 (training, batch 4).  For
each: forward alone (no_grad) and forward + backward with the gradients of all inputs.  hipEvent brackets on random data after a warm-up; median and
quartiles over --iters calls.  Every timed call is enqueued behind a matrix product of about a millisecond, so the host has finished enqueueing
before the first event fires (the timing method of tools/bench_conv1x1.py).

This process itself never touches the GPU.  It starts two children, one after the other, each under its own time limit, and starts nothing more
once one has failed:
  * `fused`: the autograd op (what a call from regresser_forward costs, allocations included), and each kernel on its own through the C-ABI on
    preallocated tensors with its algorithmic bytes -- one read of every input and one write of out for the forward, one read of dout[:, :Ca] and
    one write of da for the backward -- and the GB/s they make; the yardstick is gshead's forward at 3.4-3.8 TB/s (profiles/gshead_shapes.md);
  * `aten`: up(a), then torch.cat([up, torch.cat([s0, s1])]) as the reference orders them (S1: one torch.cat of three), the same passes, and the
    names of the GPU kernels one forward + backward call launched (torch.profiler), so that the atomics-based backward is named.

Prints one JSON line (all numbers) and a markdown table (also to --md FILE); lists the (site, pass) rows on which the fused median is above ATen's.
NOT measured here: a training iteration or the pipeline with the regresser converted.  Needs a GPU: no fallback.

    timeout 900 python tools/bench_upcat.py [--iters 10] [--warmup 3] [--md profiles/upcat_shapes.md]
"""
import argparse
import json
import os
import signal
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (site, Ca, h, w, skip channels, the reference concatenates the skips first)
SHAPES = [("S3", 96, 128, 128, (48, 48), True), ("S2", 64, 256, 256, (32, 32), True), ("S1", 48, 512, 512, (3, 1), False)]
SITES = [(name, N, Ca, h, w, sk, two) for N in (2, 8) for name, Ca, h, w, sk, two in SHAPES]


def _quartiles(v):
    v = sorted(v)
    q = lambda f: v[min(len(v) - 1, int(round(f * (len(v) - 1))))]
    return dict(median=q(0.5), q1=q(0.25), q3=q(0.75))


def child(args):
    signal.alarm(args.timeout)
    import ctypes

    import torch
    from torch import nn

    import gps_gaussian_amd  # noqa: F401
    from gps_gaussian_amd import _ops, upcat

    assert torch.cuda.is_available(), "bench_upcat.py needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    blk = torch.randn(4096, 4096, device=dev)
    blk_out = torch.empty_like(blk)
    up = nn.Upsample(scale_factor=2, mode="bilinear")

    def timed(fn):
        times = []
        for it in range(args.warmup + args.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.mm(blk, blk, out=blk_out)   # keeps the GPU busy while the host enqueues what follows
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= args.warmup:
                times.append(e0.elapsed_time(e1) * 1e3)
        return _quartiles(times)

    rows = []
    for name, N, Ca, h, w, sk, two in SITES:
        a = torch.randn(N, Ca, h, w, device=dev).requires_grad_(True)
        skips = [torch.randn(N, c, 2 * h, 2 * w, device=dev).requires_grad_(True) for c in sk]
        dout = torch.randn(N, Ca + sum(sk), 2 * h, 2 * w, device=dev)
        rec = dict(site=name, N=N, Ca=Ca, h=h, w=w, skips=list(sk))
        if args.child == "fused":
            op = lambda: upcat.upsample2x_cat(a, *skips)
        elif two:
            op = lambda: torch.cat([up(a), torch.cat(skips, dim=1)], dim=1)
        else:
            op = lambda: torch.cat([up(a)] + skips, dim=1)

        def fwd():
            with torch.no_grad():
                return op()

        def fwd_bwd():
            return torch.autograd.grad(op(), [a] + skips, dout)

        rec["fwd"] = timed(fwd)
        rec["fwd_bwd"] = timed(fwd_bwd)
        if args.child == "fused":   # each kernel on its own, on preallocated tensors
            p = _ops.ptr
            ad, sd = a.detach(), [s.detach() for s in skips]
            out, da = torch.empty_like(dout), torch.empty_like(ad)
            ptrs, counts = (ctypes.c_void_p * len(sd))(*[p(s) for s in sd]), (ctypes.c_int * len(sk))(*sk)
            rec["k_fwd"] = timed(lambda: _ops.call("uc_forward", dev, p(ad), ptrs, counts, len(sk), N, Ca, h, w, p(out)))
            rec["k_bwd"] = timed(lambda: _ops.call("uc_backward", dev, p(dout), counts, len(sk), N, Ca, h, w, p(da)))
            del out, da
        else:                       # the GPU kernels of one forward + backward call, by name
            try:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    fwd_bwd()
                    torch.cuda.synchronize()
                dev_us = lambda e: float(getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0)))
                ev = sorted((e for e in prof.key_averages() if dev_us(e) > 0), key=lambda e: -dev_us(e))   # kernels only, longest first
                rec["kernels"] = [[e.key[:100], dev_us(e), int(e.count)] for e in ev[:8]]
            except Exception as e:   # the profiler is a convenience: the timings stand without it
                rec["kernels"] = [["(profiler unavailable: %s)" % type(e).__name__, 0.0, 0]]
        rows.append(rec)
        del a, skips, dout
        torch.cuda.empty_cache()
    print(json.dumps(dict(child=args.child, device=torch.cuda.get_device_name(0), rows=rows)))
    return 0


def _bytes(r):
    """The algorithmic traffic of the two kernels: each input read once, each result written once."""
    up = r["N"] * r["Ca"] * r["h"] * r["w"]
    skips = r["N"] * sum(r["skips"]) * 4 * r["h"] * r["w"]
    return dict(k_fwd=4.0 * (up + skips + 4 * up + skips), k_bwd=4.0 * (4 * up + up))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300, help="each child process ends itself after this many seconds")
    ap.add_argument("--md", default=None, help="also write the markdown table to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)

    res = {}
    for kind in ("fused", "aten"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--iters", str(args.iters), "--warmup", str(args.warmup),
               "--timeout", str(args.timeout)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.timeout + 30)
        if r.returncode != 0:      # a child that failed: nothing more is started on the GPU
            print(r.stdout[-4000:])
            return r.returncode or 1
        res[kind] = json.loads(r.stdout.strip().splitlines()[-1])
        print("[bench_upcat] %s: done" % kind, file=sys.stderr, flush=True)
    print(json.dumps(dict(tool="bench_upcat", iters=args.iters, warmup=args.warmup, runs=res)))

    cell = lambda d: "%.0f (%.0f–%.0f)" % (d["median"], d["q1"], d["q3"])
    shape = lambda r: "[%d,%d,%d,%d] + %s → [%d,%d,%d,%d]" % (r["N"], r["Ca"], r["h"], r["w"], "+".join(str(c) for c in r["skips"]), r["N"],
                                                             r["Ca"] + sum(r["skips"]), 2 * r["h"], 2 * r["w"])
    md = ["| site | a + skip channels → out | pass | ATen µs (q1–q3) | fused µs (q1–q3) | × ATen |", "|" + "---|" * 6]
    losing = []
    for rf, ra in zip(res["fused"]["rows"], res["aten"]["rows"]):
        for mode in ("fwd", "fwd_bwd"):
            f, a = rf[mode], ra[mode]
            md.append("| %s | %s | %s | %s | %s | %.2f |" % (rf["site"], shape(rf), "fwd" if mode == "fwd" else "fwd+bwd", cell(a), cell(f),
                                                          a["median"] / f["median"]))
            if f["median"] > a["median"]:
                losing.append("%s N=%d %s" % (rf["site"], rf["N"], mode))
    md += ["", "fp32, the autograd op on both sides (allocations included); ATen: nn.Upsample, then the reference's two-stage concatenation (S3, S2) or "
           "its one concatenation of three (S1); gradients of a and of every skip.", "",
           "The fused kernels on their own (C-ABI calls on preallocated tensors).  MB: the algorithmic traffic -- one read of a and of every skip and one "
           "write of out for the forward; one read of dout[:, :Ca] and one write of da for the backward.  Yardstick: gshead's forward, 3.4–3.8 TB/s.", "",
           "| a + skip channels → out | k_uc_fwd µs | MB | GB/s | k_uc_bwd µs | MB | GB/s |", "|" + "---|" * 7]
    for rf in res["fused"]["rows"]:
        cells, by = [], _bytes(rf)
        for k in ("k_fwd", "k_bwd"):
            cells += [cell(rf[k]), "%.0f" % (by[k] / 1e6), "%.0f" % (by[k] / (rf[k]["median"] * 1e-6) / 1e9)]
        md.append("| %s | %s |" % (shape(rf), " | ".join(cells)))
    md += ["", "ATen's GPU kernels of one forward + backward call (torch.profiler: name, µs in that call, launches):", ""]
    for ra in res["aten"]["rows"]:
        md.append("- %s N=%d: %s" % (ra["site"], ra["N"], "; ".join("`%s` %.0f µs ×%d" % tuple(k) for k in ra["kernels"])))
    md += ["", "Not measured here: a training iteration or the pipeline with the regresser converted (upcat.convert).", "",
           "Rows on which the fused median is above ATen's: %s" % (", ".join(losing) if losing else "none")]
    print()
    print("\n".join(md))
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(md) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
