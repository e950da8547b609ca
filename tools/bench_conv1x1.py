#!/usr/bin/env python
"""Per-layer timing of the 1x1 convolutions that open the residual shortcuts (core/extractor.py:43-45, `downsample[0]`) -- ATen's own convolution
against conv1x1.conv1x1 (the fp32 matrix-core kernels of csrc/conv1x1.hip).

Layers: the five fp32 instances with config/stage2.yaml's widths and a 1024^2 stereo pair -- UnetExtractor.res2[0] / res3[0] (stride 2) and the first
block of GSRegresser.decoder3 / decoder2 / decoder1 (stride 1) -- plus res1[0] of the default widths, Conv2d(32, 64, 1) at 512^2, each at N = 2
(one stereo pair) and N = 8 (training, batch 4).  For each: forward alone (no_grad) and forward + backward with all three gradients.  hipEvent
brackets on random data after a warm-up; median and quartiles over --iters calls.  Every timed call is enqueued behind a matrix product of about a
millisecond, so the host has finished enqueueing before the first event fires (the timing method of tools/bench_stemconv.py).

This process itself never touches the GPU.  It starts three children, one after the other, each under its own time limit, and starts nothing more
once one has failed:
  * `fused`: the fused op, all layers in one process -- the autograd op (what a module call costs), and each kernel on its own through the C-ABI
    (forward, input gradient, weight gradient + reduction) with its algorithmic bytes -- every needed element read once, every result written once
    -- and the GB/s they make; the yardstick is gshead's forward, the same access pattern, at 3.4-3.8 TB/s (profiles/gshead_shapes.md);
  * `aten`, MIOPEN_FIND_MODE unset, and `aten`, MIOPEN_FIND_MODE=FAST (what the profiled runs of profiles/r04_* used): ATen's conv2d, the same
    passes, and the names of the GPU kernels one forward call launched (torch.profiler): whether `batched_transpose` is among them and which
    implicit-GEMM tile.
The verdict on the two implicit-GEMM rows of profiles/r04_config3_kernel_stats.md that no earlier layer kind turned out to be (`...bt128x32x32`,
651.6 us per call, 3 calls per view; `...bt256x32x4`, 1724.6 us, 2 calls per view): a row is attributed to these layers -- confirmed -- where, at
N = 2 under FAST, a layer's forward is within 2x of the row's time (the rule of profiles/stemconv_shapes.md) AND an implicit-GEMM kernel with the
row's tile is among that call's kernels; refuted otherwise.

Prints one JSON line (all numbers) and a markdown table (also to --md FILE); lists the (layer, pass) rows on which the fused median is above ATen's
under either find mode.  NOT measured here: a training iteration or the pipeline with GPSGS_ACCELERATE=conv1x1 set.  Needs a GPU: no fallback.

    timeout 1100 python tools/bench_conv1x1.py [--iters 10] [--warmup 3] [--md profiles/conv1x1_shapes.md]
"""
import argparse
import json
import os
import signal
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (layer, C_in, C_out, H, W, stride)
SHAPES = [("res2[0]", 32, 48, 512, 512, 2), ("res3[0]", 48, 96, 256, 256, 2), ("decoder3[0]", 192, 96, 128, 128, 1),
          ("decoder2[0]", 192, 64, 256, 256, 1), ("decoder1[0]", 128, 48, 512, 512, 1), ("res1[0] (default widths)", 32, 64, 512, 512, 1)]
LAYERS = [(name, N, Ci, Co, H, W, s) for N in (2, 8) for name, Ci, Co, H, W, s in SHAPES]
PROFILE_ROWS = [("bt128x32x32", 651.6, 3), ("bt256x32x4", 1724.6, 2)]   # profiles/r04_config3_kernel_stats.md: tile, us per call, calls per view


def _quartiles(v):
    v = sorted(v)
    q = lambda f: v[min(len(v) - 1, int(round(f * (len(v) - 1))))]
    return dict(median=q(0.5), q1=q(0.25), q3=q(0.75))


def child(args):
    signal.alarm(args.timeout)
    import torch
    import torch.nn.functional as F

    import gps_gaussian_amd  # noqa: F401
    from gps_gaussian_amd import _capi, _ops, conv1x1

    assert torch.cuda.is_available(), "bench_conv1x1.py needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    blk = torch.randn(4096, 4096, device=dev)
    blk_out = torch.empty_like(blk)

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
    for name, N, Ci, Co, H, W, s in LAYERS:
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        x = torch.randn(N, Ci, H, W, device=dev).requires_grad_(True)
        w = (torch.randn(Co, Ci, 1, 1, device=dev) * 0.1).requires_grad_(True)
        b = torch.randn(Co, device=dev).requires_grad_(True)
        dy = torch.randn(N, Co, Ho, Wo, device=dev)
        rec = dict(layer=name, N=N, C_in=Ci, C_out=Co, H=H, W=W, stride=s)
        if args.child == "fused":
            op = lambda: conv1x1.conv1x1(x, w, b, s)
        else:
            op = lambda: F.conv2d(x, w, b, stride=s)

        def fwd():
            with torch.no_grad():
                return op()

        def fwd_bwd():
            return torch.autograd.grad(op(), (x, w, b), dy)

        rec["fwd"] = timed(fwd)
        rec["fwd_bwd"] = timed(fwd_bwd)
        if args.child == "fused":   # each kernel on its own, on preallocated tensors
            lib = _capi.lib()
            xd, wd, bd = x.detach(), w.detach(), b.detach()
            y, dx, dw, db = torch.empty_like(dy), torch.empty_like(xd), torch.empty_like(wd), torch.empty_like(bd)
            scratch = torch.empty(lib.c1_scratch_bytes(N, Ci, Co, H, W, s) // 4 + 4, device=dev)
            p = _ops.ptr
            rec["k_fwd"] = timed(lambda: _ops.call("c1_forward", dev, p(xd), p(wd), p(bd), N, Ci, Co, H, W, s, p(y)))
            rec["k_bwd_input"] = timed(lambda: _ops.call("c1_backward", dev, p(xd), p(wd), p(dy), N, Ci, Co, H, W, s, p(dx), None, None, None))
            rec["k_bwd_weight"] = timed(lambda: _ops.call("c1_backward", dev, p(xd), p(wd), p(dy), N, Ci, Co, H, W, s, None, p(dw), p(db), p(scratch)))
            del y, dx, dw, db, scratch
        else:                       # the GPU kernels of one forward call, by name
            try:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    fwd()
                    torch.cuda.synchronize()
                dev_us = lambda e: float(getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0)))
                ev = sorted((e for e in prof.key_averages() if dev_us(e) > 0), key=lambda e: -dev_us(e))   # kernels only, longest first
                rec["kernels"] = [[e.key[:120], dev_us(e), int(e.count)] for e in ev[:6]]
            except Exception as e:   # the profiler is a convenience: the timings stand without it
                rec["kernels"] = [["(profiler unavailable: %s)" % type(e).__name__, 0.0, 0]]
        rows.append(rec)
        del x, w, b, dy
        torch.cuda.empty_cache()
    print(json.dumps(dict(child=args.child, find_mode=os.environ.get("MIOPEN_FIND_MODE", "default"), device=torch.cuda.get_device_name(0), rows=rows)))
    return 0


def _bytes(r):
    """The algorithmic traffic of the three kernels: each needed element read once, each result written once (the weights are noise)."""
    P = r["N"] * ((r["H"] - 1) // r["stride"] + 1) * ((r["W"] - 1) // r["stride"] + 1)
    full = r["N"] * r["H"] * r["W"]
    return dict(k_fwd=4.0 * P * (r["C_in"] + r["C_out"]),                  # the sampled x, y
                k_bwd_input=4.0 * (P * r["C_out"] + full * r["C_in"]),     # dy, ALL of dx
                k_bwd_weight=4.0 * P * (r["C_in"] + r["C_out"]))           # the sampled x, dy


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
    for tag, kind, mode in (("fused", "fused", None), ("default", "aten", None), ("FAST", "aten", "FAST")):
        env = dict(os.environ)
        env.pop("MIOPEN_FIND_MODE", None)
        if mode:
            env["MIOPEN_FIND_MODE"] = mode
        cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--iters", str(args.iters), "--warmup", str(args.warmup),
               "--timeout", str(args.timeout)]
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=args.timeout + 30)
        if r.returncode != 0:      # a child that failed: nothing more is started on the GPU
            print(r.stdout[-4000:])
            return r.returncode or 1
        res[tag] = json.loads(r.stdout.strip().splitlines()[-1])
        print("[bench_conv1x1] %s: done" % tag, file=sys.stderr, flush=True)
    print(json.dumps(dict(tool="bench_conv1x1", iters=args.iters, warmup=args.warmup, runs=res)))

    cell = lambda d: "%.0f (%.0f–%.0f)" % (d["median"], d["q1"], d["q3"])
    shape = lambda r: "[%d,%d,%d,%d] → %d, stride %d" % (r["N"], r["C_in"], r["H"], r["W"], r["C_out"], r["stride"])
    md = ["| layer | x → C_out | pass | ATen µs, default find (q1–q3) | ATen µs, FAST (q1–q3) | fused µs (q1–q3) | × default | × FAST |", "|" + "---|" * 8]
    losing = []
    for rf, rd, ra in zip(res["fused"]["rows"], res["default"]["rows"], res["FAST"]["rows"]):
        for mode in ("fwd", "fwd_bwd"):
            f, a, af = rf[mode], rd[mode], ra[mode]
            md.append("| %s | %s | %s | %s | %s | %s | %.2f | %.2f |" % (
                rf["layer"], shape(rf), "fwd" if mode == "fwd" else "fwd+bwd", cell(a), cell(af), cell(f), a["median"] / f["median"],
                af["median"] / f["median"]))
            if f["median"] > min(a["median"], af["median"]):
                losing.append("%s %s %s" % (rf["layer"], shape(rf), mode))
    md += ["", "fp32, the autograd op on both sides (allocations included).", "",
           "The fused kernels on their own (C-ABI calls on preallocated tensors).  MB: the algorithmic traffic -- the sampled x and y for the forward, dy and "
           "ALL of dx for the input gradient, the sampled x and dy for the weight gradient (which also writes and re-reads its partial sums: not counted).  "
           "For stride 2 half of every fetched sector of x is not needed and half of dx is zeros.  Yardstick: gshead's forward, the same access "
           "pattern, 3.4–3.8 TB/s.", "",
           "| x → C_out | k_c1_fwd µs | MB | GB/s | k_c1_bwd_input µs | MB | GB/s | k_c1_bwd_weight + reduce µs | MB | GB/s |", "|" + "---|" * 10]
    for rf in res["fused"]["rows"]:
        cells, by = [], _bytes(rf)
        for k in ("k_fwd", "k_bwd_input", "k_bwd_weight"):
            cells += [cell(rf[k]), "%.0f" % (by[k] / 1e6), "%.0f" % (by[k] / (rf[k]["median"] * 1e-6) / 1e9)]
        md.append("| %s | %s |" % (shape(rf), " | ".join(cells)))
    for tag, title in (("FAST", "MIOPEN_FIND_MODE=FAST"), ("default", "the default find mode")):
        md += ["", "ATen's GPU kernels of one forward call (torch.profiler: name, µs in that call, launches), %s:" % title, ""]
        for ra in res[tag]["rows"]:
            names = [k[0] for k in ra["kernels"]]
            md.append("- %s: %s -- `batched_transpose`: %s; implicit-GEMM kernel: %s" % (
                shape(ra), "; ".join("`%s` %.0f µs ×%d" % tuple(k) for k in ra["kernels"]),
                "yes, %d launches" % sum(k[2] for k in ra["kernels"] if "batched_transpose" in k[0]) if any("batched_transpose" in n for n in names) else "no",
                ", ".join("`%s`" % n for n in names if "igemm" in n) or "none"))
    md.append("")
    n2 = [(ra, rd) for ra, rd in zip(res["FAST"]["rows"], res["default"]["rows"]) if ra["N"] == 2]
    for tile, us, per_view in PROFILE_ROWS:
        named = [ra for ra, rd in n2 if any("igemm" in k[0] and tile in k[0] for k in ra["kernels"] + rd["kernels"])]
        held = [ra for ra in named if 0.5 * us <= ra["fwd"]["median"] <= 2.0 * us]
        times = ", ".join("%s %.0f µs" % (ra["layer"], ra["fwd"]["median"]) for ra, rd in n2)
        md.append("Attribution check, the profile's `igemm_fwd_gtcx35_nhwc_fp32_…_%s` row (%.1f µs per call, %d calls per view): ATen's forwards at N = 2 "
                  "under FAST take %s.  An implicit-GEMM kernel with that tile appears in the call of: %s; of those, within 2× of the row's time: %s.  The "
                  "attribution of that row to the shortcut convolutions is **%s**."
                  % (tile, us, per_view, times, ", ".join(ra["layer"] for ra in named) or "no layer", ", ".join(ra["layer"] for ra in held) or "none",
                     "confirmed for " + ", ".join(ra["layer"] for ra in held) if held else "refuted: that row is some other convolution"))
    md += ["", "Not measured here: a training iteration or the pipeline with GPSGS_ACCELERATE=conv1x1 set.", "",
           "Rows on which the fused median is above ATen's (either find mode): %s" % (", ".join(losing) if losing else "none")]
    print()
    print("\n".join(md))
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(md) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
