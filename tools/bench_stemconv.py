#!/usr/bin/env python
"""Per-shape timing of the stem convolution Conv2d(C_in, 32, 5, stride 2, padding 2): the ATen path (nn.Conv2d) against this package's direct
kernels (stemconv.FusedStemConv2d), in ONE process.

Shapes: what the two encoders' first layer meets -- [N, C_in, 1024, 1024] for N = 2 (one stereo pair) and N = 8 (training, batch 4), C_in = 3
(image) and 1 (depth) -- plus [2, 3, 2048, 2048]; in fp32 and under fp16 autocast (fp16 result, fp16 incoming gradient).  For each: forward alone
(no_grad) and forward + backward; the backward leaves out the input gradient for C_in = 3 (the image needs none) and includes it for C_in = 1
(the depth encoder's input does).  hipEvent brackets on random data, the two paths ALTERNATING call by call after a warm-up of both; median and
quartiles over --iters calls.  Every timed call is enqueued behind a matrix product of about a millisecond, so the host has finished enqueueing
before the first event fires: the bracket holds the GPU time of the call's kernels and the gaps between them, not the Python time of either path.

The ATen column is also the measurement that settles what the kernel-name attribution of profiles/r04_config3/4_kernel_stats.md could only infer:
whether these two layers are the 1.7 ms (inference) / 6.4 ms (training) implicit-GEMM rows.  profiles/stemconv_shapes.md says which.

Prints one JSON line (all numbers) and a markdown table (also to --md FILE) with, per row: ATen us, fused us, the ratio, and the fused op's GB/s of
algorithmic bytes (every tensor read or written once) and TFLOP/s (2 flops per multiply-add).  Exits 1 if on any row the fused median is above
ATen's.  Needs a GPU: there is no fallback.

    timeout 900 python tools/bench_stemconv.py [--iters 20] [--warmup 3] [--md profiles/stemconv_shapes.md]
"""
import argparse
import copy
import json
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(2, 3, 1024, 1024), (2, 1, 1024, 1024), (8, 3, 1024, 1024), (8, 1, 1024, 1024), (2, 3, 2048, 2048)]   # [N, C_in, H, W]
C_OUT, K, S, P = 32, 5, 2, 2
# the implicit-GEMM row (bt256x32x4, fp32) that the kernel-name attribution assigned to these two layers: microseconds per call at N = 2 (inference,
# profiles/r04_config3_kernel_stats.md) and N = 8 (training, profiles/r04_config4_kernel_stats.md)
PROFILE_ROW_US = {2: 1724.6, 8: 6395.4}


def _quartiles(v):
    v = sorted(v)
    q = lambda f: v[min(len(v) - 1, int(round(f * (len(v) - 1))))]
    return dict(median=q(0.5), q1=q(0.25), q3=q(0.75))


def _work(N, Ci, H, W, half, mode):
    """(algorithmic bytes, flops) of a row: forward reads x, w, b and writes y; the backward reads x, dy (and w) and writes dw, db (and dx)."""
    Ho, Wo = (H + 2 * P - K) // S + 1, (W + 2 * P - K) // S + 1
    x, y, w = 4 * N * Ci * H * W, (2 if half else 4) * N * C_OUT * Ho * Wo, 4 * C_OUT * (Ci * K * K + 1)
    macs = N * C_OUT * Ho * Wo * Ci * K * K
    if mode == "fwd":
        return x + w + y, 2 * macs
    nbytes, flops = (x + w + y) + (x + y + w), 2 * macs + 2 * macs        # forward + weight / bias gradient
    if Ci == 1:
        nbytes, flops = nbytes + y + w + x, flops + 2 * macs              # + input gradient
    return nbytes, flops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=900, help="the process ends itself after this many seconds")
    ap.add_argument("--md", default=None, help="also write the markdown table to this file")
    args = ap.parse_args()
    signal.alarm(args.timeout)

    import torch
    from torch import nn

    import gps_gaussian_amd  # noqa: F401
    from gps_gaussian_amd import accelerate, stemconv

    assert torch.cuda.is_available(), "bench_stemconv.py needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    blk = torch.randn(4096, 4096, device=dev)
    blk_out = torch.empty_like(blk)
    rows = []
    for N, Ci, H, W in SHAPES:
        Ho, Wo = (H + 2 * P - K) // S + 1, (W + 2 * P - K) // S + 1
        for half in (False, True):
            aten = nn.Conv2d(Ci, C_OUT, K, stride=S, padding=P).to(dev)
            fused = copy.deepcopy(aten)
            assert stemconv.convert(fused) == 1
            x = torch.randn(N, Ci, H, W, device=dev)
            xg = x.clone().requires_grad_(Ci == 1)
            dy = torch.randn(N, C_OUT, Ho, Wo, device=dev, dtype=torch.float16 if half else torch.float32)

            def fwd(m):
                with torch.no_grad(), torch.autocast("cuda", torch.float16, enabled=half):
                    return m(x)

            def fwdbwd(m):
                xg.grad = None
                m.weight.grad = m.bias.grad = None
                with torch.autocast("cuda", torch.float16, enabled=half):
                    y = m(xg)
                y.backward(dy)

            rec = dict(N=N, C_in=Ci, H=H, W=W, C_out=C_OUT, y_dtype="fp16 (autocast)" if half else "fp32", dx=Ci == 1)
            for mode, fn in (("fwd", fwd), ("fwd_bwd", fwdbwd)):
                before = accelerate.calls["stemconv"]
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
                assert accelerate.calls["stemconv"] - before == args.warmup + args.iters   # the fused path really ran the kernels
                a, f = _quartiles(times["aten"]), _quartiles(times["fused"])
                nbytes, flops = _work(N, Ci, H, W, half, mode)
                rec[mode] = dict(aten_us=a, fused_us=f, ratio=a["median"] / f["median"], fused_gbs=nbytes / f["median"] / 1e3,
                                 fused_tflops=flops / f["median"] / 1e6)
            rows.append(rec)
            del x, xg, dy, aten, fused
            torch.cuda.empty_cache()

    print(json.dumps(dict(tool="bench_stemconv", device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, rows=rows)))
    cell = lambda d: "%.0f (%.0f–%.0f)" % (d["median"], d["q1"], d["q3"])
    md = ["| x | y | fwd ATen µs (q1–q3) | fwd fused µs (q1–q3) | × | GB/s | TFLOP/s | fwd+bwd ATen µs (q1–q3) | fwd+bwd fused µs (q1–q3) | × | GB/s | TFLOP/s |",
          "|" + "---|" * 12]
    losing = []
    for r in rows:
        f, b = r["fwd"], r["fwd_bwd"]
        md.append("| [%d,%d,%d,%d] | %s | %s | %s | %.2f | %.0f | %.2f | %s | %s | %.2f | %.0f | %.2f |" % (
            r["N"], r["C_in"], r["H"], r["W"], r["y_dtype"], cell(f["aten_us"]), cell(f["fused_us"]), f["ratio"], f["fused_gbs"], f["fused_tflops"],
            cell(b["aten_us"]), cell(b["fused_us"]), b["ratio"], b["fused_gbs"], b["fused_tflops"]))
        for mode in ("fwd", "fwd_bwd"):
            if r[mode]["fused_us"]["median"] > r[mode]["aten_us"]["median"]:
                losing.append("[%d,%d,%d,%d] %s %s" % (r["N"], r["C_in"], r["H"], r["W"], r["y_dtype"], mode))
    md += [""]
    for N, row_us in sorted(PROFILE_ROW_US.items()):   # does ATen's time for these layers match the profile row they were attributed to?
        got = {r["C_in"]: r["fwd"]["aten_us"]["median"] for r in rows if r["N"] == N and r["H"] == 1024 and r["y_dtype"] == "fp32"}
        if len(got) == 2:
            held = all(0.5 * row_us <= v <= 2.0 * row_us for v in got.values())
            md.append("Attribution check, N = %d: ATen's forward takes %.0f µs (C_in = 3) and %.0f µs (C_in = 1); the profile's `igemm_fwd_gtcx35_nhwc_fp32_…"
                      "_bt256x32x4` row is %.1f µs per call.  The attribution of that row to these two layers is **%s** (within 2× counts as "
                      "confirmed)." % (N, got[3], got[1], row_us, "confirmed" if held else "refuted: that row is some other convolution"))
    md += ["", "C_out = 32, 5×5, stride 2, padding 2; the backward includes the input gradient for C_in = 1 only.  GB/s and TFLOP/s are the fused op's, of "
           "algorithmic bytes and 2 flops per multiply-add.", "", "Rows on which the fused median is above ATen's: %s" % (", ".join(losing) if losing else "none")]
    print()
    print("\n".join(md))
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(md) + "\n")
    return 1 if losing else 0


if __name__ == "__main__":
    sys.exit(main())
