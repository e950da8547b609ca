#!/usr/bin/env python
"""Per-layer timing of the regresser's full-resolution 3x3 convolutions (lib/gs_parm_network.py:31-50): `out_relu(out_conv(x))` with
out_conv = Conv2d(52, 32, 3, padding=1), and the Conv2d(32, 32, 3, padding=1) that opens each head -- ATen's own convolution against
conv3x3.conv3x3 (the fp32 matrix-core kernels of csrc/conv3x3.hip).

Layers: [2, 52, 1024, 1024] + ReLU and [2, 32, 1024, 1024] (one stereo pair), the same two at N = 8 (training, batch 4), and one ragged size.  For
each: forward alone (no_grad) and forward + backward with all three gradients.  hipEvent brackets on random data after a warm-up; median and
quartiles over --iters calls.  Every timed call is enqueued behind a matrix product of about a millisecond, so the host has finished enqueueing
before the first event fires (the timing method of tools/bench_stemconv.py).

This process itself never touches the GPU.  It starts three children, one after the other, each under its own time limit, and starts nothing more
once one has failed:
  * `fused`: the fused op, all layers in one process -- the autograd op (what a module call costs), and each kernel on its own through the C-ABI
    (forward, input gradient, weight gradient + reduction) for the achieved TFLOP/s against the 157 TF fp32 matrix peak;
  * `aten`, MIOPEN_FIND_MODE unset, and `aten`, MIOPEN_FIND_MODE=FAST (what the profiled runs of profiles/r04_* used): ATen's conv2d (+ relu), the
    same passes, and the names of the GPU kernels one forward call launched (torch.profiler).
The table states ATen's own per-layer times and kernel names and whether they are the two implicit-GEMM rows of profiles/r04_config3_kernel_stats.md
that the work was planned on (`...bt256x32x4`, 1724.6 us per call, supposed to be out_conv; `...bt128x32x32`, 651.6 us, supposed to be the heads'
3x3 layers): confirmed where, at N = 2 under FAST, the time is within 2x of the row's (the rule of profiles/stemconv_shapes.md) AND an implicit-GEMM
kernel with the row's tile is among the call's kernels; refuted otherwise.

Prints one JSON line (all numbers) and a markdown table (also to --md FILE); lists the (layer, pass) rows on which the fused median is above ATen's
under either find mode.  NOT measured here: a training iteration or the pipeline with GPSGS_ACCELERATE=conv3x3 set.  Needs a GPU: no fallback.

    timeout 1100 python tools/bench_conv3x3.py [--iters 10] [--warmup 3] [--md profiles/conv3x3_shapes.md]
"""
import argparse
import json
import os
import signal
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CO = 32
LAYERS = [("out_conv", 2, 52, 1024, 1024, True), ("head[0]", 2, 32, 1024, 1024, False), ("out_conv", 8, 52, 1024, 1024, True),
          ("head[0]", 8, 32, 1024, 1024, False), ("ragged", 2, 52, 511, 771, True)]
PROFILE_US = {52: ("bt256x32x4", 1724.6), 32: ("bt128x32x32", 651.6)}   # profiles/r04_config3_kernel_stats.md, per call, N = 2
PEAK_TF = 157.0


def _quartiles(v):
    v = sorted(v)
    q = lambda f: v[min(len(v) - 1, int(round(f * (len(v) - 1))))]
    return dict(median=q(0.5), q1=q(0.25), q3=q(0.75))


def child(args):
    signal.alarm(args.timeout)
    import torch
    import torch.nn.functional as F

    import gps_gaussian_amd  # noqa: F401
    from gps_gaussian_amd import _capi, _ops, conv3x3

    assert torch.cuda.is_available(), "bench_conv3x3.py needs a GPU"
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
    for name, N, Ci, H, W, relu in LAYERS:
        x = torch.randn(N, Ci, H, W, device=dev).requires_grad_(True)
        w = (torch.randn(CO, Ci, 3, 3, device=dev) * 0.1).requires_grad_(True)
        b = torch.randn(CO, device=dev).requires_grad_(True)
        dy = torch.randn(N, CO, H, W, device=dev)
        rec = dict(layer=name, N=N, C_in=Ci, H=H, W=W, relu=relu)
        if args.child == "fused":
            op = lambda: conv3x3.conv3x3(x, w, b, relu)
        else:
            op = (lambda: F.relu(F.conv2d(x, w, b, padding=1))) if relu else (lambda: F.conv2d(x, w, b, padding=1))

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
            scratch = torch.empty(lib.c3_scratch_bytes(N, Ci, H, W) // 4 + 4, device=dev)
            p = _ops.ptr
            rec["k_fwd"] = timed(lambda: _ops.call("c3_forward", dev, p(xd), p(wd), p(bd), N, Ci, H, W, int(relu), p(y)))
            rec["k_bwd_input"] = timed(lambda: _ops.call("c3_backward", dev, p(xd), p(wd), p(y), p(dy), N, Ci, H, W, int(relu), p(dx), None, None, None))
            rec["k_bwd_weight"] = timed(lambda: _ops.call("c3_backward", dev, p(xd), p(wd), p(y), p(dy), N, Ci, H, W, int(relu), None, p(dw), p(db),
                                                          p(scratch)))
            del y, dx, dw, db, scratch
        else:                       # the GPU kernels of one forward call, by name
            try:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    fwd()
                    torch.cuda.synchronize()
                dev_us = lambda e: float(getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0)))
                ev = sorted((e for e in prof.key_averages() if dev_us(e) > 0), key=lambda e: -dev_us(e))   # kernels only, longest first
                rec["kernels"] = [[e.key[:120], dev_us(e), int(e.count)] for e in ev[:4]]
            except Exception as e:   # the profiler is a convenience: the timings stand without it
                rec["kernels"] = [["(profiler unavailable: %s)" % type(e).__name__, 0.0, 0]]
        rows.append(rec)
        del x, w, b, dy
        torch.cuda.empty_cache()
    print(json.dumps(dict(child=args.child, find_mode=os.environ.get("MIOPEN_FIND_MODE", "default"), device=torch.cuda.get_device_name(0), rows=rows)))
    return 0


def _tflops(r, us, passes=1.0):
    """TFLOP/s of `passes` convolution passes (2 N H W 32 9 C_in FLOP each) done in `us` microseconds"""
    return passes * 2.0 * r["N"] * r["H"] * r["W"] * CO * 9 * r["C_in"] / (us * 1e-6) / 1e12


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
    print(json.dumps(dict(tool="bench_conv3x3", iters=args.iters, warmup=args.warmup, runs=res)))

    cell = lambda d: "%.0f (%.0f–%.0f)" % (d["median"], d["q1"], d["q3"])
    shape = lambda r: "[%d,%d,%d,%d]%s" % (r["N"], r["C_in"], r["H"], r["W"], " + ReLU" if r["relu"] else "")
    md = ["| layer | x | pass | ATen µs, default find (q1–q3) | ATen µs, FAST (q1–q3) | fused µs (q1–q3) | × default | × FAST | fused TFLOP/s |",
          "|" + "---|" * 9]
    losing = []
    for rf, rd, ra in zip(res["fused"]["rows"], res["default"]["rows"], res["FAST"]["rows"]):
        for mode, mult in (("fwd", 1.0), ("fwd_bwd", 3.0)):
            f, a, af = rf[mode], rd[mode], ra[mode]
            md.append("| %s | %s | %s | %s | %s | %s | %.2f | %.2f | %.1f |" % (
                rf["layer"], shape(rf), "fwd" if mode == "fwd" else "fwd+bwd", cell(a), cell(af), cell(f), a["median"] / f["median"],
                af["median"] / f["median"], _tflops(rf, f["median"], mult)))
            if f["median"] > min(a["median"], af["median"]):
                losing.append("%s %s %s" % (rf["layer"], shape(rf), mode))
    md += ["", "fp32, the autograd op on both sides (allocations included).  TFLOP/s: 2·N·H·W·32·9·C_in per pass (forward 1, forward + backward 3 passes) "
           "over the fused median; the fp32 matrix peak is %.0f TF." % PEAK_TF, "",
           "The fused kernels on their own (C-ABI calls on preallocated tensors):", "",
           "| x | k_c3_fwd µs | TF | % of peak | k_c3_bwd_input µs | TF | % of peak | k_c3_bwd_weight + reduce µs | TF | % of peak |", "|" + "---|" * 10]
    for rf in res["fused"]["rows"]:
        cells = []
        for k in ("k_fwd", "k_bwd_input", "k_bwd_weight"):
            tf = _tflops(rf, rf[k]["median"])
            cells += [cell(rf[k]), "%.1f" % tf, "%.0f" % (100.0 * tf / PEAK_TF)]
        md.append("| %s | %s |" % (shape(rf), " | ".join(cells)))
    md += ["", "ATen's GPU kernels of one forward call (torch.profiler: name, µs in that call, launches), MIOPEN_FIND_MODE=FAST:", ""]
    for ra in res["FAST"]["rows"]:
        md.append("- %s: %s" % (shape(ra), "; ".join("`%s` %.0f µs ×%d" % tuple(k) for k in ra["kernels"])))
    md += ["", "... and under the default find mode:", ""]
    for rd in res["default"]["rows"]:
        md.append("- %s: %s" % (shape(rd), "; ".join("`%s` %.0f µs ×%d" % tuple(k) for k in rd["kernels"])))
    md.append("")
    for ra, rd in zip(res["FAST"]["rows"], res["default"]["rows"]):
        if ra["N"] != 2 or ra["layer"] == "ragged":
            continue
        tile, us = PROFILE_US[ra["C_in"]]
        t = ra["fwd"]["median"]
        named = any("igemm" in k[0] and tile in k[0] for k in ra["kernels"] + rd["kernels"])
        held = 0.5 * us <= t <= 2.0 * us
        md.append("Attribution check, %s %s: ATen's forward takes %.0f µs under FAST (%.0f µs under the default find mode), its convolution kernel is "
                  "`%s`; the profile's `igemm_fwd_gtcx35_nhwc_fp32_…_%s` row is %.1f µs per call.  The time is %s 2× of the row's and an implicit-GEMM "
                  "kernel with that tile %s in the call: the attribution of that row to this layer is **%s**."
                  % (ra["layer"], shape(ra), t, rd["fwd"]["median"], ra["kernels"][0][0], tile, us, "within" if held else "NOT within",
                     "appears" if named else "does NOT appear",
                     "confirmed" if held and named else "refuted: that row is some other convolution"))
    md += ["", "Not measured here: a training iteration or the pipeline with GPSGS_ACCELERATE=conv3x3 set.", "",
           "Rows on which the fused median is above ATen's (either find mode): %s" % (", ".join(losing) if losing else "none")]
    print()
    print("\n".join(md))
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(md) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
