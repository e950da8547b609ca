#!/usr/bin/env python
"""Per-layer timing of the stride-1 3x3 convolutions of the residual blocks (core/extractor.py:10-11) at the widths of stage 2's depth encoder
and decoders -- ATen's own convolution against resconv.conv3x3 (the fp32 matrix-core kernels of csrc/resconv.hip).

Layers: the eight distinct shapes of one 1024^2 stereo pair (LAYERS: name, how many of the pair's 22 layers have the shape, C_in, C_out, plane),
at N = 2 (one pair) and N = 8 (training, batch 4).  For each: forward alone (no_grad) and forward + backward with all three gradients.  hipEvent
brackets on random data after a warm-up; median and quartiles over --iters calls.  Every timed call is enqueued behind a matrix product of about a
millisecond, so the host has finished enqueueing before the first event fires (the timing method of tools/bench_stemconv.py).

This process itself never touches the GPU.  It starts three children, one after the other, each under its own alarm, and starts nothing more once
one has failed:
  * `fused`: the fused op, all layers in one process -- the autograd op (what a module call costs), each kernel on its own through the C-ABI
    (forward, input gradient, weight gradient + reduction) for the achieved TFLOP/s against the 157 TF fp32 matrix peak;
  * `aten`, MIOPEN_FIND_MODE unset, and `aten`, MIOPEN_FIND_MODE=FAST: ATen's conv2d, the same passes, and the names of the GPU kernels one forward
    and one backward call launched (torch.profiler).
A row WINS where the fused upper quartile is below ATen's lower quartile under both find modes; every other row loses.  The total line is the sum of
the forward + backward medians over the 22 layers of a pair (each shape times its count), ATen (the faster find mode per row) against the fused op
as routed: the fused median where resconv.keeps() (the routing rule of FusedResConv3x3, asked by this process for each row's sizes and the
device's compute-unit count) keeps the row, ATen's where it routes it away.  --render FILE renders the table again from the JSON line of an earlier
run (no GPU work): the numbers are that run's, the `routed to` column and the totals follow the rule as it stands.

Prints one JSON line (all numbers) and a markdown table (also to --md FILE).  NOT measured here: a training iteration or the pipeline with the
layers converted.  Needs a GPU: no fallback.

    timeout 1100 python tools/bench_resconv.py [--iters 10] [--warmup 3] [--md profiles/resconv_shapes.md]
"""
import argparse
import json
import os
import signal
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (where the shape occurs, layers of one pair with it, C_in, C_out, H, W): 4 + 3 + 1 + 3 + 3 + 1 + 6 + 1 = 22
LAYERS = [("depth res1", 4, 32, 32, 512, 512), ("decoder1", 3, 48, 48, 512, 512), ("decoder1[0].conv1", 1, 128, 48, 512, 512),
          ("depth res2", 3, 48, 48, 256, 256), ("decoder2", 3, 64, 64, 256, 256), ("decoder2[0].conv1", 1, 192, 64, 256, 256),
          ("depth res3, decoder3", 6, 96, 96, 128, 128), ("decoder3[0].conv1", 1, 192, 96, 128, 128)]
BATCHES = (2, 8)
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
    from gps_gaussian_amd import _capi, _ops, resconv

    assert torch.cuda.is_available(), "bench_resconv.py needs a GPU"
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
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

    def kernels(fn):
        """the GPU kernels of one call, by name, longest first"""
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            dev_us = lambda e: float(getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0)))
            ev = sorted((e for e in prof.key_averages() if dev_us(e) > 0), key=lambda e: -dev_us(e))
            return [[e.key[:100], dev_us(e), int(e.count)] for e in ev[:5]]
        except Exception as e:   # the profiler is a convenience: the timings stand without it
            return [["(profiler unavailable: %s)" % type(e).__name__, 0.0, 0]]

    rows = []
    for N in BATCHES:
        for name, count, Ci, Co, H, W in LAYERS:
            x = torch.randn(N, Ci, H, W, device=dev).requires_grad_(True)
            w = (torch.randn(Co, Ci, 3, 3, device=dev) * 0.1).requires_grad_(True)
            b = torch.randn(Co, device=dev).requires_grad_(True)
            dy = torch.randn(N, Co, H, W, device=dev)
            rec = dict(layer=name, count=count, N=N, C_in=Ci, C_out=Co, H=H, W=W)
            op = (lambda: resconv.conv3x3(x, w, b)) if args.child == "fused" else (lambda: F.conv2d(x, w, b, padding=1))

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
                scratch = torch.empty(lib.rc_scratch_bytes(N, Ci, Co, H, W) // 4 + 4, device=dev)
                p = _ops.ptr
                rec["k_fwd"] = timed(lambda: _ops.call("rc_forward", dev, p(xd), p(wd), p(bd), N, Ci, Co, H, W, p(y)))
                rec["k_bwd_input"] = timed(lambda: _ops.call("rc_backward", dev, p(xd), p(wd), p(dy), N, Ci, Co, H, W, p(dx), None, None, None))
                rec["k_bwd_weight"] = timed(lambda: _ops.call("rc_backward", dev, p(xd), p(wd), p(dy), N, Ci, Co, H, W, None, p(dw), p(db), p(scratch)))
                del y, dx, dw, db, scratch
            else:
                rec["kernels"] = kernels(fwd)
                rec["kernels_bwd"] = kernels(fwd_bwd)
            rows.append(rec)
            del x, w, b, dy
            torch.cuda.empty_cache()
    print(json.dumps(dict(child=args.child, find_mode=os.environ.get("MIOPEN_FIND_MODE", "default"), device=torch.cuda.get_device_name(0),
                          compute_units=cus, rows=rows)))
    return 0


def _tflops(r, us, passes=1.0):
    """TFLOP/s of `passes` convolution passes (2 N H W C_out 9 C_in FLOP each) done in `us` microseconds"""
    return passes * 2.0 * r["N"] * r["H"] * r["W"] * r["C_out"] * 9 * r["C_in"] / (us * 1e-6) / 1e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300, help="each child process ends itself after this many seconds")
    ap.add_argument("--md", default=None, help="also write the markdown table to this file")
    ap.add_argument("--render", default=None, help="no GPU work: render the table again from the JSON line a run printed (a file holding it)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)

    res = {}
    if args.render:
        with open(args.render) as f:
            saved = json.loads([l for l in f.read().splitlines() if l.startswith("{")][-1])
        res, args.iters, args.warmup = saved["runs"], saved["iters"], saved["warmup"]
    for tag, kind, mode in (() if args.render else (("fused", "fused", None), ("default", "aten", None), ("FAST", "aten", "FAST"))):
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
        print("bench_resconv: child %s done" % tag, file=sys.stderr, flush=True)
    if not args.render:
        print(json.dumps(dict(tool="bench_resconv", iters=args.iters, warmup=args.warmup, runs=res)))
    from gps_gaussian_amd import resconv     # the routing rule is a function of the sizes and the device's compute units: no GPU needed to ask it
    cus = res["fused"]["compute_units"]
    for r in res["fused"]["rows"]:
        dims = (r["N"], r["C_in"], r["C_out"], r["H"], r["W"])
        r["kept"] = dict(fwd=bool(resconv.keeps(*dims, False, cus)), fwd_bwd=bool(resconv.keeps(*dims, True, cus)))

    cell = lambda d: "%.0f (%.0f–%.0f)" % (d["median"], d["q1"], d["q3"])
    shape = lambda r: "[%d,%d,%d,%d] → %d" % (r["N"], r["C_in"], r["H"], r["W"], r["C_out"])
    md = ["Device: %s, %d compute units." % (res["fused"]["device"], res["fused"]["compute_units"]), "",
          "| layer | ×/pair | x → C_out | pass | ATen µs, default find (q1–q3) | ATen µs, FAST (q1–q3) | fused µs (q1–q3) | × default | × FAST | "
          "fused TFLOP/s | verdict | routed to |",
          "|" + "---|" * 12]
    totals = {N: dict(aten=0.0, routed=0.0, fused=0.0) for N in BATCHES}
    won, lost = [], []
    for rf, rd, ra in zip(res["fused"]["rows"], res["default"]["rows"], res["FAST"]["rows"]):
        for mode, mult in (("fwd", 1.0), ("fwd_bwd", 3.0)):
            f, a, af = rf[mode], rd[mode], ra[mode]
            wins = f["q3"] < min(a["q1"], af["q1"])
            (won if wins else lost).append("%s %s" % (shape(rf), mode))
            md.append("| %s | %d | %s | %s | %s | %s | %s | %.2f | %.2f | %.1f | %s | %s |" % (
                rf["layer"], rf["count"], shape(rf), "fwd" if mode == "fwd" else "fwd+bwd", cell(a), cell(af), cell(f), a["median"] / f["median"],
                af["median"] / f["median"], _tflops(rf, f["median"], mult), "wins" if wins else "loses", "fused" if rf["kept"][mode] else "ATen"))
            if mode == "fwd_bwd":
                best = min(a["median"], af["median"])
                t = totals[rf["N"]]
                t["aten"] += rf["count"] * best
                t["fused"] += rf["count"] * f["median"]
                t["routed"] += rf["count"] * (f["median"] if rf["kept"][mode] else best)
    md += ["", "fp32, the autograd op on both sides (allocations included).  TFLOP/s: 2·N·H·W·C_out·9·C_in per pass (forward 1, forward + backward 3 "
           "passes) over the fused median; the fp32 matrix peak is %.0f TF.  A row wins where the fused upper quartile is below ATen's lower "
           "quartile under both find modes.  `routed to`: what resconv.keeps() answers for the call." % PEAK_TF, ""]
    for N in BATCHES:
        t = totals[N]
        md.append("Total, N = %d: forward + backward medians summed over the 22 layers of a pair (each shape × its count): ATen (the faster find mode "
                  "per row) %.0f µs; fused as routed %.0f µs (%.2f×); fused on every layer %.0f µs (%.2f×)."
                  % (N, t["aten"], t["routed"], t["aten"] / t["routed"], t["fused"], t["aten"] / t["fused"]))
    md += ["", "The fused kernels on their own (C-ABI calls on preallocated tensors):", "",
           "| x → C_out | k_rc_fwd µs | TF | % of peak | k_rc_bwd_input µs | TF | % of peak | k_rc_bwd_weight + reduce µs | TF | % of peak |", "|" + "---|" * 10]
    for rf in res["fused"]["rows"]:
        cells = []
        for k in ("k_fwd", "k_bwd_input", "k_bwd_weight"):
            tf = _tflops(rf, rf[k]["median"])
            cells += [cell(rf[k]), "%.1f" % tf, "%.0f" % (100.0 * tf / PEAK_TF)]
        md.append("| %s | %s |" % (shape(rf), " | ".join(cells)))
    for tag, title in (("FAST", "MIOPEN_FIND_MODE=FAST"), ("default", "the default find mode")):
        md += ["", "ATen's GPU kernels of one forward call, then of one forward + backward call (torch.profiler: name, µs in that call, launches), %s:" % title, ""]
        for r in res[tag]["rows"]:
            fmt = lambda ks: "; ".join("`%s` %.0f µs ×%d" % tuple(k) for k in ks)
            md.append("- %s: %s — fwd+bwd: %s" % (shape(r), fmt(r["kernels"]), fmt(r["kernels_bwd"])))
    md += ["", "Not measured here: a training iteration or the pipeline with the layers converted.", "",
           "Rows that win: %s" % (", ".join(won) if won else "none"), "", "Rows that lose: %s" % (", ".join(lost) if lost else "none")]
    print()
    print("\n".join(md))
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(md) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
