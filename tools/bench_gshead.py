#!/usr/bin/env python
"""Per-shape timing of the tail of the three Gaussian-parameter heads, ReLU -> Conv2d(32, K, 1) -> activation (lib/gs_parm_network.py:34-50): the
reference's module chain on ATen against the same chain after gshead.convert() (one FusedHeadConv on the kernels of csrc/gshead.hip).

Shapes: the hidden tensor of a head, [N, 32, 1024, 1024] fp32, for N = 2 (one stereo pair) and N = 8 (training, batch 4), with K = 4 and no
activation (rot_head), K = 3 and Softplus(beta=100) (scale_head), K = 1 and Sigmoid (opacity_head).  For each: forward alone (no_grad) and forward +
backward with all three gradients (the hidden tensor's included, as in training).  hipEvent brackets on random data, the two paths ALTERNATING
call by call after a warm-up of both; median and quartiles over --iters calls.  Every timed call is enqueued behind a matrix product of about a
millisecond, so the host has finished enqueueing before the first event fires (the timing method of tools/bench_stemconv.py).  The input of a call
is a fresh non-leaf copy made BEFORE the bracket: the reference's ReLU is in place.

The ATen side depends on which solver MIOpen picks, and that depends on MIOPEN_FIND_MODE: the profiled runs (profiles/r04_*) used FAST, a plain
run uses the library's default.  So every measurement is taken twice, each in a FRESH child process: one with MIOPEN_FIND_MODE unset, one with
FAST.  This process itself never touches the GPU.  The FAST child also times what the kernel-name attribution of the profiles needs settled:
  * ATen's 1x1 convolution alone at N = 2, against the profile's `igemm_fwd_gtcx35_nhwc_fp32 ... bt128x32x32` row (651.6 us per call, 3 calls per
    view): within 2x counts as confirmed, the rule of profiles/stemconv_shapes.md;
  * ATen's two stem convolutions, Conv2d(3 | 1, 32, 5, stride 2, padding 2) at [2 | 8, C_in, 1024, 1024], against the `bt256x32x4` rows
    (1724.6 us at N = 2, 6395.4 us at N = 8) they were once attributed to: tools/bench_stemconv.py refuted that, but without FAST.
Both children also measure the error of ATen's own elementwise sigmoid and softplus(beta=100) against fp64 on the same fp32 z, in units of u |y|
(u = 2^-24): the figure tests/gshead_ref.py derives its activation tolerance from.

Prints one JSON line (all numbers) and a markdown table (also to --md FILE) with, per row: ATen us under both find modes, fused us, the ratios, and
the fused op's GB/s of algorithmic bytes -- forward (C + K) * 4 bytes per pixel, backward (2 C + K) * 4: h and dy read, dh written.  Exits 1 if on
any row the fused median is above ATen's under the DEFAULT find mode.  Needs a GPU: there is no fallback.

    timeout 1100 python tools/bench_gshead.py [--iters 20] [--warmup 3] [--md profiles/gshead_shapes.md]
"""
import argparse
import copy
import json
import os
import signal
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, H, W = 32, 1024, 1024
HEADS = [("rot", 4, "none"), ("scale", 3, "softplus"), ("opacity", 1, "sigmoid")]
BATCHES = (2, 8)
PROFILE_1X1_US = 651.6                       # profiles/r04_config3_kernel_stats.md: igemm_fwd_gtcx35_nhwc_fp32 ... bt128x32x32, per call
PROFILE_STEM_US = {2: 1724.6, 8: 6395.4}     # the bt256x32x4 rows of r04_config3 / r04_config4 (tools/bench_stemconv.py)


def _quartiles(v):
    v = sorted(v)
    q = lambda f: v[min(len(v) - 1, int(round(f * (len(v) - 1))))]
    return dict(median=q(0.5), q1=q(0.25), q3=q(0.75))


def act_error(dev, n=1 << 22):
    """The worst error of ATen's elementwise sigmoid and softplus(beta=100) on `dev` against fp64 on the same fp32 z, in units of u |y|, over
    results that are normal fp32 numbers.  z: uniform over beta z in [-30, 30] and normal with deviation 3 (softplus: divided by beta)."""
    import torch
    import torch.nn.functional as F

    gen = torch.Generator().manual_seed(1)
    t = torch.cat([torch.rand(n // 2, generator=gen) * 60 - 30, torch.randn(n // 2, generator=gen) * 3])
    out = {}
    for name, z, f in (("sigmoid", t, torch.sigmoid), ("softplus", t / 100, lambda v: F.softplus(v, 100, 20))):
        z = z.float()
        y = f(z.to(dev)).double().cpu()
        y64 = f(z.double())
        ok = y64.abs() >= 2.0 ** -126
        out[name] = float(((y - y64).abs() / (2.0 ** -24 * y64.abs()))[ok].max())
    return out


def child(args):
    """One find mode (whatever MIOPEN_FIND_MODE this process was started with): every timing, as one JSON line."""
    signal.alarm(args.timeout)
    import torch
    from torch import nn

    import gps_gaussian_amd  # noqa: F401
    from gps_gaussian_amd import accelerate, gshead

    assert torch.cuda.is_available(), "bench_gshead.py needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    blk = torch.randn(4096, 4096, device=dev)
    blk_out = torch.empty_like(blk)

    def timed(fns, prepare=lambda: None):
        """fns: tag -> callable(prepared); alternating, each call bracketed by events behind a matrix product -> tag -> quartiles (us)"""
        times = {tag: [] for tag in fns}
        for it in range(args.warmup + args.iters):
            for tag, fn in fns.items():
                inp = prepare()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.mm(blk, blk, out=blk_out)   # keeps the GPU busy while the host enqueues what follows
                e0.record()
                fn(inp)
                e1.record()
                e1.synchronize()
                if it >= args.warmup:
                    times[tag].append(e0.elapsed_time(e1) * 1e3)
        return {tag: _quartiles(v) for tag, v in times.items()}

    rows, conv_only, stems = [], {}, []
    for N in BATCHES:
        x = torch.randn(N, C, H, W, device=dev)
        for head, K, act in HEADS:
            tail = {"none": [], "softplus": [nn.Softplus(beta=100)], "sigmoid": [nn.Sigmoid()]}[act]
            aten = nn.Sequential(nn.ReLU(inplace=True), nn.Conv2d(C, K, 1), *tail).to(dev)
            fused = copy.deepcopy(aten)
            assert gshead.convert(fused) == 1
            dy = torch.randn(N, K, H, W, device=dev)
            leaf = x.clone().requires_grad_(True)

            def fwd(m):
                def run(h):
                    with torch.no_grad():
                        return m(h)
                return run

            def fwdbwd(m):
                def run(h):   # the gradient of the tensor BEFORE the in-place ReLU (`h` itself names the rectified one afterwards)
                    y = m(h)
                    return torch.autograd.grad(y, (leaf,) + tuple(m.parameters()), dy)
                return run

            rec = dict(head=head, N=N, C=C, K=K, act=act, H=H, W=W)
            before = accelerate.calls["gshead"]
            rec["fwd"] = timed({"aten": fwd(aten), "fused": fwd(fused)}, prepare=lambda: x.clone())
            rec["fwd_bwd"] = timed({"aten": fwdbwd(aten), "fused": fwdbwd(fused)}, prepare=lambda: leaf + 0)   # a non-leaf that requires grad
            assert accelerate.calls["gshead"] - before == 2 * (args.warmup + args.iters)   # the fused path really ran the kernels
            rows.append(rec)
            if N == 2:   # the convolution alone: what the profile's implicit-GEMM row would be
                conv = aten[1]
                conv_only[K] = timed({"aten": fwd(conv)}, prepare=lambda: x)["aten"]
            del aten, fused, dy, leaf
        del x
        torch.cuda.empty_cache()
    for N in BATCHES:
        for Ci in (3, 1):
            conv = nn.Conv2d(Ci, 32, 5, stride=2, padding=2).to(dev)
            x = torch.randn(N, Ci, H, W, device=dev)
            with torch.no_grad():
                stems.append(dict(N=N, C_in=Ci, fwd=timed({"aten": lambda inp, m=conv: m(inp)}, prepare=lambda: x)["aten"]))
            del x, conv
    print(json.dumps(dict(find_mode=os.environ.get("MIOPEN_FIND_MODE", "default"), device=torch.cuda.get_device_name(0), rows=rows,
                          conv_only=conv_only, stems=stems, act_error=act_error(dev))))
    return 0


def _bytes(K, N, mode):
    px = N * H * W
    return 4 * px * ((C + K) if mode == "fwd" else (C + K) + (2 * C + K))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=500, help="each child process ends itself after this many seconds")
    ap.add_argument("--md", default=None, help="also write the markdown table to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)

    res = {}
    for mode in ("default", "FAST"):
        env = dict(os.environ)
        env.pop("MIOPEN_FIND_MODE", None)
        if mode == "FAST":
            env["MIOPEN_FIND_MODE"] = "FAST"
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--iters", str(args.iters), "--warmup", str(args.warmup), "--timeout", str(args.timeout)]
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=args.timeout + 30)
        if r.returncode != 0:      # a child that failed: nothing more is started on the GPU
            print(r.stdout[-4000:])
            return r.returncode or 1
        res[mode] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(dict(tool="bench_gshead", iters=args.iters, warmup=args.warmup, runs=res)))

    cell = lambda d: "%.0f (%.0f–%.0f)" % (d["median"], d["q1"], d["q3"])
    md = ["| head | h | K, act | pass | ATen µs, default find (q1–q3) | ATen µs, FAST (q1–q3) | fused µs (q1–q3) | × default | × FAST | fused GB/s |",
          "|" + "---|" * 10]
    losing = []
    for rd, rf in zip(res["default"]["rows"], res["FAST"]["rows"]):
        for mode in ("fwd", "fwd_bwd"):
            a, af, f = rd[mode]["aten"], rf[mode]["aten"], rd[mode]["fused"]
            md.append("| %s | [%d,%d,%d,%d] | %d, %s | %s | %s | %s | %s | %.2f | %.2f | %.0f |" % (
                rd["head"], rd["N"], C, H, W, rd["K"], rd["act"], "fwd" if mode == "fwd" else "fwd+bwd", cell(a), cell(af), cell(f),
                a["median"] / f["median"], af["median"] / f["median"], _bytes(rd["K"], rd["N"], mode) / f["median"] / 1e3))
            if f["median"] > a["median"]:
                losing.append("%s [%d,%d,%d,%d] %s" % (rd["head"], rd["N"], C, H, W, mode))
    md += ["", "fp32; the fused column is the one measured beside the default-find ATen column (the FAST child's fused medians: %s µs).  GB/s: the fused "
           "op's, of algorithmic bytes -- forward (C + K)·4 B per pixel, backward (2C + K)·4 B." % ", ".join(
               "%.0f / %.0f" % (r["fwd"]["fused"]["median"], r["fwd_bwd"]["fused"]["median"]) for r in res["FAST"]["rows"]), ""]
    co = res["FAST"]["conv_only"]
    got = {int(k): v["median"] for k, v in co.items()}
    held = all(0.5 * PROFILE_1X1_US <= v <= 2.0 * PROFILE_1X1_US for v in got.values())
    md.append("Attribution check (MIOPEN_FIND_MODE=FAST, N = 2): ATen's 1×1 convolution forward alone takes %s; the profile's "
              "`igemm_fwd_gtcx35_nhwc_fp32_…_bt128x32x32` row is %.1f µs per call.  The attribution of that row to the three 1×1 head convolutions is "
              "**%s** (within 2× counts as confirmed).  Under the default find mode the same calls take %s."
              % (", ".join("%.0f µs (K = %d)" % (got[k], k) for k in sorted(got, reverse=True)), PROFILE_1X1_US,
                 "confirmed" if held else "refuted: that row is some other convolution",
                 ", ".join("%.0f µs (K = %d)" % (res["default"]["conv_only"][str(k)]["median"], k) for k in sorted(got, reverse=True))))
    md.append("")
    for N, row_us in sorted(PROFILE_STEM_US.items()):
        t = {m: {s["C_in"]: s["fwd"]["median"] for s in res[m]["stems"] if s["N"] == N} for m in res}
        held = all(0.5 * row_us <= v <= 2.0 * row_us for v in t["FAST"].values())
        md.append("Stem convolutions, N = %d: ATen's forward takes %.0f µs (C_in = 3) and %.0f µs (C_in = 1) under FAST, %.0f µs and %.0f µs under the "
                  "default find mode; the `bt256x32x4` row is %.1f µs per call.  Under FAST the attribution of that row to the stems is **%s**."
                  % (N, t["FAST"][3], t["FAST"][1], t["default"][3], t["default"][1], row_us,
                     "confirmed" if held else "refuted, as without FAST: the earlier refutation was not a find-mode artefact"))
    md += ["", "Error of ATen's own elementwise activations on this GPU against fp64 on the same fp32 z, worst over 2^22 points, in units of u·|y| "
           "(u = 2^-24): sigmoid %.3f, softplus(beta=100) %.3f." % (res["default"]["act_error"]["sigmoid"], res["default"]["act_error"]["softplus"]),
           "", "Rows on which the fused median is above ATen's: %s" % (", ".join(losing) if losing else "none")]
    print()
    print("\n".join(md))
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(md) + "\n")
    return 1 if losing else 0


if __name__ == "__main__":
    sys.exit(main())
