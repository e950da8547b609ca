"""Static instruction mix of the kernels of one HIP unit (cross-compiled for gfx950, no GPU needed).
python tools/isa_stats.py gsr_composite_tiles.hip [kernel-substring] [--dump FILE] [extra hipcc flags...]"""
import collections, os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META_KEYS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size")


def unit_flags(unit):
    """The hipcc flags csrc/Makefile compiles `unit` (a file name) with."""
    flags = ["-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-fhip-fp32-correctly-rounded-divide-sqrt"]
    if unit in ("gsr_preprocess.hip",): flags += ["-ffp-contract=off", "-fno-slp-vectorize"]
    if unit in ("corr_sampler.hip", "pack_views.hip", "unproject.hip", "gsr_binning.hip", "splat.hip"): flags += ["-ffp-contract=off"]
    if unit == "gsr_binning.hip": flags += ["-mllvm", "-simplifycfg-sink-common=false"]
    if unit.startswith("gsr_composite") or unit in ("fused_loss.hip", "stem_conv.hip"): flags += ["-fno-slp-vectorize"]
    return flags


def compile_asm(path, out, extra=()):
    """Device-only assembly of the unit at `path`, written to `out`; returns its lines."""
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *unit_flags(os.path.basename(path)), *extra, "-S", "--cuda-device-only", "-o", out, path],
                   check=True, stderr=subprocess.DEVNULL)
    return open(out).read().split("\n")


def kernel_meta(lines):
    """{kernel symbol: {META_KEYS: int}} from the amdhsa.kernels metadata.  Relies on the layout this compiler prints: one YAML list item per kernel
    starting "  - ." (indent 2) with the kernel's own keys at indent 4; deeper items (.args) are skipped.  Another layout gives an empty dict."""
    meta, blk = {}, None
    for l in lines:
        if l.startswith("  - ."): blk = {}
        m = re.match(r"  (?:- |  )\.(\w+):\s+(\S+)", l)
        if m is None or blk is None: continue
        if m.group(1) == "name": meta[m.group(2)] = blk
        elif m.group(1) in META_KEYS: blk[m.group(1)] = int(m.group(2))
    return meta


def kernel_bodies(lines):
    """{kernel symbol: its lines from the symbol to .Lfunc_end}, in the unit's order (a kernel with early exits has several s_endpgm)."""
    bodies, i = {}, 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):", lines[i])
        if m and "k_" in m.group(1):
            j = i
            while j < len(lines) and not lines[j].startswith(".Lfunc_end"): j += 1
            bodies[m.group(1)] = lines[i:j + 1]
            i = j
        i += 1
    return bodies


def opcodes(body):
    return collections.Counter(re.match(r"\s+([a-z_0-9]+)", l).group(1) for l in body if re.match(r"\s+[vsd]_|\s+(global|buffer|flat|ds)_", l))


if __name__ == "__main__":
    src = sys.argv[1]
    args = sys.argv[2:]
    dump = None
    if "--dump" in args:
        i = args.index("--dump"); dump = args[i + 1]; del args[i:i + 2]
    want = args[0] if args and not args[0].startswith("-") else ""
    extra = [a for a in args if a.startswith("-")]
    path = src if os.path.exists(src) else os.path.join(ROOT, "gps-gaussian_amd", "csrc", src)
    lines = compile_asm(path, "/tmp/isa_%s.s" % os.path.basename(path), extra)
    meta = kernel_meta(lines)
    for name, body in kernel_bodies(lines).items():
        if want not in name: continue
        c = opcodes(body)
        cls = collections.Counter()
        for o, n in c.items():
            k = "mfma" if "mfma" in o else "valu" if o.startswith("v_") else "salu" if o.startswith("s_") else "lds" if o.startswith("ds_") else "vmem"
            cls[k] += n
        short = re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", name)[:40]
        print(short, dict(cls), meta.get(name, {}))
        print("   top:", ", ".join("%s %d" % kv for kv in c.most_common(14)))
        if dump: open(dump, "w").write("\n".join(body))
