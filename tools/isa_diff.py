"""Does a source change alter the device code of one HIP unit?  Cross-compiles the unit in two trees with its Makefile flags (gfx950, no GPU needed) and
compares the assembly kernel by kernel.  Exit status 0 only if every kernel body is identical.
python tools/isa_diff.py OLD_TREE NEW_TREE gsr_composite.hip"""
import os, sys, tempfile
from isa_stats import META_KEYS, compile_asm, kernel_bodies, kernel_meta, opcodes


def unit_kernels(tree, unit, tmp, tag):
    lines = compile_asm(os.path.join(tree, "gps-gaussian_amd", "csrc", unit), os.path.join(tmp, tag + ".s"))
    bodies = {k: [l for l in b if "__hip_cuid_" not in l] for k, b in kernel_bodies(lines).items()}
    return bodies, kernel_meta(lines)


def main(old_tree, new_tree, unit):
    with tempfile.TemporaryDirectory() as tmp:
        old, old_meta = unit_kernels(old_tree, unit, tmp, "old")
        new, new_meta = unit_kernels(new_tree, unit, tmp, "new")
    same = 0
    for name in list(old) + [k for k in new if k not in old]:
        if name not in old or name not in new:
            print("%s: only in %s" % (name, "OLD" if name in old else "NEW"))
        elif old[name] == new[name]:
            same += 1
            print("%s: identical" % name)
        else:
            a, b = opcodes(old[name]), opcodes(new[name])
            delta = ", ".join("%s %+d" % (o, b[o] - a[o]) for o in sorted(set(a) | set(b)) if a[o] != b[o])
            print("%s: DIFFERS (%d -> %d lines); opcodes: %s" % (name, len(old[name]), len(new[name]), delta or "same counts, other order or operands"))
            for k in META_KEYS:
                print("    .%s: %s -> %s" % (k, old_meta.get(name, {}).get(k), new_meta.get(name, {}).get(k)))
    total = len(set(old) | set(new))
    print("%s: %d of %d kernel bodies identical" % (unit, same, total))
    return 0 if same == total else 1


if __name__ == "__main__":
    if len(sys.argv) != 4: sys.exit(__doc__)
    sys.exit(main(*sys.argv[1:]))
