#!/usr/bin/env python3
"""Per-kernel comparison of two builds' device assembly: which kernels a change left identical, which it altered, added or removed.

    tools/isa_compare.py OLD NEW

OLD and NEW are two .s files (hipcc -S --cuda-device-only, or what -save-temps leaves: csrc/.isa/*-gfx950.s) or two directories of them
(files are paired by name, sub-directories included: .isa/ and .isa/f16/).  A file is split into kernels by symbol: the body runs from the
label `<symbol>:` to the kernel's `.amdhsa_kernel <symbol>` directive, the descriptor from there to `.end_amdhsa_kernel`.  Before the
comparison assembler comments are dropped and the function ordinal in local labels (.LBB<fn>_<block> -> .LBB_<block>) is removed: it is the
position of the function in the module, which moves when another function comes or goes, not machine code.  Kernels are matched under the
demangled name (llvm-cxxfilt / c++filt when there is one, else the symbol).

Text only: the tool knows no instruction by name; an "instruction" is a body line that is neither a label nor a directive.  For a differing
kernel it prints one row: instruction count, then the descriptor's next_free_vgpr, accum_offset, next_free_sgpr, group_segment_fixed_size
(LDS) and private_segment_fixed_size (scratch), each as old -> new.  Exit status 1 when any kernel
differs, was added or was removed."""
import os
import re
import shutil
import subprocess
import sys

FIELDS = ("next_free_vgpr", "accum_offset", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")
_LOCAL = re.compile(r"(\.L[A-Za-z_]+?)\d+_(\d+)")


def _clean(line):
    line = line.split(";", 1)[0].rstrip()
    return _LOCAL.sub(r"\1_\2", line).strip()


def kernels(path):
    """{symbol: (body lines, descriptor lines)} of one .s file"""
    with open(path, errors="replace") as f:
        lines = f.read().splitlines()
    label = {}
    for i, ln in enumerate(lines):
        head = ln.split(";", 1)[0].rstrip()
        if head.endswith(":") and not head[0].isspace() and not head.startswith("."):
            label.setdefault(head[:-1], i)
    out = {}
    for i, ln in enumerate(lines):
        t = ln.split()
        if len(t) == 2 and t[0] == ".amdhsa_kernel" and t[1] in label:
            end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
            body = [c for c in map(_clean, lines[label[t[1]] + 1:i]) if c]
            out[t[1]] = (body, [c for c in map(_clean, lines[i + 1:end]) if c])
    return out


def demangle(symbols):
    tool = next((p for p in (shutil.which("llvm-cxxfilt"), "/opt/rocm/llvm/bin/llvm-cxxfilt", shutil.which("c++filt")) if p and os.path.exists(p)), None)
    if not tool or not symbols:
        return {s: s for s in symbols}
    res = subprocess.run([tool], input="\n".join(symbols) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(symbols, res))


def by_name(path):
    ks = kernels(path)
    names = demangle(sorted(ks))
    return {names[s]: v for s, v in ks.items()}


def figures(kernel):
    body, desc = kernel
    n_instr = sum(1 for ln in body if not ln.endswith(":") and not ln.startswith("."))
    d = {ln.split()[0][len(".amdhsa_"):]: ln.split()[1] for ln in desc if len(ln.split()) == 2}
    return [str(n_instr)] + [d.get(k, "-") for k in FIELDS]


def short(name):
    """demangled name without the return type, the anonymous namespace and the parameter list"""
    name = re.sub(r"^void ", "", name).replace("(anonymous namespace)::", "")
    k = name.find(">(")
    return name[:k + 1] if k >= 0 else name.split("(")[0]


def row(name, old, new):
    cols = ("instr", "vgpr", "accum", "sgpr", "lds", "scratch")
    return "%-66s " % short(name) + "  ".join("%s %s -> %s" % (c, o, n) if old is not None else "%s %s" % (c, n)
                                               for c, o, n in zip(cols, old or new, new))


def compare(old, new, title):
    a, b = by_name(old), by_name(new)
    same = [n for n in a if n in b and a[n] == b[n]]
    diff = [n for n in a if n in b and a[n] != b[n]]
    added, removed = [n for n in b if n not in a], [n for n in a if n not in b]
    print("%s: old %d kernels, new %d; identical body+descriptor %d, differing %d, new %d, only in old %d"
          % (title, len(a), len(b), len(same), len(diff), len(added), len(removed)))
    for n in sorted(diff):
        print("    differs: " + row(n, figures(a[n]), figures(b[n])))
    for n in sorted(added):
        print("    new:     " + row(n, None, figures(b[n])))
    for n in sorted(removed):
        print("    only in old: %s" % n)
    return bool(diff or added or removed)


def s_files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs if f.endswith(".s"))


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    old, new = argv[1:]
    if os.path.isdir(old) != os.path.isdir(new):
        print("give two files or two directories")
        return 2
    if not os.path.isdir(old):
        return int(compare(old, new, os.path.basename(new)))
    fo, fn = s_files(old), s_files(new)
    changed = False
    for rel in fo:
        if rel in fn:
            changed |= compare(os.path.join(old, rel), os.path.join(new, rel), rel)
        else:
            print("%s: only in %s" % (rel, old))
            changed = True
    for rel in fn:
        if rel not in fo:
            print("%s: only in %s" % (rel, new))
            changed = True
    return int(changed)


if __name__ == "__main__":
    sys.exit(main(sys.argv))
