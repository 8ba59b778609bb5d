#!/usr/bin/env python3
"""Value-only mutants of atspeed_amd/csrc/scan.hip for tests/test_walk_gpu.py (profiles/walk_mutations.txt).

    python tools/walk_mutants.py OUT_DIR            # needs the built library (atspeed_amd/lib/libatspeed_hip.so)

For every mutant: a scratch copy of scan.hip with the textual replacements below, compiled with the Makefile's flags and linked into a SMALL
library OUT_DIR/<name>.so that holds the mutated scan object alone and names the built library as its dependency.  Loaded through
ATSPEED_LIB, the calls tests/test_walk_gpu.py makes (atspeed_beam_sample_step, atspeed_verify_walk) resolve to the mutant and launch its
kernels; everything else resolves to the built library.  Run one pytest process per mutant:

    ATSPEED_LIB=OUT_DIR/<name>.so python -m pytest tests/test_walk_gpu.py -k "test_sampled_step or test_sampled_walk or test_greedy_walk"

No replacement changes an address, the bound of a memory access, a loop count or a barrier.  `--predict` prints, without a GPU, the cases
the same wrong rule changes in tests/walk_ref.py.
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "atspeed_amd", "csrc")

# name: (the rule of tests/walk_ref.py that restates it, [(old text, new text), ...])
MUTANTS = {
    "m1_accept_strict": ("accept_strict", [("acc = (u * q <= p) ? 1 : 0;", "acc = (u * q < p) ? 1 : 0;")]),
    "m2_taken_ignored": ("residual_keeps_taken", [("        if (!taken) {\n          pr[s2] = p;", "        if (true) {\n          pr[s2] = p;")]),
    "m3_no_fallback": ("no_fallback", [("    if (tot == 0.f) {\n#pragma unroll", "    if (false) {\n#pragma unroll")]),
    "m4_subset_largest": ("subset_largest", [("(d_h[j] < d_h[tid] || (d_h[j] == d_h[tid] && j < tid))",
                                              "(d_h[j] > d_h[tid] || (d_h[j] == d_h[tid] && j < tid))")]),
    "m5_rf_on_tid": ("draft_order", [("rf += (d_acc[j] && d_flat[j] < d_flat[tid]) ? 1 : 0;", "rf += (d_acc[j] && j < tid) ? 1 : 0;")]),
    "m6_rank_on_flat": ("hit_by_flat", [("if (tid < k) { t_pos[tid] = pos; if (pos < 0) atomicOr(&reject, 1); }",
                                         "if (tid < k) { t_pos[tid] = pk.flat; if (pos < 0) atomicOr(&reject, 1); }"),
                                        ("for (int j = 0; j < k; ++j) rank += (t_pos[j] < pos) ? 1 : 0;\n      hit[rank] = pos;",
                                         "for (int j = 0; j < k; ++j) rank += (t_pos[j] < pk.flat) ? 1 : 0;\n      hit[rank] = pos;")]),
    "m7_vis_word0": ("vis_word0", [("if ((s >> 6) == w) bits |= 1ull << (s & 63);", "if (w == 0) bits |= 1ull << (s & 63);")]),
    "m8_base_no_cnt": ("base_no_cnt", [("const int base_next = a.cur.slot[rowbase] + cnt;", "const int base_next = a.cur.slot[rowbase];")]),
    "m9_accept_swapped": ("accept_swapped", [("acc = (u * q <= p) ? 1 : 0;", "acc = (u * p <= q) ? 1 : 0;")]),
}
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + CSRC]


def predict():
    sys.path.insert(0, ROOT)
    from tests import walk_cases as W
    from tests.test_walk_cpu import _same
    cases = [("test_sampled_walk", c) for c in W.sampled_walk_cases()] + [("test_greedy_walk", c) for c in W.greedy_walk_cases()]
    for name, (rule, _) in MUTANTS.items():
        bad = [f"{t}[{c.name}]" for t, c in cases if not _same(c.expected(), c.expected((rule,)))]
        print(name, rule, len(bad), " ".join(bad))


def build(out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    lib_dir = os.path.join(ROOT, "atspeed_amd", "lib")
    src = open(os.path.join(CSRC, "scan.hip")).read()
    os.makedirs(out, exist_ok=True)
    for name, (_, subs) in MUTANTS.items():
        text = src
        for old, new in subs:
            assert text.count(old) == 1, (name, old, text.count(old))
            text = text.replace(old, new)
        d = os.path.join(out, name)
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "scan.hip"), "w") as f:
            f.write(text)
        subprocess.check_call([hipcc] + FLAGS + ["-c", os.path.join(d, "scan.hip"), "-o", os.path.join(d, "scan.o")])
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", os.path.join(out, name + ".so"), os.path.join(d, "scan.o"),
                               "-L" + lib_dir, "-l:libatspeed_hip.so", "-Wl,-rpath," + lib_dir])
        print(name, "built")


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "--predict":
        predict()
    elif len(sys.argv) == 2:
        build(sys.argv[1])
    else:
        sys.exit(__doc__)
