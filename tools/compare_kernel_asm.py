#!/usr/bin/env python3
"""Compares the device code of two builds of one translation unit, kernel by kernel (by mangled name).

Make the inputs with the Makefile's flags plus `--cuda-device-only -S`, e.g. in compseed_amd/csrc
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off --cuda-device-only -S -o new.s seed_pass.hip
and the same at the commit to compare with.  Prints one line per kernel that differs and a summary; exit status 1 if
any kernel's registers, scratch, LDS or instruction count differ (or, with --text, its instruction text).
--kernarg: loads from the kernel-argument pointer may differ in their offset (an argument struct changed size)."""
import re
import sys

META = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def kernels(path, kernarg):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        ins = [re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0].strip()) for l in m.group(2).split("\n")]
        ins = [l for l in ins if l and not l.startswith((".", "s_nop", "s_code_end")) or l.startswith(".LBB_")]
        if kernarg:  # s_load_* from the kernarg pointer: drop the offset
            ins = [re.sub(r"^(s_load_\w+ \S+ s\[\d+:\d+\],) 0x[0-9a-f]+$", r"\1 OFF", l) for l in ins]
        out[m.group(1)] = {"ins": ins}
    for m in re.finditer(r"^  - \.agpr_count.*?(?=^  - \.agpr_count|^amdhsa\.target)", text, re.M | re.S):
        name = re.search(r"^    \.name:\s+(\S+)", m.group(0), re.M).group(1)
        for k in META:
            out[name][k] = int(re.search(r"^    %s:\s+(\d+)" % re.escape(k), m.group(0), re.M).group(1))
    return {k: v for k, v in out.items() if ".vgpr_count" in v}


def main():
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    a, b = [kernels(p, "--kernarg" in flags) for p in sys.argv[1:] if not p.startswith("--")]
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("only in one build:", name); bad += 1; continue
        ka, kb = a[name], b[name]
        meta = [(k, ka[k], kb[k]) for k in META if ka[k] != kb[k]]
        if len(ka["ins"]) != len(kb["ins"]):
            meta.append(("instructions", len(ka["ins"]), len(kb["ins"])))
        n_text = sum(x != y for x, y in zip(ka["ins"], kb["ins"]))
        if meta or n_text:
            print(name, meta, "%d lines of instruction text differ" % n_text)
        bad += bool(meta) or ("--text" in flags and n_text > 0)
    print("%d kernels compared, %d differ" % (len(set(a) | set(b)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
