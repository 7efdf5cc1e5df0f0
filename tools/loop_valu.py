#!/usr/bin/env python3
"""tools/loop_valu.py ASM KERNEL [KERNEL ...] [--path LABEL,LABEL,...] -- instruction counts of a kernel's outermost loop, per basic block.

ASM is the device assembly of a translation unit, e.g.
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o seed_pass.s compseed_amd/csrc/seed_pass.hip
KERNEL is a substring of the kernel's (mangled) symbol: bwd_win_kernelILi256ELb0E is bwd_win_kernel<256, false>.

A block starts at a label or behind a branch and ends with its branch; its successors are the branch's target and, unless the branch is
unconditional or the block ends the program, the block that follows.  A back edge is a branch to a block at or above its own; the
outermost loop is taken to be the layout range [target, source] of the back edge that spans the most blocks (the compiler lays a loop
out contiguously; blocks it moved out of line are not listed).  Blocks inside a shorter back edge's range are marked with the depth of
that nesting.  Instructions are classed by mnemonic prefix only: v_ VALU, s_load SMEM, other s_ SALU (waits, nops and branches included),
ds_ LDS, global_ / flat_ / buffer_ / scratch_ VMEM.  --path sums the named blocks in the order given (block names as printed: a label, or
LABEL+k for the k-th unlabelled block behind it), which turns "the iteration in which no call ends" into one figure per build.
Needs no GPU."""
import argparse
import re
import sys

CLASSES = ("VALU", "SALU", "SMEM", "VMEM", "LDS", "other")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
FUNC = re.compile(r"^([A-Za-z_][\w$.]*):\s*;\s*@")
INSN = re.compile(r"^\s+([a-z][a-z0-9_]*)\b(.*)$")


def classify(m):
    if m.startswith("v_"):
        return "VALU"
    if m.startswith("s_load"):
        return "SMEM"
    if m.startswith("s_"):
        return "SALU"
    if m.startswith("ds_"):
        return "LDS"
    if m.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    return "other"


class Block:
    def __init__(self, name):
        self.name, self.n, self.succ, self.falls = name, dict.fromkeys(CLASSES, 0), [], True


def functions(lines):
    """{symbol: [line, ...]} of every function body in the file"""
    out, cur, body = {}, None, []
    for ln in lines:
        m = FUNC.match(ln)
        if m:
            cur, body = m.group(1), []
            continue
        if cur is not None:
            if ln.startswith(".Lfunc_end"):
                out[cur] = body
                cur = None
            else:
                body.append(ln)
    return out


def blocks_of(body):
    blocks, cur, anon, base = [], Block("entry"), 0, "entry"
    blocks.append(cur)
    fresh = False                                   # the previous instruction was a branch: the next one opens a block
    for ln in body:
        ln = ln.split(";")[0].rstrip()
        m = LABEL.match(ln)
        if m:
            cur, base, anon, fresh = Block(m.group(1)), m.group(1), 0, False
            blocks.append(cur)
            continue
        m = INSN.match(ln)
        if not m or ln.lstrip().startswith("."):
            continue
        if fresh:
            anon += 1
            cur, fresh = Block("%s+%d" % (base, anon)), False
            blocks.append(cur)
        op, rest = m.group(1), m.group(2)
        cur.n[classify(op)] += 1
        if op.startswith(("s_branch", "s_cbranch")):
            t = re.search(r"(\.LBB\d+_\d+)", rest)
            if t:
                cur.succ.append(t.group(1))
            cur.falls = not op.startswith("s_branch")
            fresh = True
        elif op.startswith(("s_endpgm", "s_setpc")):
            cur.falls, fresh = False, True
    for i, b in enumerate(blocks):
        if b.falls and i + 1 < len(blocks):
            b.succ.append(blocks[i + 1].name)
    return blocks


def report(sym, body, path):
    blocks = blocks_of(body)
    at = {b.name: i for i, b in enumerate(blocks)}
    back = [(at[t], i) for i, b in enumerate(blocks) for t in b.succ if t in at and at[t] <= i]
    print("== %s: %d blocks, %d back edges" % (sym, len(blocks), len(back)))
    if not back:
        print("   no loop")
        return
    lo, hi = max(back, key=lambda e: (e[1] - e[0], -e[0]))
    print("   outermost loop: %s .. %s (%d blocks)" % (blocks[lo].name, blocks[hi].name, hi - lo + 1))
    print("   %-16s %5s %5s %5s %5s %5s %5s  %s" % (("block",) + CLASSES[:5] + ("depth", "successors")))
    tot = dict.fromkeys(CLASSES, 0)
    for i in range(lo, hi + 1):
        b = blocks[i]
        depth = sum(1 for t, s in back if (t, s) != (lo, hi) and t <= i <= s)
        for c in CLASSES:
            tot[c] += b.n[c]
        print("   %-16s %5d %5d %5d %5d %5d %5d  %s" % ((b.name,) + tuple(b.n[c] for c in CLASSES[:5]) + (depth, " ".join(b.succ))))
    print("   %-16s %5d %5d %5d %5d %5d" % (("all blocks",) + tuple(tot[c] for c in CLASSES[:5])))
    if path:
        s = dict.fromkeys(CLASSES, 0)
        for name in path:
            if name not in at:
                sys.exit("no block %s in %s" % (name, sym))
            for c in CLASSES:
                s[c] += blocks[at[name]].n[c]
        print("   %-16s %5d %5d %5d %5d %5d  (%d blocks)" % (("path",) + tuple(s[c] for c in CLASSES[:5]) + (len(path),)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("asm")
    ap.add_argument("kernels", nargs="+")
    ap.add_argument("--path", default="", help="comma-separated block names to sum (one kernel)")
    a = ap.parse_args()
    with open(a.asm) as f:
        funcs = functions(f.read().split("\n"))
    for k in a.kernels:
        hits = [s for s in funcs if k in s]
        if not hits:
            sys.exit("no function matches %s" % k)
        for s in hits:
            report(s, funcs[s], [p for p in a.path.split(",") if p])


if __name__ == "__main__":
    main()
