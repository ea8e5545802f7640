#!/usr/bin/env python3
"""Static instruction categories of one kernel per source range, from a
listing with line tables:

  hipcc <the Makefile's HIPFLAGS> -gline-tables-only --cuda-device-only -S -o k.s rt_kernel.hip
  python scripts/isa_blocks.py k.s 'render_kernel<false, true, 1, 4, true, true>' \\
      --part head=rt_device.h:1586-1660 --part guard=rt_device.h:198-204,rt_device.h:1672-1674 ...

Every instruction of the kernel is attributed to the innermost source line of
its `.loc` (inlined code carries the callee's line) and counted in the first
part whose ranges hold that line; the rest is "(elsewhere)".  The counts are
static and sum over every inlined copy of a range in the kernel: they compare
two builds of the same text, they are not a trip through one iteration.
Without --part the script prints the counts per source file.

Categories: fp64 arith (v_*_f64 but compares), v_cmp, select/move (v_cndmask,
v_mov, accvgpr moves), lane moves (v_readlane, v_writelane, v_readfirstlane),
other VALU, SALU (but branches, waits and nops), branches, s_nop, memory (loads,
stores, LDS, scalar loads) and s_waitcnt."""
import argparse
import collections
import re
import subprocess

CATS = ["fp64", "v_cmp", "sel/mov", "lane", "valu", "salu", "branch", "s_nop", "mem", "wait"]


def category(op):
    if op.startswith("v_cmp"):
        return "v_cmp"
    if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
        return "lane"
    if op.startswith(("v_cndmask", "v_mov", "v_accvgpr")):
        return "sel/mov"
    if op.startswith("v_") and "_f64" in op:
        return "fp64"
    if op.startswith("v_"):
        return "valu"
    if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc", "s_call", "s_endpgm")):
        return "branch"
    if op == "s_nop":
        return "s_nop"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith(("s_load", "s_buffer_load", "global_", "flat_", "scratch_", "buffer_", "ds_")):
        return "mem"
    if op.startswith("s_"):
        return "salu"
    return "valu"


def kernel_body(lines, want):
    """Lines of the function whose demangled name holds `want`."""
    labels = [(i, m.group(1)) for i, l in enumerate(lines) if (m := re.match(r"^(_Z\w+):", l))]
    names = subprocess.run(["c++filt"], input="\n".join(n for _, n in labels), capture_output=True,
                           text=True).stdout.splitlines()
    hits = [(i, n) for (i, _), n in zip(labels, names) if want in n]
    if len(hits) != 1:
        raise SystemExit("kernel name matches %d functions: %s" % (len(hits), [n for _, n in hits][:8]))
    start = hits[0][0]
    for j in range(start, len(lines)):
        if lines[j].startswith(".Lfunc_end"):
            return hits[0][1], lines[start:j]
    raise SystemExit("no end of function")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("listing")
    ap.add_argument("kernel")
    ap.add_argument("--part", action="append", default=[], metavar="NAME=FILE:LO-HI[,FILE:LO-HI...]")
    a = ap.parse_args()
    lines = open(a.listing).read().splitlines()
    files = {}
    for l in lines:
        m = re.match(r'\s*\.file\s+(\d+)\s+(?:"([^"]*)"\s+)?"([^"]*)"', l)
        if m:
            files[int(m.group(1))] = m.group(3).rsplit("/", 1)[-1]
    parts = []
    for p in a.part:
        name, spec = p.split("=", 1)
        rs = []
        for r in spec.split(","):
            f, lohi = r.rsplit(":", 1)
            lo, hi = lohi.split("-")
            rs.append((f, int(lo), int(hi)))
        parts.append((name, rs))
    name, body = kernel_body(lines, a.kernel)
    counts = collections.defaultdict(collections.Counter)
    cur = ("?", 0)
    for l in body:
        s = l.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            cur = (files.get(int(m.group(1)), "?"), int(m.group(2)))
            continue
        if not s or s.startswith((".", ";", "//")) or s.endswith(":"):
            continue
        op = s.split()[0]
        if not re.match(r"^[a-z_0-9]+$", op) or not op.startswith(("v_", "s_", "global_", "flat_", "scratch_", "buffer_", "ds_")):
            continue
        where = "(elsewhere)" if parts else cur[0]
        for pname, rs in parts:
            if any(cur[0] == f and lo <= cur[1] <= hi for f, lo, hi in rs):
                where = pname
                break
        counts[where][category(op)] += 1
    print(name)
    print("%-28s" % "part" + "".join("%9s" % c for c in CATS) + "%9s" % "total")
    order = [p for p, _ in parts] + ["(elsewhere)"] if parts else sorted(counts)
    tot = collections.Counter()
    for w in order:
        c = counts.get(w, collections.Counter())
        tot.update(c)
        print("%-28s" % w + "".join("%9d" % c[k] for k in CATS) + "%9d" % sum(c.values()))
    print("%-28s" % "kernel" + "".join("%9d" % tot[k] for k in CATS) + "%9d" % sum(tot.values()))


if __name__ == "__main__":
    main()
