"""Compare the device assembly of two builds of csrc/rt_kernel.hip kernel by kernel.

Each input is the output of the library's compile line (csrc/Makefile HIPFLAGS,
plus the variant's -D flags) with `--cuda-device-only -S`.  Every function
symbol's text from its label to its .size line -- for a kernel that encloses its
.amdhsa_kernel descriptor block -- is compared line by line after the numbers in
block labels (.LBB<f>_<b>, .Lfunc_end<f>, .LJTI<f>_<t>) are replaced by their
order of appearance inside the function: the function number in them follows the
order of emission, which follows the order of the host's references.

    python profiles/trace_host/compare_asm.py parent.s head.s

Prints one summary line; exit status 1 when a symbol or a line differs.
"""
import re
import sys

LABEL = re.compile(r"\.L(BB|JTI|func_begin|func_end|tmp)(\d+)(_\d+)?")


def functions(path):
    """{symbol: [lines]}: a function from its label to its .size line, which for a
    kernel encloses the .amdhsa_kernel block; and the set of kernel symbols."""
    lines = open(path).read().splitlines()
    syms = {m.group(1) for ln in lines for m in [re.match(r"\s*\.type\s+(\S+),@function", ln)] if m}
    bodies, kernels, cur, name = {}, set(), None, None
    for ln in lines:
        s = ln.strip()
        if cur is None:
            m = re.match(r"(\S+):", s)
            if m and m.group(1) in syms and m.group(1) not in bodies:
                name, cur = m.group(1), bodies.setdefault(m.group(1), [])
            continue
        cur.append(s)
        if s.startswith(".amdhsa_kernel "):
            assert s.split()[1] == name, (s, name)
            kernels.add(name)
        if re.match(r"\.size\s+" + re.escape(name) + ",", s):
            cur = None
    assert cur is None, name
    return bodies, kernels


def normalised(body):
    order = {}

    def sub(m):
        key = (m.group(1), m.group(2))
        return ".L%s#%d%s" % (m.group(1), order.setdefault(key, len(order)), m.group(3) or "")

    return [LABEL.sub(sub, ln) for ln in body]


def main(a, b):
    (ba, ka), (bb, kb) = functions(a), functions(b)
    bad = sorted((set(ba) ^ set(bb)) | (ka ^ kb))
    for s in bad:
        print("only in one build:", s)
    compared = differing = 0
    for s in sorted(set(ba) & set(bb)):
        x, y = normalised(ba[s]), normalised(bb[s])
        compared += len(x)
        d = sum(1 for p, q in zip(x, y) if p != q) + abs(len(x) - len(y))
        if d:
            print("differs:", s, d, "lines")
        differing += d
    print("%d kernels of %d functions, %d lines compared, %d differing, %d symbols unmatched"
          % (len(ka), len(ba), compared, differing, len(bad)))
    return 1 if differing or bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
