#!/usr/bin/env python3
"""Per-kernel comparison of two device assembly files of hip/pt_host.hip: is every kernel's instruction stream the same?

  cd amber_amd/csrc && hipcc --offload-arch=gfx950 $(CXXFLAGS of the Makefile) [-DAMBER_LAB] --offload-device-only -S hip/pt_host.hip -o new.s
  tools/isa_compare.py old.s new.s

Per kernel (a symbol of type @function) the comments, the directives and the names of the local labels are dropped -- a label becomes
its rank among the kernel's labels, so a kernel that merely moved in the file compares equal.  Prints one line per kernel, `equal`,
`DIFFERENT (n -> m instructions)` or `only in <file>`, then the totals; exit status 1 unless every kernel is in both files and equal."""
import re
import sys

LABEL = re.compile(r"\.L[A-Za-z_]*[0-9][0-9_]*")


def kernels(path):
    """{symbol: [instruction, ...]} with comments, directives and local label names removed."""
    out, name, labels = {}, None, {}
    with open(path) as f:
        for raw in f:
            line = raw.split(";", 1)[0].strip()
            if not line:
                continue
            m = re.match(r"\.type\s+(\S+),@function", line)
            if m:
                name, labels = m.group(1), {}
                out[name] = []
                continue
            if name is None:
                continue
            if line.startswith(".Lfunc_end"):
                name = None
                continue
            if line == name + ":":
                continue
            m = re.fullmatch(r"(\.L\S+):", line)
            if m:
                out[name].append("L%d:" % labels.setdefault(m.group(1), len(labels)))
                continue
            if line.startswith("."):
                continue
            out[name].append(LABEL.sub(lambda l: "L%d" % labels.setdefault(l.group(0), len(labels)), " ".join(line.split())))
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    n_equal = n_bad = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            verdict = "only in " + (sys.argv[1] if k in a else sys.argv[2])
        elif a[k] == b[k]:
            verdict = "equal"
        else:
            count = lambda body: sum(not i.endswith(":") for i in body)
            verdict = "DIFFERENT (%d -> %d instructions)" % (count(a[k]), count(b[k]))
        n_equal += verdict == "equal"
        n_bad += verdict != "equal"
        print("%-13s %s" % (verdict, k))
    print("%d kernels in %s, %d in %s: %d equal, %d not" % (len(a), sys.argv[1], len(b), sys.argv[2], n_equal, n_bad))
    return 1 if n_bad else 0


if __name__ == "__main__":
    sys.exit(main())
