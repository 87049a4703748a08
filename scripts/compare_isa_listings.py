#!/usr/bin/env python3
"""Compare the kernels of two gfx950 listings (`make -C delta_graph_slam_amd/csrc build/NAME.s`), one line per kernel.

    compare_isa_listings.py PARENT.s BRANCH.s [-m 'parent kernel=branch kernel' ...]

A refactor that must not move a bit has to leave every contraction decision (a * b + c as one fma or as a multiply and an add) where it
was, and that is visible in the listing: per kernel, the multiset of floating-point instructions of every basic block must be the same in
both files.  The line also says whether the floating-point instructions come in the same order (scheduling), and gives both files'
VGPR / SGPR / scratch / LDS figures and instruction counts.  Kernels are matched by their demangled name up to the argument list; -m
pairs kernels that were renamed (concatenate listings with `cat` when kernels moved between files).  Exit status 1 when a matched kernel
differs in a block's multiset or in a resource figure, or when a kernel of PARENT has no partner."""
import argparse
import collections
import re
import subprocess
import sys

FP = re.compile(r"^v_\w*_(?:f16|f32|f64|bf16)\b")
ENDS_BLOCK = re.compile(r"^(?:s_cbranch\w*|s_branch|s_endpgm|s_setpc_b64)\b")
FIGURES = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def demangle(symbols):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(symbols), capture_output=True, text=True, check=True).stdout.split("\n")
    except (OSError, subprocess.CalledProcessError):
        out = symbols
    short = {}
    for sym, name in zip(symbols, out):
        name = re.sub(r"^void ", "", name).replace("dgs::", "")
        depth = 0
        for i, ch in enumerate(name):   # cut at the argument list: the first '(' outside template brackets
            depth += (ch == "<") - (ch == ">")
            if ch == "(" and depth == 0:
                name = name[:i]
                break
        short[sym] = name
    return short


def kernels(path):
    text = open(path).read()
    symbols = re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, flags=re.M)
    figures = {}
    for entry in re.split(r"^  - \.agpr_count:", text, flags=re.M)[1:]:
        name = re.search(r"^    \.name:\s+(\S+)", entry, flags=re.M)
        if name:
            figures[name.group(1)] = tuple(int(re.search(r"^    %s:\s+(\d+)" % re.escape(f), entry, flags=re.M).group(1)) for f in FIGURES)
    short = demangle(symbols)
    result = {}
    for sym in symbols:
        start = re.search(r"^%s:" % re.escape(sym), text, flags=re.M).end()
        blocks, order, count = [collections.Counter()], [], 0
        for line in text[start:text.index(".Lfunc_end", start)].splitlines():
            line = line.split(";")[0].strip()
            if not line:
                continue
            if line.endswith(":"):
                blocks.append(collections.Counter())
                continue
            if line.startswith("."):
                continue
            count += 1
            op = line.split()[0]
            if FP.match(op):
                blocks[-1][op] += 1
                order.append(op)
            if ENDS_BLOCK.match(op):
                blocks.append(collections.Counter())
        fp_blocks = collections.Counter(frozenset(b.items()) for b in blocks if b)
        result[short[sym]] = dict(blocks=fp_blocks, order=order, count=count, figures=figures[sym])
    return result


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("-m", "--match", action="append", default=[], metavar="PARENT=BRANCH", help="a renamed kernel, demangled names without arguments")
    args = ap.parse_args()
    old, new = kernels(args.parent), kernels(args.branch)
    renamed = dict(m.split("=", 1) for m in args.match)
    bad = False
    print("| parent kernel | branch kernel | FP blocks | FP instructions | block multisets | FP order | VGPR | SGPR | scratch | LDS | instructions |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for name, a in old.items():
        partner = renamed.get(name, name)
        b = new.get(partner)
        if b is None:
            print("| `%s` | none | | | | | | | | | |" % name)
            bad = True
            continue
        same_blocks, same_order = a["blocks"] == b["blocks"], a["order"] == b["order"]
        bad = bad or not same_blocks or a["figures"] != b["figures"]
        fig = ["%d" % x if x == y else "%d -> %d" % (x, y) for x, y in zip(a["figures"], b["figures"])]
        print("| `%s` | %s | %d | %d | %s | %s | %s | %s -> %s |" % (name, "the same" if partner == name else "`%s`" % partner, sum(a["blocks"].values()),
                                                                  len(a["order"]), "equal" if same_blocks else "DIFFER", "equal" if same_order else "differs",
                                                                  " | ".join(fig), format(a["count"], ","), format(b["count"], ",")))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
