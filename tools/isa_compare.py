#!/usr/bin/env python3
"""Text diff of two `make check-isa` trees (build/isa/*.s), kernel by kernel.

    python3 tools/isa_compare.py PARENT/build/isa build/isa [--rename REGEX REPL] [--only REGEX] [--table REGEX]

The method of DESIGN.md's refactor entries: both trees come from the same compiler and flags;
comments, label numbers and debug lines are stripped, and every function's body and its kernel
descriptor (registers, scratch, LDS, occupancy) are compared with the function of the same name in
the other tree, whichever file holds it.  --rename rewrites the parent's names first (a kernel
whose template parameters changed).  Reads text only; prints a table and the head of each diff.
"""
import argparse
import difflib
import glob
import os
import re
import sys

INFO = ("TotalNumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "LDSByteSize", "Occupancy")
SPILL = (".sgpr_spill_count", ".vgpr_spill_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def functions(path, rename):
    """name -> (body lines, descriptor dict) of one .s file"""
    text = open(path).read()
    for pat, repl in rename:
        text = re.sub(pat, repl, text)
    out, name, body, desc = {}, None, [], {}
    lines = text.split("\n")
    for ln in lines:
        m = re.match(r"^([A-Za-z_$][\w$.]*):\s*(;.*)?$", ln)
        if name is None:
            if m and not ln.startswith(".L") and "@" in (m.group(2) or ""):
                name, body, desc = m.group(1), [], {}
            continue
        if re.match(r"^\.Lfunc_end\d+:", ln):
            out[name] = [body, desc]
            last, name = name, None
            continue
        code = ln.split(";")[0].rstrip()
        code = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", code).strip()
        if not code or code.startswith((".loc", ".file", ".cfi", ".p2align")):
            continue
        body.append(code)
    # "; Kernel info:" comment blocks follow their function; the metadata holds the spill counts
    cur = None
    for ln in lines:
        m = re.match(r"^\s*\.amdhsa_kernel (\S+)", ln) or re.match(r"^\s*\.name:\s+(\S+)", ln)
        if m:
            cur = m.group(1)
        m = re.match(r"^([A-Za-z_$][\w$.]*):\s*; @", ln)
        if m:
            cur = m.group(1)
        m = re.match(r"^; (\w+)\s*:?\s+(\d+)", ln)
        if m and cur in out and m.group(1) in INFO:
            out[cur][1][m.group(1)] = int(m.group(2))
        m = re.match(r"^\s+(\.\w+):\s+(\d+)", ln)
        if m and cur in out and m.group(1) in SPILL:
            out[cur][1][m.group(1)] = int(m.group(2))
    return out


def tree(d, rename):
    fns = {}
    for p in sorted(glob.glob(os.path.join(d, "*.s"))):
        for k, v in functions(p, rename).items():
            fns[k] = (os.path.basename(p), v[0], v[1])
    return fns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--rename", nargs=2, action="append", default=[], metavar=("REGEX", "REPL"))
    ap.add_argument("--only", default="", help="report only functions matching this regex")
    ap.add_argument("--context", type=int, default=40, help="diff lines shown per function")
    ap.add_argument("--table", default="", help="also print a resource table of the functions matching this regex")
    a = ap.parse_args()
    old, new = tree(a.parent, a.rename), tree(a.new, [])
    keep = (lambda k: re.search(a.only, k)) if a.only else (lambda k: True)
    print(f"parent: {len(old)} functions; new: {len(new)} functions")
    print("only in parent:", sorted(k for k in old if k not in new and keep(k)))
    print("only in new:", sorted(k for k in new if k not in old and keep(k)))
    same, differ, worse = 0, [], []
    for k in sorted(old):
        if k not in new or not keep(k):
            continue
        (f0, b0, d0), (f1, b1, d1) = old[k], new[k]
        if b0 == b1 and d0 == d1:
            same += 1
            continue
        differ.append(k)
        dd = {x: (d0.get(x), d1.get(x)) for x in sorted(set(d0) | set(d1)) if d0.get(x) != d1.get(x)}
        if dd:
            worse.append(k)
        print(f"=== DIFF {k} {f0} -> {f1} {len(b0)} -> {len(b1)} lines; descriptor "
              f"{'EQUAL ' + str(d0) if not dd else 'DIFFERS ' + str(dd)}")
        for i, ln in enumerate(difflib.unified_diff(b0, b1, lineterm="", n=1)):
            if i >= a.context:
                break
            print(ln)
    print(f"compared {same + len(differ)}: identical {same}, differing {len(differ)}, "
          f"descriptor differs {len(worse)}")
    if a.table:
        # parent / new per kernel: registers, scratch, LDS, occupancy, global loads and stores
        cols = ("TotalNumSgprs", "NumVgprs", "ScratchSize", "LDSByteSize", "Occupancy")
        count = lambda b, op: sum(1 for ln in b if ln.startswith(op))  # noqa: E731
        print("\n" + "  ".join(("sgpr", "vgpr", "scratch", "lds", "occ", "gload", "gstore")) + "  kernel (parent/new)")
        for k in sorted(new):
            if not re.search(a.table, k):
                continue
            b0, d0 = (old[k][1], old[k][2]) if k in old else ([], {})
            cells = [f"{d0.get(c, '-')}/{new[k][2].get(c, '-')}" for c in cols]
            cells += [f"{count(b0, op) if k in old else '-'}/{count(new[k][1], op)}" for op in ("global_load", "global_store")]
            print("  ".join(cells) + "  " + k)
    return 1 if worse else 0


if __name__ == "__main__":
    sys.exit(main())
