#!/usr/bin/env python3
"""Compares the kernels of two sets of AMDGPU device-assembly files (hipcc --cuda-device-only -S, or a -save-temps .s), per kernel
symbol: (a) the instruction stream with comments, labels, directives and symbol-relative offsets stripped, (b) the kernel descriptor
(next_free_vgpr, accum_offset, next_free_sgpr, group / private segment size) and, when the compile's
-Rpass-analysis=kernel-resource-usage output is given, the spill counts.

    compare_kernels.py --old OLD.s [...] --new NEW.s [...] [--kernel REGEX] [--old-remarks LOG ...] [--new-remarks LOG ...] [--diff N]

Prints one line per kernel and a summary; --diff N adds the first N differing lines of a unified diff per differing kernel.
Exit status 1 when the two sets do not hold the same kernel symbols (after --kernel)."""
import argparse
import difflib
import re
import sys

FIELDS = ["next_free_vgpr", "accum_offset", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size"]


def kernels(paths):
    """symbol -> (instruction lines, descriptor dict)"""
    out = {}
    for path in paths:
        txt = open(path).read()
        for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)\.end_amdhsa_kernel", txt, re.M | re.S):
            sym, desc = m.group(1), m.group(2)
            start = re.search(r"^%s:.*$" % re.escape(sym), txt, re.M)
            end = txt.index(".Lfunc_end", start.end())
            ins = []
            for line in txt[start.end():end].split("\n"):
                code = line.split(";")[0].strip()
                if not code or code.endswith(":") or code.startswith(".") or code.startswith("#"):
                    continue
                code = re.sub(r"\b\S+@(rel32@lo|rel32@hi|gotpcrel32@lo|gotpcrel32@hi)\S*", "SYM", code)
                code = re.sub(r"\.LBB\d+_\d+", "L", code)
                ins.append(re.sub(r"\s+", " ", code))
            d = {f: int(re.search(r"\.amdhsa_%s\s+(\d+)" % f, desc).group(1)) for f in FIELDS}
            out[sym] = (ins, d)
    return out


def spills(paths):
    out = {}
    for path in paths or []:
        cur = None
        for line in open(path):
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                cur = out.setdefault(m.group(1), {})
            m = re.search(r"remark:\s+(SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
            if m and cur is not None:
                cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--kernel", default=".", help="regex on the kernel symbol")
    ap.add_argument("--old-remarks", nargs="*")
    ap.add_argument("--new-remarks", nargs="*")
    ap.add_argument("--diff", type=int, default=0)
    a = ap.parse_args()
    ko = {k: v for k, v in kernels(a.old).items() if re.search(a.kernel, k)}
    kn = {k: v for k, v in kernels(a.new).items() if re.search(a.kernel, k)}
    so, sn = spills(a.old_remarks), spills(a.new_remarks)
    same = worse = 0
    for sym in sorted(set(ko) & set(kn)):
        (io, do), (inn, dn) = ko[sym], kn[sym]
        do, dn = dict(do, **so.get(sym, {})), dict(dn, **sn.get(sym, {}))
        ident = io == inn
        same += ident
        changed = {f: (do[f], dn[f]) for f in do if f in dn and do[f] != dn[f]}
        w = any(n > o for o, n in changed.values())
        worse += w
        print("%s  %-9s %6d -> %6d instructions  descriptor %s%s" % (
            sym, "IDENTICAL" if ident else "DIFFERENT", len(io), len(inn), "same" if not changed else changed, "  WORSE" if w else ""))
        if not ident and a.diff:
            for ln in list(difflib.unified_diff(io, inn, "old", "new", n=1, lineterm=""))[:a.diff]:
                print("    " + ln)
    lost, added = sorted(set(ko) - set(kn)), sorted(set(kn) - set(ko))
    print("%d kernels in both, %d with identical instruction streams, %d with a worse descriptor field; lost: %s; added: %s"
          % (len(set(ko) & set(kn)), same, worse, lost or "none", added or "none"))
    return 1 if lost or added else 0


if __name__ == "__main__":
    sys.exit(main())
