#!/usr/bin/env python3
"""developer helper: static census of one kernel's gfx950 ISA by source region, from an assembly listing with line tables
(hipcc --offload-arch=gfx950 -O3 ... --cuda-device-only -S -g1).  An instruction belongs to the function whose text holds the line
its .loc names (an inlined helper counts as itself, not as its caller).
usage: tools/isa_census.py LISTING.s MANGLED_KERNEL_NAME_SUBSTRING [LISTING2.s]   (two listings: second minus first as a third column)"""
import collections
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNC = re.compile(r"^(?:__host__ )?__device__ [^(]*?(\w+)\s*\(")   # a definition starts at column 0 (its template line above it)
KINDS = [("v_cndmask", re.compile(r"^v_cndmask")), ("v_mov", re.compile(r"^v_mov_b(32|64)")),
         ("saveexec", re.compile(r"^s_(and|or|andn2|xor)_saveexec")), ("mfma", re.compile(r"^v_mfma")), ("valu", re.compile(r"^v_"))]


def regions(path):
    """[(first line, function name)] of a header, in order"""
    out = []
    for i, line in enumerate(open(path), 1):
        m = FUNC.match(line)
        if m and not line.rstrip().endswith(";"):
            out.append((i, m.group(1)))
    return out


def census(listing, kernel):
    files, table = {}, {}
    counts = collections.defaultdict(lambda: collections.Counter())
    inside, cur = False, ("?", 0)
    for line in open(listing, errors="replace"):
        s = line.strip()
        if s.startswith(".file"):
            m = re.match(r'\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', s)
            if m:
                files[int(m.group(1))] = os.path.basename(m.group(3) or m.group(2))
            continue
        if not inside:
            if s.split(";")[0].strip().endswith(":") and kernel in s and not s.startswith("."):
                inside = True
            continue
        if s.startswith(".Lfunc_end"):
            break
        if s.startswith(".loc"):
            p = s.split()
            cur = (files.get(int(p[1]), "?"), int(p[2]))
            continue
        if not s or s.startswith((".", ";")) or s.endswith(":"):
            continue
        op = s.split()[0]
        f, ln = cur
        if f not in table:
            path = os.path.join(ROOT, "opensot_amd", "csrc", f)
            table[f] = regions(path) if os.path.exists(path) else []
        name = f
        for first, fn in table[f]:
            if first <= ln:
                name = f"{f}:{fn}"
        c = counts[name]
        c["all"] += 1
        for kind, rx in KINDS:
            if rx.match(op):
                c[kind] += 1
                if kind != "valu":
                    c["valu"] += 0 if kind == "saveexec" else 1
                break
    return counts


def main():
    a = census(sys.argv[1], sys.argv[2])
    b = census(sys.argv[3], sys.argv[2]) if len(sys.argv) > 3 else None
    cols = ["all", "valu", "v_cndmask", "v_mov", "saveexec", "mfma"]
    names = sorted(set(a) | set(b or {}), key=lambda n: -(a.get(n, {}).get("all", 0)))
    print(f"{'region':58s} " + " ".join(f"{c:>10s}" for c in cols) + ("   | second listing minus first: " + " ".join(cols) if b else ""))
    tot_a, tot_d = collections.Counter(), collections.Counter()
    for n in names:
        ra = a.get(n, collections.Counter())
        row = f"{n:58s} " + " ".join(f"{ra[c]:10d}" for c in cols)
        tot_a.update(ra)
        if b:
            d = {c: b.get(n, collections.Counter())[c] - ra[c] for c in cols}
            tot_d.update(d)
            row += "   | " + " ".join(f"{d[c]:8d}" for c in cols)
        print(row)
    print(f"{'TOTAL':58s} " + " ".join(f"{tot_a[c]:10d}" for c in cols) + ("   | " + " ".join(f"{tot_d[c]:8d}" for c in cols) if b else ""))


if __name__ == "__main__":
    main()
