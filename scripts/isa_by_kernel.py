#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel, wherever a kernel lies: for a change that moves kernels between
translation units without touching them.

    python scripts/isa_by_kernel.py DIR_A DIR_B

Each directory holds, per translation unit (and per -D variant of one), NAME.s and NAME.res made with the Makefile's flags:

    hipcc $(FLAGS) [-DLZ_INST_GROUP=g | -DLZ_RS_INST=k] --cuda-device-only -S -Rpass-analysis=kernel-resource-usage \
          csrc/UNIT.hip -o DIR/NAME.s 2> DIR/NAME.res

A kernel is its text (from its label to .Lfunc_end), its .amdhsa_kernel descriptor, its .set lines and its metadata entry.
`;` comments and the __hip_cuid_* lines are dropped, and the labels that carry the function's position in its unit
(.LBB<n>_, .Lfunc_begin<n> / .Lfunc_end<n>) lose the number.  Prints a table by (unit in A, unit in B): kernels,
lines compared, differing lines, kernels whose resource remarks differ; exit status 1 if the symbol sets or any line differ."""
import collections
import glob
import os
import re
import sys


def norm(line):
    line = line.split(";", 1)[0].rstrip()
    line = re.sub(r"\.LBB\d+_", ".LBB_", line)
    return re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line).strip()


def kernels_of(path):
    """{kernel symbol: its normalised lines}"""
    out = collections.defaultdict(list)
    lines = [ln for ln in open(path).read().split("\n") if "__hip_cuid_" not in ln]
    syms = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln) for ln in lines) if m}
    cur = None
    for ln in lines:
        m = re.match(r"^(\S+):\s*(;.*)?$", ln)
        if m and m.group(1) in syms:
            cur = ("text", m.group(1))
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            cur = ("desc", m.group(1))
        if cur:
            t = norm(ln)
            if t:
                out[cur[1]].append(t)
            if (cur[0] == "text" and re.match(r"\s*\.Lfunc_end\d+:", ln)) or (cur[0] == "desc" and ".end_amdhsa_kernel" in ln):
                cur = None
    for ln in lines:
        m = re.match(r"\s*\.set\s+(\S+?)\.\w+,", ln)
        if m and m.group(1) in syms:
            out[m.group(1)].append(norm(ln))
    text = "\n".join(lines)
    at = text.find("amdhsa.kernels:")
    if at >= 0:
        for entry in re.split(r"\n  - (?=\.)", text[at:text.find("amdhsa.target", at)])[1:]:
            name = re.search(r"\.name:\s+(\S+)", entry)
            if name and name.group(1) in syms:
                out[name.group(1)] += ["META " + x.strip() for x in entry.split("\n") if x.strip()]
    return out


def resources_of(path):
    """{function: its kernel-resource-usage remarks}"""
    out, cur = collections.defaultdict(list), None
    for ln in open(path, errors="replace"):
        m = re.search(r"remark: (.*)$", ln)
        if m:
            t = m.group(1).split("[-Rpass")[0].strip()
            f = re.match(r"Function Name: (\S+)", t)
            if f:
                cur = f.group(1)
            elif cur:
                out[cur].append(t)
    return out


def collect(d):
    kernels, remarks, where = {}, {}, {}
    for p in sorted(glob.glob(os.path.join(d, "*.s"))):
        unit = os.path.basename(p)[:-2]
        for sym, body in kernels_of(p).items():
            assert sym not in kernels, ("a kernel in two units", sym, unit, where[sym])
            kernels[sym], where[sym] = body, unit
        remarks.update(resources_of(p[:-2] + ".res"))
    return kernels, remarks, where


def main():
    ak, ar, aw = collect(sys.argv[1])
    bk, br, bw = collect(sys.argv[2])
    print(f"kernel symbols: {len(ak)} and {len(bk)}; only in A {len(set(ak) - set(bk))}, only in B {len(set(bk) - set(ak))}; "
          f"without resource remarks {sum(1 for s in ak if not ar.get(s))}")
    rows, bad = collections.OrderedDict(), 0
    for sym in sorted(set(ak) & set(bk)):
        a, b = ak[sym], bk[sym]
        diff = sum(1 for x, y in zip(a, b) if x != y) + abs(len(a) - len(b))
        res = int(ar.get(sym) != br.get(sym))
        row = rows.setdefault((aw[sym], bw[sym]), [0, 0, 0, 0])
        row[0] += 1
        row[1] += len(a)
        row[2] += diff
        row[3] += res
        if diff or res:
            bad += 1
            print("DIFF", sym[:120], diff, res)
    print("%-34s | %-32s | %7s | %14s | %15s | %17s" % ("unit in A", "unit in B", "kernels", "lines compared", "differing lines",
                                                        "resources differ"))
    for (au, bu), r in list(rows.items()) + [(("total", ""), [sum(r[i] for r in rows.values()) for i in range(4)])]:
        print("%-34s | %-32s | %7d | %14d | %15d | %17d" % (au, bu, *r))
    sys.exit(1 if bad or set(ak) != set(bk) else 0)


if __name__ == "__main__":
    main()
