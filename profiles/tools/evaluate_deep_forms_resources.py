#!/usr/bin/env python3
"""Writes the table of profiles/evaluate_deep_forms_kernel_resources.txt: every instantiation of the stats and the record form of
evaluate_deep_kernel<Variant, L, F> (csrc/pds_evaluate_deep.h) in the built library beside its metrics twin
evaluate_deep_kernel<Variant, L, EvalForm::Metrics> -- read from the code objects' metadata (profiles/tools/kernel_resources.py:
what the compiler made; no device needed).  With profiles/evaluate_deep_kernel_resources.txt as second argument the metrics form's
figures are compared with the rows of that table (the commit before), and with a library built from the commit before as third
every evaluate_kernel and evaluate_hist_kernel of the two libraries figure for figure.

  python profiles/tools/evaluate_deep_forms_resources.py [libpds_hip.so [evaluate_deep_kernel_resources.txt [parent library]]] > table.txt
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as kr  # noqa: E402
from evaluate_deep_resources import LDS_LIMIT, VARIANT, _key  # noqa: E402

DEEP = re.compile(r"evaluate_deep_kernel<" + VARIANT + r", (\d), \(pds::EvalForm\)(\d)>")
FORM = {1: "metrics", 2: "stats", 3: "record"}


def main():
    table = kr.kernel_table(sys.argv[1] if len(sys.argv) > 1 else None)
    deep = {}
    for r in table:
        m = DEEP.search(r[0])
        if m:
            deep[_key(m.groups()) + (int(m.group(10)), FORM[int(m.group(11))])] = r[1:]
    cols = lambda r: (r[0], r[2], r[4], r[1], r[3], r[5])  # VGPRs, SGPRs, scratch, spilled VGPRs, spilled SGPRs, LDS
    name = lambda k: f"{k[0]} {k[1]} L {k[-2]} {k[-1]}"
    for form in ("stats", "record"):
        for L in (3, 4):
            rows = [cols(v) for k, v in deep.items() if k[-2] == L and k[-1] == form]
            print(f"{form} L = {L}: {len(rows)} kernels; VGPRs {min(c[0] for c in rows)} .. {max(c[0] for c in rows)}; LDS {min(c[5] for c in rows)} .. "
                  f"{max(c[5] for c in rows)} B per block (limit {LDS_LIMIT}); scratch at most {max(c[2] for c in rows)} B per lane; spilled "
                  f"VGPRs at most {max(c[3] for c in rows)}; spilled SGPRs at most {max(c[4] for c in rows)}.")
    forms = sorted(k for k in deep if k[-1] != "metrics")
    worse = [k for k in forms if deep[k][1] > deep[k[:-1] + ("metrics",)][1]]
    scratch = [k for k in forms if deep[k][4] > 0]
    print("Variants that need scratch: " + (", ".join(name(k) for k in scratch) if scratch else "none") + ".")
    print("Variants that spill VGPRs where their metrics twin does not (not to be launched): " + (", ".join(name(k) for k in worse) if worse else "none") + ".")
    if len(sys.argv) > 2:  # the metrics form against the table of the commit before
        row = re.compile(r"^(\w+)\s+(\S+)\s+(\d) \|\s*(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+) \|")
        old = {}
        for line in open(sys.argv[2]):
            m = row.match(line)
            if m:
                old[(m.group(1), m.group(2), int(m.group(3)))] = tuple(int(x) for x in m.groups()[3:])
        mine = {(k[0], k[1], k[-2]): cols(v) for k, v in deep.items() if k[-1] == "metrics"}
        same = sum(1 for k, v in mine.items() if old.get(k) == v)
        print(f"evaluate_deep_kernel, metrics form: {len(mine)} code objects, {same} with every figure of {os.path.basename(sys.argv[2])} ({len(old)} rows).")
    if len(sys.argv) > 3:
        old = {r[0]: r[1:] for r in kr.kernel_table(sys.argv[3])}
        for kernel in ("evaluate_kernel<", "evaluate_hist_kernel<"):
            mine = {r[0]: r[1:] for r in table if kernel in r[0]}
            same = sum(1 for n, v in mine.items() if old.get(n) == v)
            print(f"{kernel[:-1]}: {len(mine)} code objects, {same} with every figure of the parent commit's build.")
    print()
    print(f"{'task':8s}{'flags':7s}{'L':>2s} {'form':7s}|{'VGPR':>5s}{'SGPR':>5s}{'scr':>5s}{'spV':>4s}{'spS':>4s}{'LDS':>8s} |{'VGPR':>5s}{'SGPR':>5s}{'scr':>5s}{'spV':>4s}{'spS':>4s}{'LDS':>8s} | dVGPR    dLDS")
    for k in forms:
        d, t = cols(deep[k]), cols(deep[k[:-1] + ("metrics",)])
        print(f"{k[0]:8s}{k[1]:7s}{k[-2]:2d} {k[-1]:7s}|{d[0]:5d}{d[1]:5d}{d[2]:5d}{d[3]:4d}{d[4]:4d}{d[5]:8d} |{t[0]:5d}{t[1]:5d}{t[2]:5d}{t[3]:4d}{t[4]:4d}{t[5]:8d} |"
              f"{d[0] - t[0]:+6d}{d[5] - t[5]:+8d}")


if __name__ == "__main__":
    main()
