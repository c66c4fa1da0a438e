#!/usr/bin/env python3
"""Writes the table of profiles/evaluate_deep_kernel_resources.txt: every instantiation of evaluate_deep_kernel<Variant, L>
(csrc/pds_evaluate_deep.h) in the built library beside its twin with two hidden layers, the one-team metrics form
evaluate_kernel<Variant, 1, EvalForm::Metrics> of the same variant -- read from the code objects' metadata
(profiles/tools/kernel_resources.py: what the compiler made; no device needed).  With a second library, built from the commit
before, every evaluate_kernel and evaluate_hist_kernel of the two is compared figure for figure.

  python profiles/tools/evaluate_deep_resources.py [libpds_hip.so [library of the parent commit]] > table.txt
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as kr  # noqa: E402

TASK = {0: "Hover", 1: "Circle", 2: "TakeOff"}
VARIANT = r"pds::Variant<(\d), (\w+), (\w+), (\w+), (\w+), (\w+), (\d), (\w+), (\w+)>"
DEEP = re.compile(r"evaluate_deep_kernel<" + VARIANT + r", (\d)(?:, \(pds::EvalForm\)1)?>")  # (the plain / metrics form)
TWIN = re.compile(r"evaluate_kernel<" + VARIANT + r", 1, \(pds::EvalForm\)1>")
LDS_LIMIT = 160 * 1024


def _key(groups):
    task, motor, dr, ge, tn, on, ctrl, lat, hold = groups[:9]
    flags = "".join(c for c, v in zip("MDGTO", (motor, dr, ge, tn, on)) if v == "true") or "-"
    return TASK[int(task)], flags, int(ctrl), lat == "true", hold == "true"


def main():
    lib = sys.argv[1] if len(sys.argv) > 1 else None
    table = kr.kernel_table(lib)
    deep, twin = {}, {}
    for r in table:
        m = DEEP.search(r[0])
        if m:
            deep[_key(m.groups()) + (int(m.group(10)),)] = r[1:]
        m = TWIN.search(r[0])
        if m:
            twin[_key(m.groups())] = r[1:]
    cols = lambda r: (r[0], r[2], r[4], r[1], r[3], r[5])  # VGPRs, SGPRs, scratch, spilled VGPRs, spilled SGPRs, LDS
    for L in (3, 4):
        rows = [cols(v) for k, v in deep.items() if k[-1] == L]
        print(f"L = {L}: {len(rows)} kernels; VGPRs {min(c[0] for c in rows)} .. {max(c[0] for c in rows)}; LDS {min(c[5] for c in rows)} .. "
              f"{max(c[5] for c in rows)} B per block (limit {LDS_LIMIT}); scratch at most {max(c[2] for c in rows)} B per lane; spilled VGPRs at "
              f"most {max(c[3] for c in rows)}; spilled SGPRs at most {max(c[4] for c in rows)}.")
    scratch = sorted(k for k, v in deep.items() if v[4] > 0)
    worse = sorted(k for k, v in deep.items() if v[1] > twin[k[:-1]][1])
    name = lambda k: f"{k[0]} {k[1]} L {k[-1]}"
    print("Variants that need scratch: " + (", ".join(name(k) for k in scratch) if scratch else "none") + ".")
    print("Variants that spill VGPRs where their two-hidden-layer one-team twin does not (not to be launched): " +
          (", ".join(name(k) for k in worse) if worse else "none") + ".")
    if len(sys.argv) > 2:
        old = {r[0]: r[1:] for r in kr.kernel_table(sys.argv[2])}
        for kernel in ("evaluate_kernel<", "evaluate_hist_kernel<"):
            mine = {r[0]: r[1:] for r in table if kernel in r[0]}
            same = sum(1 for n, v in mine.items() if old.get(n) == v)
            gone = sorted(n for n in old if kernel in n and n not in mine)
            print(f"{kernel[:-1]}: {len(mine)} code objects, {same} with every figure of the parent commit's build"
                  + (f"; {len(gone)} of the parent's are missing" if gone else "") + ".")
    print()
    print(f"{'task':8s}{'flags':7s}{'L':>2s} |{'VGPR':>5s}{'SGPR':>5s}{'scr':>5s}{'spV':>4s}{'spS':>4s}{'LDS':>8s} |{'VGPR':>5s}{'SGPR':>5s}{'scr':>5s}{'spV':>4s}{'spS':>4s}{'LDS':>8s} | dVGPR    dLDS")
    for k in sorted(deep):
        d, t = cols(deep[k]), cols(twin[k[:-1]])
        print(f"{k[0]:8s}{k[1]:7s}{k[-1]:2d} |{d[0]:5d}{d[1]:5d}{d[2]:5d}{d[3]:4d}{d[4]:4d}{d[5]:8d} |{t[0]:5d}{t[1]:5d}{t[2]:5d}{t[3]:4d}{t[4]:4d}{t[5]:8d} |"
              f"{d[0] - t[0]:+6d}{d[5] - t[5]:+8d}")


if __name__ == "__main__":
    main()
