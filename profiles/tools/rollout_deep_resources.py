#!/usr/bin/env python3
"""Writes the table of profiles/rollout_deep_kernel_resources.txt: every instantiation of rollout_deep_kernel<Variant, L>
(csrc/pds_rollout_deep.h) in the built library beside evaluate_deep_kernel<Variant, L> of the same variant and depth, the kernel
its network waves come from -- read from the code objects' metadata (profiles/tools/kernel_resources.py: what the compiler made;
no device needed).  With a second library, built from the commit before, EVERY code object the two share is compared figure for
figure, and what moved is listed by name.

  python profiles/tools/rollout_deep_resources.py [libpds_hip.so [library of the parent commit]] > table.txt
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as kr  # noqa: E402
from evaluate_deep_resources import LDS_LIMIT, VARIANT, _key  # noqa: E402

DEEP = re.compile(r"rollout_deep_kernel<" + VARIANT + r", (\d)>")
TWIN = re.compile(r"evaluate_deep_kernel<" + VARIANT + r", (\d)>")


def main():
    lib = sys.argv[1] if len(sys.argv) > 1 else None
    table = kr.kernel_table(lib)
    deep, twin = {}, {}
    for r in table:
        for rx, into in ((DEEP, deep), (TWIN, twin)):
            m = rx.search(r[0])
            if m:
                into[_key(m.groups()) + (int(m.group(10)),)] = r[1:]
    cols = lambda r: (r[0], r[2], r[4], r[1], r[3], r[5])  # VGPRs, SGPRs, scratch, spilled VGPRs, spilled SGPRs, LDS
    for L in (3, 4):
        rows = [cols(v) for k, v in deep.items() if k[-1] == L]
        print(f"L = {L}: {len(rows)} kernels; VGPRs {min(c[0] for c in rows)} .. {max(c[0] for c in rows)}; LDS {min(c[5] for c in rows)} .. "
              f"{max(c[5] for c in rows)} B per block (limit {LDS_LIMIT}); scratch at most {max(c[2] for c in rows)} B per lane; spilled VGPRs at "
              f"most {max(c[3] for c in rows)}; spilled SGPRs at most {max(c[4] for c in rows)}.")
    scratch = sorted(k for k, v in deep.items() if v[4] > 0)
    worse = sorted(k for k, v in deep.items() if v[1] > twin[k][1])
    name = lambda k: f"{k[0]} {k[1]} L {k[-1]}"
    print("Variants that need scratch: " + (", ".join(name(k) for k in scratch) if scratch else "none") + ".")
    print("Variants that spill VGPRs where evaluate_deep_kernel of the same variant and depth does not (withheld): " +
          (", ".join(name(k) for k in worse) if worse else "none") + ".")
    if len(sys.argv) > 2:
        old = {r[0]: r[1:] for r in kr.kernel_table(sys.argv[2])}
        mine = {r[0]: r[1:] for r in table}
        new = sorted(n for n in mine if n not in old)
        gone = sorted(n for n in old if n not in mine)
        moved = sorted(n for n in mine if n in old and old[n] != mine[n])
        print(f"All code objects: {len(mine)} here, {len(old)} in the parent commit's build; {len(new)} new"
              f" ({sum(1 for n in new if 'rollout_deep_kernel<' in n)} of them rollout_deep_kernel), {len(gone)} of the parent's missing, "
              f"{len(mine) - len(new) - len(moved)} of the {len(mine) - len(new)} shared ones with every figure of the parent's, {len(moved)} moved.")
        for n in moved:
            print(f"  moved: {n}: {old[n]} -> {mine[n]}")
        for n in gone:
            print(f"  missing: {n}")
    print()
    print(f"{'task':8s}{'flags':7s}{'L':>2s} |{'VGPR':>5s}{'SGPR':>5s}{'scr':>5s}{'spV':>4s}{'spS':>4s}{'LDS':>8s} |{'VGPR':>5s}{'SGPR':>5s}{'scr':>5s}{'spV':>4s}{'spS':>4s}{'LDS':>8s} | dVGPR    dLDS")
    for k in sorted(deep):
        d, t = cols(deep[k]), cols(twin[k])
        print(f"{k[0]:8s}{k[1]:7s}{k[-1]:2d} |{d[0]:5d}{d[1]:5d}{d[2]:5d}{d[3]:4d}{d[4]:4d}{d[5]:8d} |{t[0]:5d}{t[1]:5d}{t[2]:5d}{t[3]:4d}{t[4]:4d}{t[5]:8d} |"
              f"{d[0] - t[0]:+6d}{d[5] - t[5]:+8d}")


if __name__ == "__main__":
    main()
