#!/usr/bin/env python3
"""Writes the table of profiles/evaluate_metrics_kernel_resources.txt: every instantiation of evaluate_kernel<Variant, TEAMS,
EvalForm> in the built library, plain and metrics form, the metrics form next to the plain form, read from the code objects' metadata
(profiles/tools/kernel_resources.py: what the compiler made; no device needed).

  python profiles/tools/evaluate_metrics_resources.py > table.txt
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evaluate_names as en  # noqa: E402


def rows(lib=None):
    """{(task, flags, ctrl, ring, teams): {metrics form?: (vgprs, vgpr spills, sgprs, sgpr spills, scratch, lds)}}"""
    return {key: {False: forms["plain"], True: forms["metrics"]} for key, forms in en.rows(lib).items()}


def main():
    table = rows(sys.argv[1] if len(sys.argv) > 1 else None)
    launched = {}
    for key, forms in table.items():
        if key[4] == 2:
            one = table[key[:4] + (1,)]
            for metrics in (False, True):
                launched[(key[:4], metrics)] = "two" if forms[metrics][4] <= one[metrics][4] else "one"
    n_fell = sum(1 for k in {k for k, _ in launched} if launched[(k, False)] == "two" and launched[(k, True)] == "one")
    n_one = sum(1 for (k, m), v in launched.items() if m and v == "one")
    one_team = [f for k, f in table.items() if k[4] == 1]
    spills_new = [k for k, f in table.items() if k[4] == 1 and f[True][1] > 0 and f[False][1] == 0]
    print(f"{2 * len(table)} kernels ({len(table) // 2} variants x {{1, 2}} teams x {{plain, metrics}}).")
    print(f"One-team metrics forms: at most {max(f[True][0] for f in one_team)} VGPRs (plain: {max(f[False][0] for f in one_team)}), "
          f"{len(spills_new)} spill VGPRs where the plain one-team form does not.")
    print(f"Launched above 256 tiles with one team per block: {n_one} variants of the metrics form "
          f"({sum(1 for (k, m), v in launched.items() if not m and v == 'one')} of the plain form); {n_fell} fall from two teams to one.")
    print()
    for key in sorted(table, key=lambda k: (k[0] != "Circle", k[0] != "Hover", k[0], k[1], k[2], k[3], k[4])):
        task, flags, ctrl, ring, teams = key
        p, m = table[key][False], table[key][True]
        lp = launched[(key[:4], False)] if teams == 2 else "   "
        lm = launched[(key[:4], True)] if teams == 2 else "   "
        print(f"{task:8s} {flags:5s} {ctrl:4s} {ring:4s} {teams} | {p[0]:4d} {p[2]:4d} {p[4]:4d} {p[1]:3d} {p[3]:3d} {p[5]:7d}  {lp} | "
              f"{m[0]:4d} {m[2]:4d} {m[4]:4d} {m[1]:3d} {m[3]:3d} {m[5]:7d}  {lm} | {m[0] - p[0]:+4d} {m[4] - p[4]:+4d}")


if __name__ == "__main__":
    main()
