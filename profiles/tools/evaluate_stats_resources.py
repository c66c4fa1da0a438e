#!/usr/bin/env python3
"""Writes the table of profiles/evaluate_stats_kernel_resources.txt: every instantiation of evaluate_kernel<Variant, TEAMS,
EvalForm> in the built library, the stats form next to the metrics form, read from the code objects'
metadata (profiles/tools/kernel_resources.py: what the compiler made; no device needed) -- and compares the plain and the metrics
form, kernel by kernel, with the rows of profiles/evaluate_metrics_kernel_resources.txt.

  python profiles/tools/evaluate_stats_resources.py > table.txt
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from evaluate_names import CTRL, TASK, rows  # noqa: E402,F401  (profiles/tools/evaluate_history_resources.py reads them here)

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "evaluate_metrics_kernel_resources.txt")
ROW = re.compile(r"^(\w+) +(\S+) +(\w+) +(lat|hold|) +([12]) \|((?: +-?\d+){6}) +\w* *\|((?: +-?\d+){6}) +\w* *\|")


def recorded():
    """the rows of the metrics record: {key: {"plain" / "metrics": (vgprs, sgprs, scratch, vgpr spills, sgpr spills, lds)}}"""
    out = {}
    with open(RECORD) as f:
        for line in f:
            m = ROW.match(line)
            if m:
                task, flags, ctrl, ring, teams, p, q = m.groups()
                out[(task, flags, ctrl, ring, int(teams))] = {"plain": tuple(int(x) for x in p.split()), "metrics": tuple(int(x) for x in q.split())}
    return out


def main():
    table = rows(sys.argv[1] if len(sys.argv) > 1 else None)
    cols = lambda r: (r[0], r[2], r[4], r[1], r[3], r[5])  # the record's column order
    rec = recorded()
    same = sum(1 for k, forms in table.items() for f in ("plain", "metrics") if k in rec and cols(forms[f]) == rec[k][f])
    differ = [(k, f) for k, forms in table.items() for f in ("plain", "metrics") if k not in rec or cols(forms[f]) != rec[k][f]]
    launched = {}
    for key, forms in table.items():
        if key[4] == 2:
            one = table[key[:4] + (1,)]
            for f in ("metrics", "stats"):
                launched[(key[:4], f)] = "two" if forms[f][4] <= one[f][4] else "one"
    variants = {k for k, _ in launched}
    fell = sorted(k for k in variants if launched[(k, "metrics")] == "two" and launched[(k, "stats")] == "one")
    rose = sorted(k for k in variants if launched[(k, "metrics")] == "one" and launched[(k, "stats")] == "two")
    one_team = [f for k, f in table.items() if k[4] == 1]
    spills_new = sorted(k for k, f in table.items() if k[4] == 1 and f["stats"][1] > 0 and f["metrics"][1] == 0)
    scratch_new = sorted(k for k, f in table.items() if k[4] == 1 and f["stats"][4] > f["metrics"][4])
    name = lambda k: " ".join(x for x in k[:4] if x)
    print(f"{3 * len(table)} kernels ({len(table) // 2} variants x {{1, 2}} teams x {{plain, metrics, stats}}).")
    print(f"Plain and metrics form: {same} of {2 * len(table)} kernels reproduce the VGPR, SGPR, scratch, spill and LDS figures of "
          f"profiles/evaluate_metrics_kernel_resources.txt" + ("." if not differ else f"; {len(differ)} differ: {differ}"))
    print(f"One-team stats forms: at most {max(f['stats'][0] for f in one_team)} VGPRs (metrics: {max(f['metrics'][0] for f in one_team)}); "
          f"{len(spills_new)} spill VGPRs where the one-team metrics form does not" + (": " + ", ".join(name(k) for k in spills_new) if spills_new else "") + "; "
          f"{len(scratch_new)} need more scratch than it" + (": " + ", ".join(name(k) for k in scratch_new) if scratch_new else "") + ".")
    print(f"VGPRs, stats - metrics: one team {min(f['stats'][0] - f['metrics'][0] for f in one_team):+d} .. "
          f"{max(f['stats'][0] - f['metrics'][0] for f in one_team):+d}; LDS: "
          f"{' / '.join(sorted({'%+d' % (f['stats'][5] - f['metrics'][5]) for f in table.values()}))} B per block.")
    print(f"Launched above 256 tiles with one team per block: {sum(1 for (k, f), v in launched.items() if f == 'stats' and v == 'one')} "
          f"variants of the stats form ({sum(1 for (k, f), v in launched.items() if f == 'metrics' and v == 'one')} of the metrics form); "
          f"{len(fell)} fall from two teams to one" + (": " + ", ".join(name(k) for k in fell) if fell else "") +
          f"; {len(rose)} go the other way" + (": " + ", ".join(name(k) for k in rose) if rose else "") + ".")
    print()
    for key in sorted(table, key=lambda k: (k[0] != "Circle", k[0] != "Hover", k[0], k[1], k[2], k[3], k[4])):
        task, flags, ctrl, ring, teams = key
        p, m = table[key]["metrics"], table[key]["stats"]
        lp = launched[(key[:4], "metrics")] if teams == 2 else "   "
        lm = launched[(key[:4], "stats")] if teams == 2 else "   "
        print(f"{task:8s} {flags:5s} {ctrl:4s} {ring:4s} {teams} | {p[0]:4d} {p[2]:4d} {p[4]:4d} {p[1]:3d} {p[3]:3d} {p[5]:7d}  {lp} | "
              f"{m[0]:4d} {m[2]:4d} {m[4]:4d} {m[1]:3d} {m[3]:3d} {m[5]:7d}  {lm} | {m[0] - p[0]:+4d} {m[4] - p[4]:+4d}")


if __name__ == "__main__":
    main()
