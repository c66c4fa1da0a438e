#!/usr/bin/env python3
"""Writes the table of profiles/evaluate_record_kernel_resources.txt: every instantiation of evaluate_kernel<Variant, TEAMS,
EvalForm> in the built library, the record form next to the metrics form, read from the code
objects' metadata (profiles/tools/kernel_resources.py: what the compiler made; no device needed) -- and compares the plain, the
metrics and the stats form, kernel by kernel, with the rows of profiles/evaluate_metrics_kernel_resources.txt and
profiles/evaluate_stats_kernel_resources.txt, and evaluate_hist_kernel with profiles/evaluate_history_kernel_resources.txt
(through profiles/tools/evaluate_history_resources.py, where that tool offers the comparison).

  python profiles/tools/evaluate_record_resources.py > table.txt
"""
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from evaluate_names import rows  # noqa: E402

ROW = re.compile(r"^(\w+) +(\S+) +(\w+) +(lat|hold|) +([12]) \|((?: +-?\d+){6}) +\w* *\|((?: +-?\d+){6}) +\w* *\|")
RECORDS = (("evaluate_metrics_kernel_resources.txt", "plain", "metrics"), ("evaluate_stats_kernel_resources.txt", "metrics", "stats"))


def recorded(name, left, right):
    """the rows of an earlier record: {key: {left form / right form: (vgprs, sgprs, scratch, vgpr spills, sgpr spills, lds)}}"""
    out = {}
    with open(os.path.join(HERE, "..", name)) as f:
        for line in f:
            m = ROW.match(line)
            if m:
                task, flags, ctrl, ring, teams, p, q = m.groups()
                out[(task, flags, ctrl, ring, int(teams))] = {left: tuple(int(x) for x in p.split()), right: tuple(int(x) for x in q.split())}
    return out


def main():
    table = rows(sys.argv[1] if len(sys.argv) > 1 else None)
    cols = lambda r: (r[0], r[2], r[4], r[1], r[3], r[5])  # the records' column order
    name = lambda k: " ".join(x for x in k[:4] if x)
    print(f"{4 * len(table)} kernels ({len(table) // 2} variants x {{1, 2}} teams x {{plain, metrics, stats, record}}).")
    for file, left, right in RECORDS:
        rec = recorded(file, left, right)
        differ = [(name(k) + f" x{k[4]}", f) for k, forms in table.items() for f in (left, right) if k not in rec or cols(forms[f]) != rec[k][f]]
        print(f"{left.capitalize()} and {right} form: {2 * len(table) - len(differ)} of {2 * len(table)} kernels reproduce the VGPR, SGPR, scratch, "
              f"spill and LDS figures of profiles/{file}" + ("." if not differ else f"; {len(differ)} differ: {differ}"))
    launched = {}
    for key, forms in table.items():
        if key[4] == 2:
            one = table[key[:4] + (1,)]
            for f in ("metrics", "record"):
                launched[(key[:4], f)] = "two" if forms[f][4] <= one[f][4] else "one"
    variants = {k for k, _ in launched}
    fell = sorted(k for k in variants if launched[(k, "metrics")] == "two" and launched[(k, "record")] == "one")
    rose = sorted(k for k in variants if launched[(k, "metrics")] == "one" and launched[(k, "record")] == "two")
    one_team = [f for k, f in table.items() if k[4] == 1]
    spills_new = sorted(k for k, f in table.items() if f["record"][1] > 0 and f["metrics"][1] == 0)
    scratch_new = sorted(k for k, f in table.items() if f["record"][4] > f["metrics"][4])
    teams = lambda k: name(k) + (" (two teams)" if k[4] == 2 else " (one team)")
    print(f"One-team record forms: at most {max(f['record'][0] for f in one_team)} VGPRs (metrics: {max(f['metrics'][0] for f in one_team)}).")
    print(f"{len(spills_new)} record kernels spill VGPRs where their metrics twin does not" +
          (": " + ", ".join(teams(k) for k in spills_new) if spills_new else "") + f"; {len(scratch_new)} need more scratch than it" +
          (": " + ", ".join(teams(k) for k in scratch_new) if scratch_new else "") + ".")
    print(f"VGPRs, record - metrics: one team {min(f['record'][0] - f['metrics'][0] for f in one_team):+d} .. "
          f"{max(f['record'][0] - f['metrics'][0] for f in one_team):+d}; LDS: "
          f"{' / '.join(sorted({'%+d' % (f['record'][5] - f['metrics'][5]) for f in table.values()}))} B per block.")
    print(f"Launched above 256 tiles with one team per block: {sum(1 for (k, f), v in launched.items() if f == 'record' and v == 'one')} "
          f"variants of the record form ({sum(1 for (k, f), v in launched.items() if f == 'metrics' and v == 'one')} of the metrics form); "
          f"{len(fell)} fall from two teams to one" + (": " + ", ".join(name(k) for k in fell) if fell else "") +
          f"; {len(rose)} go the other way" + (": " + ", ".join(name(k) for k in rose) if rose else "") + ".")
    print()
    for key in sorted(table, key=lambda k: (k[0] != "Circle", k[0] != "Hover", k[0], k[1], k[2], k[3], k[4])):
        task, flags, ctrl, ring, teams_ = key
        p, m = table[key]["metrics"], table[key]["record"]
        lp = launched[(key[:4], "metrics")] if teams_ == 2 else "   "
        lm = launched[(key[:4], "record")] if teams_ == 2 else "   "
        print(f"{task:8s} {flags:5s} {ctrl:4s} {ring:4s} {teams_} | {p[0]:4d} {p[2]:4d} {p[4]:4d} {p[1]:3d} {p[3]:3d} {p[5]:7d}  {lp} | "
              f"{m[0]:4d} {m[2]:4d} {m[4]:4d} {m[1]:3d} {m[3]:3d} {m[5]:7d}  {lm} | {m[0] - p[0]:+4d} {m[4] - p[4]:+4d}")


if __name__ == "__main__":
    main()
