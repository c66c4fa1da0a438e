#!/usr/bin/env python3
"""Writes the table of profiles/evaluate_history_record_kernel_resources.txt: every instantiation of the record form
evaluate_hist_kernel<Variant, HN, true> (csrc/pds_evaluate_hist.h) in the built library beside its twin <Variant, HN, false>, read
from the code objects' metadata (profiles/tools/kernel_resources.py: what the compiler made; no device needed) -- and compares the
twins, kernel by kernel, with the rows of profiles/evaluate_history_kernel_resources.txt, and every evaluate_kernel with the rows
of profiles/evaluate_metrics_kernel_resources.txt, profiles/evaluate_stats_kernel_resources.txt and
profiles/evaluate_record_kernel_resources.txt.

  python profiles/tools/evaluate_history_record_resources.py > table.txt
"""
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import evaluate_names as en  # noqa: E402
import evaluate_record_resources as err  # noqa: E402
import kernel_resources as kr  # noqa: E402

NAME = re.compile(r"evaluate_hist_kernel<pds::Variant<(\d), (\w+), (\w+), (\w+), (\w+), (\w+), (\d), (\w+), (\w+)>, (\d+), \(pds::EvalHistForm\)([01])>")  # (the form by value: 0 the launch without, 1 with the record; 2, the stats form, has profiles/tools/evaluate_history_stats_resources.py)
ROW = re.compile(r"^(\w+) +(\S+) +(\w+) +(\d+) \|((?: +-?\d+){6}) \|")
FORMS = err.RECORDS + (("evaluate_record_kernel_resources.txt", "metrics", "record"),)


def rows(lib=None):
    """{(task, flags, ctrl, HN): {False / True: (vgprs, vgpr spills, sgprs, sgpr spills, scratch, lds)}}"""
    out = {}
    for r in kr.kernel_table(lib):
        m = NAME.search(r[0])
        if m:
            task, motor, dr, ge, tn, on, ctrl, lat, _, hn, rec = m.groups()
            if lat == "true":  # (on the latency ring: profiles/tools/evaluate_history_latency_resources.py)
                continue
            flags = "".join(c for c, v in zip("MDGTO", (motor, dr, ge, tn, on)) if v == "true") or "-"
            out.setdefault((en.TASK[int(task)], flags, en.CTRL[int(ctrl)], int(hn)), {})[rec == "1"] = r[1:]
    return out


def recorded():
    """the evaluate_hist_kernel columns of profiles/evaluate_history_kernel_resources.txt: {key: (vgprs, sgprs, scratch, spV, spS, lds)}"""
    out = {}
    with open(os.path.join(HERE, "..", "evaluate_history_kernel_resources.txt")) as f:
        for line in f:
            m = ROW.match(line)
            if m:
                task, flags, ctrl, hn, e = m.groups()
                out[(task, flags, ctrl, int(hn))] = tuple(int(x) for x in e.split())
    return out


def main():
    lib = sys.argv[1] if len(sys.argv) > 1 else None
    table = rows(lib)
    cols = lambda r: (r[0], r[2], r[4], r[1], r[3], r[5])  # VGPRs, SGPRs, scratch, spilled VGPRs, spilled SGPRs, LDS
    rec = recorded()
    differ = [k for k, f in table.items() if k not in rec or cols(f[False]) != rec[k]]
    new = [cols(f[True]) for f in table.values()]
    print(f"{len(new)} record kernels ({len(new) // 4} variants x 4 input widths HN = 4, 6, 8, 12: d_in <= 64 / 96 / 128 / 192).")
    print(f"Without the record, evaluate_hist_kernel<Variant, HN, false>: {len(table) - len(differ)} of {len(table)} kernels reproduce the VGPR, "
          f"SGPR, scratch, spill and LDS figures of profiles/evaluate_history_kernel_resources.txt" + ("." if not differ else f"; {len(differ)} differ: {sorted(differ)}"))
    old = en.rows(lib)
    for file, left, right in FORMS:
        was = err.recorded(file, left, right)
        same = sum(1 for k, forms in old.items() if k in was and cols(forms[right]) == was[k][right])
        print(f"evaluate_kernel, {right} form: {same} of {len(old)} kernels reproduce the figures of profiles/{file}.")
    was = err.recorded(*FORMS[0])
    same = sum(1 for k, forms in old.items() if k in was and cols(forms["plain"]) == was[k]["plain"])
    print(f"evaluate_kernel, plain form: {same} of {len(old)} kernels reproduce the figures of profiles/{FORMS[0][0]}.")
    spills_new = sorted(k for k, f in table.items() if f[True][1] > 0 and f[False][1] == 0)
    scratch_new = sorted(k for k, f in table.items() if f[True][4] > f[False][4])
    name = lambda k: f"{k[0]} {k[1]} {k[2]} HN {k[3]}"
    print(f"Record kernels: VGPRs {min(c[0] for c in new)} .. {max(c[0] for c in new)}; LDS {min(c[5] for c in new)} .. {max(c[5] for c in new)} B per "
          f"block (limit 163840); scratch at most {max(c[2] for c in new)} B per lane; spilled VGPRs at most {max(c[3] for c in new)}.")
    print(f"{len(spills_new)} record kernels spill VGPRs where their twin does not" + (": " + ", ".join(name(k) for k in spills_new) if spills_new else "") +
          f"; {len(scratch_new)} need more scratch than it" + (": " + ", ".join(name(k) for k in scratch_new) if scratch_new else "") + ".")
    print(f"Record - twin: VGPRs {min(f[True][0] - f[False][0] for f in table.values()):+d} .. {max(f[True][0] - f[False][0] for f in table.values()):+d}; "
          f"spilled SGPRs {min(f[True][3] - f[False][3] for f in table.values()):+d} .. {max(f[True][3] - f[False][3] for f in table.values()):+d}; "
          f"LDS {' / '.join(sorted({'%+d' % (f[True][5] - f[False][5]) for f in table.values()}))} B per block.")
    print()
    print(f"{'task':8s}{'flags':7s}{'ctrl':6s}{'HN':>3s} |{'VGPR':>5s}{'SGPR':>5s}{'scr':>5s}{'spV':>4s}{'spS':>4s}{'LDS':>8s} |{'VGPR':>5s}{'SGPR':>5s}{'scr':>5s}{'spV':>4s}{'spS':>4s}{'LDS':>8s} | dVGPR dscr")
    for k in sorted(table):
        e, r = cols(table[k][False]), cols(table[k][True])
        print(f"{k[0]:8s}{k[1]:7s}{k[2]:6s}{k[3]:3d} |{e[0]:5d}{e[1]:5d}{e[2]:5d}{e[3]:4d}{e[4]:4d}{e[5]:8d} |{r[0]:5d}{r[1]:5d}{r[2]:5d}{r[3]:4d}{r[4]:4d}{r[5]:8d} |{r[0] - e[0]:+6d}{r[2] - e[2]:+5d}")


if __name__ == "__main__":
    main()
