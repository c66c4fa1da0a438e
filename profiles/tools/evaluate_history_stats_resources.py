#!/usr/bin/env python3
"""Writes the table of profiles/evaluate_history_stats_kernel_resources.txt: every instantiation of the stats form
evaluate_hist_kernel<Variant, HN, EvalHistForm::Stats> (csrc/pds_evaluate_hist.h) in the built library beside its metrics twin
<Variant, HN, EvalHistForm::Metrics>, read from the code objects' metadata (profiles/tools/kernel_resources.py: what the compiler
made; no device needed) -- and compares the twins and the record forms, kernel by kernel, with the rows of
profiles/evaluate_history_record_kernel_resources.txt, and every evaluate_kernel with the rows of
profiles/evaluate_metrics_kernel_resources.txt, profiles/evaluate_stats_kernel_resources.txt and
profiles/evaluate_record_kernel_resources.txt.

  python profiles/tools/evaluate_history_stats_resources.py > table.txt
"""
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import evaluate_history_record_resources as ehr  # noqa: E402
import evaluate_names as en  # noqa: E402
import evaluate_record_resources as err  # noqa: E402
import kernel_resources as kr  # noqa: E402

NAME = re.compile(r"evaluate_hist_kernel<pds::Variant<(\d), (\w+), (\w+), (\w+), (\w+), (\w+), (\d), (\w+), (\w+)>, (\d+), \(pds::EvalHistForm\)(\d)>")
ROW = re.compile(r"^(\w+) +(\S+) +(\w+) +(\d+) \|((?: +-?\d+){6}) \|((?: +-?\d+){6}) \|")
FORM = ("metrics", "record", "stats")  # EvalHistForm 0 .. 2


def rows(lib=None):
    """{(task, flags, ctrl, HN): {"metrics" / "record" / "stats": (vgprs, vgpr spills, sgprs, sgpr spills, scratch, lds)}}"""
    out = {}
    for r in kr.kernel_table(lib):
        m = NAME.search(r[0])
        if m:
            task, motor, dr, ge, tn, on, ctrl, lat, _, hn, form = m.groups()
            if lat == "true":  # (on the latency ring: profiles/tools/evaluate_history_latency_resources.py)
                continue
            flags = "".join(c for c, v in zip("MDGTO", (motor, dr, ge, tn, on)) if v == "true") or "-"
            out.setdefault((en.TASK[int(task)], flags, en.CTRL[int(ctrl)], int(hn)), {})[FORM[int(form)]] = r[1:]
    return out


def recorded():
    """both columns of profiles/evaluate_history_record_kernel_resources.txt: {key: {"metrics" / "record": (vgprs, sgprs, scratch, spV, spS, lds)}}"""
    out = {}
    with open(os.path.join(HERE, "..", "evaluate_history_record_kernel_resources.txt")) as f:
        for line in f:
            m = ROW.match(line)
            if m:
                task, flags, ctrl, hn, e, r = m.groups()
                out[(task, flags, ctrl, int(hn))] = {"metrics": tuple(int(x) for x in e.split()), "record": tuple(int(x) for x in r.split())}
    return out


def main():
    lib = sys.argv[1] if len(sys.argv) > 1 else None
    table = rows(lib)
    cols = lambda r: (r[0], r[2], r[4], r[1], r[3], r[5])  # VGPRs, SGPRs, scratch, spilled VGPRs, spilled SGPRs, LDS
    was = recorded()
    built = {k: f for k, f in table.items() if "stats" in f}
    new = [cols(f["stats"]) for f in built.values()]
    widths = sorted({k[3] for k in built})
    print(f"{len(new)} stats kernels ({len(new) // max(len(widths), 1)} variants x {len(widths)} input widths HN = {', '.join(map(str, widths))}; of HN = 4, 6, 8, 12: d_in <= 64 / 96 / 128 / 192).")
    for form, label in (("metrics", "Without the sums, evaluate_hist_kernel<Variant, HN, Metrics>"), ("record", "The record form, evaluate_hist_kernel<Variant, HN, Record>")):
        differ = sorted(k for k, f in table.items() if k not in was or cols(f[form]) != was[k][form])
        print(f"{label}: {len(table) - len(differ)} of {len(table)} kernels reproduce the VGPR, SGPR, scratch, spill and LDS figures of "
              f"profiles/evaluate_history_record_kernel_resources.txt" + ("." if not differ else f"; {len(differ)} differ: {differ}"))
    old = en.rows(lib)
    for file, left, right in ehr.FORMS:
        rec = err.recorded(file, left, right)
        same = sum(1 for k, forms in old.items() if k in rec and cols(forms[right]) == rec[k][right])
        print(f"evaluate_kernel, {right} form: {same} of {len(old)} kernels reproduce the figures of profiles/{file}.")
    rec = err.recorded(*ehr.FORMS[0])
    same = sum(1 for k, forms in old.items() if k in rec and cols(forms["plain"]) == rec[k]["plain"])
    print(f"evaluate_kernel, plain form: {same} of {len(old)} kernels reproduce the figures of profiles/{ehr.FORMS[0][0]}.")
    name = lambda k: f"{k[0]} {k[1]} {k[2]} HN {k[3]}"
    spills_new = sorted(k for k, f in built.items() if f["stats"][1] > 0)
    scratch_new = sorted(k for k, f in built.items() if f["stats"][4] > f["metrics"][4])
    print(f"Stats kernels: VGPRs {min(c[0] for c in new)} .. {max(c[0] for c in new)}; LDS {min(c[5] for c in new)} .. {max(c[5] for c in new)} B per "
          f"block (limit 163840); scratch at most {max(c[2] for c in new)} B per lane; spilled VGPRs at most {max(c[3] for c in new)}.")
    print(f"{len(spills_new)} stats kernels spill VGPRs" + (": " + ", ".join(name(k) for k in spills_new) if spills_new else "") +
          f"; {len(scratch_new)} need more scratch than their twin" + (": " + ", ".join(name(k) for k in scratch_new) if scratch_new else "") + ".")
    for hn in widths:
        f = [v for k, v in built.items() if k[3] == hn]
        print(f"HN {hn:2d}: stats - twin: VGPRs {min(v['stats'][0] - v['metrics'][0] for v in f):+d} .. {max(v['stats'][0] - v['metrics'][0] for v in f):+d}; "
              f"spilled SGPRs {min(v['stats'][3] - v['metrics'][3] for v in f):+d} .. {max(v['stats'][3] - v['metrics'][3] for v in f):+d}; "
              f"LDS {' / '.join(sorted({'%+d' % (v['stats'][5] - v['metrics'][5]) for v in f}))} B per block.")
    print()
    print(f"{'task':8s}{'flags':7s}{'ctrl':6s}{'HN':>3s} |{'VGPR':>5s}{'SGPR':>5s}{'scr':>5s}{'spV':>4s}{'spS':>4s}{'LDS':>8s} |{'VGPR':>5s}{'SGPR':>5s}{'scr':>5s}{'spV':>4s}{'spS':>4s}{'LDS':>8s} | dVGPR dscr")
    for k in sorted(built):
        e, r = cols(built[k]["metrics"]), cols(built[k]["stats"])
        print(f"{k[0]:8s}{k[1]:7s}{k[2]:6s}{k[3]:3d} |{e[0]:5d}{e[1]:5d}{e[2]:5d}{e[3]:4d}{e[4]:4d}{e[5]:8d} |{r[0]:5d}{r[1]:5d}{r[2]:5d}{r[3]:4d}{r[4]:4d}{r[5]:8d} |{r[0] - e[0]:+6d}{r[2] - e[2]:+5d}")


if __name__ == "__main__":
    main()
