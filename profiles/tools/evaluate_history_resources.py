#!/usr/bin/env python3
"""Writes the table of profiles/evaluate_history_kernel_resources.txt: every instantiation of evaluate_hist_kernel<Variant, HN>
(csrc/pds_evaluate_hist.h) in the built library beside the rollout_hist_kernel<Variant, HN> of the same variant and width, and every
evaluate_kernel against the rows of profiles/evaluate_metrics_kernel_resources.txt -- read from the code objects' metadata
(profiles/tools/kernel_resources.py: what the compiler made; no device needed).

  python profiles/tools/evaluate_history_resources.py > table.txt
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evaluate_stats_resources as esr  # noqa: E402
import kernel_resources as kr  # noqa: E402

# (evaluate_hist_kernel<Variant, HN, F>: the launch of this table is F = EvalHistForm::Metrics, 0 by value -- REC = false before the
# kernel had three forms; the record and the stats form have tables of their own -- profiles/tools/evaluate_history_record_resources.py,
# profiles/tools/evaluate_history_stats_resources.py)
NAME = re.compile(r"(evaluate_hist_kernel|rollout_hist_kernel)<pds::Variant<(\d), (\w+), (\w+), (\w+), (\w+), (\w+), (\d), (\w+), (\w+)>, (\d+)(?:, false|, \(pds::EvalHistForm\)0)?>")


def rows(lib=None):
    """{(task, flags, ctrl, HN): {"evaluate" / "rollout": (vgprs, vgpr spills, sgprs, sgpr spills, scratch, lds)}}"""
    out = {}
    for r in kr.kernel_table(lib):
        m = NAME.search(r[0])
        if not m:
            continue
        kernel, task, motor, dr, ge, tn, on, ctrl, _, _, hn = m.groups()
        flags = "".join(c for c, v in zip("MDGTO", (motor, dr, ge, tn, on)) if v == "true") or "-"
        out.setdefault((esr.TASK[int(task)], flags, esr.CTRL[int(ctrl)], int(hn)), {})["evaluate" if kernel.startswith("evaluate") else "rollout"] = r[1:]
    return out


def main():
    lib = sys.argv[1] if len(sys.argv) > 1 else None
    table = rows(lib)
    cols = lambda r: (r[0], r[2], r[4], r[1], r[3], r[5])  # VGPRs, SGPRs, scratch, spilled VGPRs, spilled SGPRs, LDS
    ev = [cols(f["evaluate"]) for f in table.values()]
    spilling = sorted(k for k, f in table.items() if f["evaluate"][1] > 0 or f["evaluate"][4] > 0)
    print(f"{len(ev)} kernels ({len(ev) // 4} variants x 4 input widths HN = 4, 6, 8, 12: d_in <= 64 / 96 / 128 / 192).")
    print(f"VGPRs {min(c[0] for c in ev)} .. {max(c[0] for c in ev)}; LDS {min(c[5] for c in ev)} .. {max(c[5] for c in ev)} B per block (limit 163840); "
          f"scratch at most {max(c[2] for c in ev)} B per lane; spilled VGPRs at most {max(c[3] for c in ev)}.")
    print("Variants with spilled VGPRs or scratch: " + (", ".join(f"{k[0]} {k[1]} {k[2]} HN {k[3]}" for k in spilling) if spilling else "none") + ".")
    old = esr.rows(lib)
    rec = esr.recorded()
    same = sum(1 for k, forms in old.items() for f in ("plain", "metrics") if k in rec and cols(forms[f]) == rec[k][f])
    total = sum(1 for k, forms in old.items() for f in ("plain", "metrics"))
    print(f"evaluate_kernel, plain and metrics form: {same} of {total} kernels reproduce the figures of profiles/evaluate_metrics_kernel_resources.txt.")
    print()
    print(f"{'task':8s}{'flags':7s}{'ctrl':6s}{'HN':>3s} |{'VGPR':>5s}{'SGPR':>5s}{'scr':>5s}{'spV':>4s}{'spS':>4s}{'LDS':>8s} |{'VGPR':>5s}{'SGPR':>5s}{'scr':>5s}{'spV':>4s}{'spS':>4s}{'LDS':>8s}")
    for k in sorted(table):
        e, r = cols(table[k]["evaluate"]), cols(table[k].get("rollout", (0,) * 6))
        print(f"{k[0]:8s}{k[1]:7s}{k[2]:6s}{k[3]:3d} |{e[0]:5d}{e[1]:5d}{e[2]:5d}{e[3]:4d}{e[4]:4d}{e[5]:8d} |{r[0]:5d}{r[1]:5d}{r[2]:5d}{r[3]:4d}{r[4]:4d}{r[5]:8d}")


if __name__ == "__main__":
    main()
