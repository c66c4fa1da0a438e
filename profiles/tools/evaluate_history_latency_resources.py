#!/usr/bin/env python3
"""Writes the table of profiles/evaluate_history_latency_kernel_resources.txt: every instantiation of evaluate_hist_kernel on the
latency ring -- <Variant<.., LAT = true, ..>, HN, F> for the three EvalHistForms (csrc/pds_evaluate_hist.h) -- in the built library
beside its twin without the ring <Variant<.., LAT = false, ..>, HN, F>, read from the code objects' metadata
(profiles/tools/kernel_resources.py: what the compiler made; no device needed) -- and compares the kernels without the ring, kernel
by kernel, with the rows of profiles/evaluate_history_record_kernel_resources.txt (metrics and record form) and
profiles/evaluate_history_stats_kernel_resources.txt (stats form).

  python profiles/tools/evaluate_history_latency_resources.py > table.txt
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import evaluate_history_stats_resources as ehs  # noqa: E402
import evaluate_names as en  # noqa: E402
import kernel_resources as kr  # noqa: E402


def rows(lib=None):
    """{LAT: {(task, flags, ctrl, HN): {"metrics" / "record" / "stats": (vgprs, vgpr spills, sgprs, sgpr spills, scratch, lds)}}}"""
    out = {False: {}, True: {}}
    for r in kr.kernel_table(lib):
        m = ehs.NAME.search(r[0])
        if m:
            task, motor, dr, ge, tn, on, ctrl, lat, _, hn, form = m.groups()
            flags = "".join(c for c, v in zip("MDGTO", (motor, dr, ge, tn, on)) if v == "true") or "-"
            out[lat == "true"].setdefault((en.TASK[int(task)], flags, en.CTRL[int(ctrl)], int(hn)), {})[ehs.FORM[int(form)]] = r[1:]
    return out


def recorded_stats():
    """the stats column of profiles/evaluate_history_stats_kernel_resources.txt: {key: (vgprs, sgprs, scratch, spV, spS, lds)}"""
    out = {}
    with open(os.path.join(HERE, "..", "evaluate_history_stats_kernel_resources.txt")) as f:
        for line in f:
            m = ehs.ROW.match(line)
            if m:
                task, flags, ctrl, hn, _, r = m.groups()
                out[(task, flags, ctrl, int(hn))] = tuple(int(x) for x in r.split())
    return out


def main():
    lib = sys.argv[1] if len(sys.argv) > 1 else None
    table = rows(lib)
    plain, ring = table[False], table[True]
    cols = lambda r: (r[0], r[2], r[4], r[1], r[3], r[5])  # VGPRs, SGPRs, scratch, spilled VGPRs, spilled SGPRs, LDS
    was, was_stats = ehs.recorded(), recorded_stats()
    for form in ehs.FORM:
        want = was_stats if form == "stats" else {k: v[form] for k, v in was.items()}
        differ = sorted(k for k, f in plain.items() if k not in want or cols(f[form]) != want[k])
        print(f"Without the ring, evaluate_hist_kernel<Variant, HN, {form}>: {len(plain) - len(differ)} of {len(plain)} kernels reproduce the VGPR, "
              f"SGPR, scratch, spill and LDS figures on record" + ("." if not differ else f"; {len(differ)} differ: {differ}"))
    name = lambda k: f"{k[0]} {k[1]} {k[2]} HN {k[3]}"
    for form in ehs.FORM:
        new = [cols(f[form]) for f in ring.values()]
        spills = sorted(k for k, f in ring.items() if f[form][1] > plain[k][form][1])
        scratch = sorted(k for k, f in ring.items() if f[form][4] > plain[k][form][4])
        print(f"On the ring, {form} form: {len(new)} kernels; VGPRs {min(c[0] for c in new)} .. {max(c[0] for c in new)}; LDS "
              f"{min(c[5] for c in new)} .. {max(c[5] for c in new)} B per block (limit 163840); scratch at most {max(c[2] for c in new)} B per lane; "
              f"spilled VGPRs at most {max(c[3] for c in new)}.  {len(spills)} spill more VGPRs than their twin" +
              (": " + ", ".join(name(k) for k in spills) if spills else "") + f"; {len(scratch)} need more scratch than their twin" +
              (": " + ", ".join(name(k) for k in scratch) if scratch else "") + ".")
        print(f"    ring - twin: VGPRs {min(cols(f[form])[0] - cols(plain[k][form])[0] for k, f in ring.items()):+d} .. "
              f"{max(cols(f[form])[0] - cols(plain[k][form])[0] for k, f in ring.items()):+d}; spilled SGPRs "
              f"{min(f[form][3] - plain[k][form][3] for k, f in ring.items()):+d} .. {max(f[form][3] - plain[k][form][3] for k, f in ring.items()):+d}; LDS "
              f"{' / '.join(sorted({'%+d' % (f[form][5] - plain[k][form][5]) for k, f in ring.items()}))} B per block.")
    for form in ehs.FORM:
        print()
        print(f"{form} form")
        print(f"{'task':8s}{'flags':7s}{'ctrl':6s}{'HN':>3s} |{'VGPR':>5s}{'SGPR':>5s}{'scr':>5s}{'spV':>4s}{'spS':>4s}{'LDS':>8s} |{'VGPR':>5s}{'SGPR':>5s}{'scr':>5s}{'spV':>4s}{'spS':>4s}{'LDS':>8s} | dVGPR dscr")
        for k in sorted(ring):
            e, r = cols(plain[k][form]), cols(ring[k][form])
            print(f"{k[0]:8s}{k[1]:7s}{k[2]:6s}{k[3]:3d} |{e[0]:5d}{e[1]:5d}{e[2]:5d}{e[3]:4d}{e[4]:4d}{e[5]:8d} |{r[0]:5d}{r[1]:5d}{r[2]:5d}{r[3]:4d}{r[4]:4d}{r[5]:8d} |{r[0] - e[0]:+6d}{r[2] - e[2]:+5d}")


if __name__ == "__main__":
    main()
