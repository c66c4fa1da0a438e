"""The names of evaluate_kernel's instantiations in the built library, read once for the tools of this directory:
    void pds::evaluate_kernel<pds::Variant<task, motor, dr, ge, tn, on, ctrl, lat, hold>, TEAMS, (pds::EvalForm)F>(...)
(csrc/pds_evaluate.h; F by value: EvalForm of csrc/pds_evaluate_args.h).  Code-object metadata: no device needed."""
import re

import kernel_resources as kr

FORMS = ("plain", "metrics", "stats", "record")  # EvalForm 0 .. 3
TASK = ("Hover", "Circle", "TakeOff")
CTRL = ("PWM", "Rate", "Att")
HOVER_DEFAULT = ("Hover", "DTO", "PWM", "")  # Hover: domain randomisation, thrust and observation noise
NAME = re.compile(r"evaluate_kernel<pds::Variant<(\d), (\w+), (\w+), (\w+), (\w+), (\w+), (\d), (\w+), (\w+)>, (\d), \(pds::EvalForm\)(\d)>")


def parse(name):
    """a demangled kernel name -> ((task, flags, ctrl, ring, teams), form), or None where it is no evaluate_kernel"""
    m = NAME.search(name)
    if not m:
        return None
    task, motor, dr, ge, tn, on, ctrl, lat, hold, teams, form = m.groups()
    flags = "".join(c for c, v in zip("MDGTO", (motor, dr, ge, tn, on)) if v == "true") or "-"
    ring = "lat" if lat == "true" else ("hold" if hold == "true" else "")
    return (TASK[int(task)], flags, CTRL[int(ctrl)], ring, int(teams)), FORMS[int(form)]


def rows(lib=None):
    """{(task, flags, ctrl, ring, teams): {form: (vgprs, vgpr spills, sgprs, sgpr spills, scratch, lds)}}"""
    out = {}
    for r in kr.kernel_table(lib):
        parsed = parse(r[0])
        if parsed:
            out.setdefault(parsed[0], {})[parsed[1]] = r[1:]
    return out


def hover_default_scratch(off, on):
    """{(is it form `on`?, teams): scratch bytes per lane} of Hover's default variant in its forms `off` and `on`"""
    return {(form == on, key[4]): figures[4] for key, forms in rows().items() if key[:4] == HOVER_DEFAULT
            for form, figures in forms.items() if form in (off, on)}
