#!/usr/bin/env python3
"""asm_identity.py [--rename REGEX=REPLACEMENT ...] PARENT.s NEW.s -- are the kernels of two device assemblies of one translation unit the same, one by one?

Both files come from hipcc with the flags of build.py plus --cuda-device-only -S.  A kernel is the text from its label through
its .end_amdhsa_kernel (instructions and kernel-descriptor directives); comments, trailing blanks, the position-dependent
number in .LBB<n>_ / .Lfunc_end<n> / .Ltmp<n> labels and the kernel's own mangled name are normalised away, nothing else.
Kernels are matched by their plain demangled name (c++filt); --rename applies re.sub(REGEX, REPLACEMENT) to the PARENT's
demangled names first, for a change that renames a kernel or its template arguments and nothing else.
Prints one row per kernel (identical / gone / APPEARED / DIFFERS, instruction lines) and exits 1 unless every kernel of NEW.s
is identical to its namesake."""
import re, subprocess, sys


def kernels(path):
    text = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    lines = text.split("\n")
    label = {ln.split(":")[0]: i for i, ln in enumerate(lines) if ln.startswith("_Z") and ":" in ln}
    out = {}
    for name in names:
        start = label[name]
        end = next(i for i in range(start, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        body = []
        for ln in lines[start:end + 1]:
            ln = ln.split(";")[0].rstrip()
            if not ln:
                continue
            ln = ln.replace(name, "KERNEL")
            ln = re.sub(r"\.(LBB|Lfunc_end|Ltmp)\d+", r".\1N", ln)
            body.append(ln)
        out[name] = body
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return r.stdout.split("\n")[:len(names)]


def insn_count(body):
    n = 0
    for ln in body:
        s = ln.strip()
        if s.startswith(".") or s.endswith(":"):
            continue
        n += 1
    return n


def load(path, renames=()):
    k = kernels(path)
    names = list(k)
    out = {}
    for nm, d in zip(names, demangle(names)):
        for pattern, replacement in renames:
            d = re.sub(pattern, replacement, d)
        assert d not in out, d  # (a rename must not merge two kernels)
        out[d] = k[nm]
    return out


argv, renames = sys.argv[1:], []
while argv and argv[0] == "--rename":
    renames.append(tuple(argv[1].split("=", 1)))
    argv = argv[2:]
a, b = load(argv[0], renames), load(argv[1])
bad = 0
for name in sorted(set(a) | set(b)):
    if name not in b:
        print("%-62s gone       %6d" % (name, insn_count(a[name])))
    elif name not in a:
        print("%-62s APPEARED   %6d" % (name, insn_count(b[name]))); bad += 1
    elif a[name] == b[name]:
        print("%-62s identical  %6d" % (name, insn_count(a[name])))
    else:
        print("%-62s DIFFERS    %6d -> %d" % (name, insn_count(a[name]), insn_count(b[name]))); bad += 1
print("parent kernels %d, new kernels %d, not identical %d" % (len(a), len(b), bad))
sys.exit(1 if bad else 0)
