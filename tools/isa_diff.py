#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two `hipcc --cuda-device-only -S` files of one unit (parent commit / this one).

Every kernel of the OLD file whose demangled name contains the filter is matched with the kernel of the NEW file that has
the same template arguments followed by SUFFIX (the arguments a template gained, with their defaults; "" if none).
Compared: the function body from its label to .Lfunc_end, comments and blank lines dropped, the kernel's own mangled name
and the basic-block label numbers normalised.  Kernarg offsets are part of the compared text.

usage: isa_diff.py old.s new.s name-filter [suffix, e.g. ", false"]"""
import hashlib
import re
import subprocess
import sys


def bodies(path):
    """mangled kernel name -> list of normalised instruction lines"""
    text = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    out = {}
    for name in names:
        m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, flags=re.M | re.S)
        lines = []
        for ln in m.group(1).splitlines():
            ln = ln.split(";")[0].strip()
            if not ln:
                continue
            ln = ln.replace(name, "KERNEL")
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
            lines.append(ln)
        out[name] = lines
    return out


def demangle(names):
    p = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return [re.sub(r"\(.*", "", n).replace("void ", "") for n in p.stdout.splitlines()]


def main():
    old, new = bodies(sys.argv[1]), bodies(sys.argv[2])
    flt = sys.argv[3]
    suffix = sys.argv[4] if len(sys.argv) > 4 else ""
    new_by_name = dict(zip(demangle(list(new)), new.values()))
    twin = lambda d: d[:-1] + suffix + ">" if suffix and d.endswith(">") else d
    print(f"{'old instr':>10s} {'new instr':>10s} {'differing':>9s}  {'sha256 old':16s} {'sha256 new':16s}  instantiation (old name; the new one ends in '{suffix}>')")
    total = missing = 0
    for dn, body in zip(demangle(list(old)), old.values()):
        if flt not in dn:
            continue
        other = new_by_name.get(twin(dn))
        if other is None:
            print(f"{len(body):10d} {'-':>10s} {'-':>9s}  no counterpart: {dn}")
            missing += 1
            continue
        diff = sum(a != b for a, b in zip(body, other)) + abs(len(body) - len(other))
        total += diff
        sha = lambda b: hashlib.sha256("\n".join(b).encode()).hexdigest()[:16]
        print(f"{len(body):10d} {len(other):10d} {diff:9d}  {sha(body)} {sha(other)}  {dn}")
    print(f"total differing lines: {total}; kernels without a counterpart: {missing}")
    print("new kernels: " + ", ".join(n for n in new_by_name if flt in n and not any(
        n == twin(d) for d in demangle(list(old)))))
    return 1 if total or missing else 0


if __name__ == "__main__":
    sys.exit(main())
