#!/usr/bin/env python3
"""Compare the kernels of two gfx950 assembly listings (hipcc --save-temps: *-hip-amdgcn-amd-amdhsa-gfx950.s), kernel by kernel.

    tools/kernel_diff.py OLD.s NEW.s [--map FILE] [--identical REGEX]

OLD.s / NEW.s may each be several files joined with commas (a source file split into translation units).  Kernels are paired by
their demangled names.  --map FILE renames the OLD kernels first: every line `REGEX => REPLACEMENT` is a re.sub applied, in file
order, to each old demangled name (blank lines and lines starting with # are skipped), e.g. when a template parameter changed its type.

Per pair the tool compares the instruction stream (labels, comments, directives and symbol names stripped) and the .amdhsa_* resource
lines, prints `identical` or `differs`, and for a kernel that differs both sets of resource figures and the instruction counts.
Exit status 1: kernels left unpaired, or a kernel whose (new) name matches --identical differs.
"""
import argparse
import re
import subprocess
import sys

RESOURCES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size", "kernarg_size")


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
            return dict(zip(names, out.splitlines()))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def normalise(line):
    line = line.split(";", 1)[0].strip()
    if not line or line.startswith(".") or re.match(r"^[^\s,]+:$", line):
        return None
    line = re.sub(r"\.L[\w$.]+", "<L>", line)                     # local labels (branch targets, function ends)
    line = re.sub(r"\b[A-Za-z_][\w$.]*@[\w@]+", "<S>", line)      # symbol@rel32@lo and the like
    line = re.sub(r"\b_Z\w+", "<S>", line)                        # mangled names
    return re.sub(r"\s+", " ", line)


def parse(paths):
    """{mangled kernel name: (instruction list, {.amdhsa_x: value})}"""
    bodies, descs = {}, {}
    for path in paths:
        cur = None
        desc = None
        for raw in open(path, errors="replace"):
            s = raw.strip()
            m = re.match(r"^\.amdhsa_kernel\s+(\S+)", s)
            if m:
                desc = descs.setdefault(m.group(1), {})
                continue
            if s == ".end_amdhsa_kernel":
                desc = None
                continue
            if desc is not None:
                m = re.match(r"^\.amdhsa_(\w+)\s+(.*)$", s)
                if m:
                    desc[m.group(1)] = m.group(2).split(";", 1)[0].strip()
                continue
            m = re.match(r"^\.type\s+(\S+),@function", s)
            if m:
                cur = bodies.setdefault(m.group(1), [])
                continue
            if s.startswith(".size") or s.startswith(".section") or s.startswith(".rodata"):
                cur = None
                continue
            if cur is not None:
                n = normalise(raw)
                if n:
                    cur.append(n)
    return {k: (bodies.get(k, []), d) for k, d in descs.items()}


def figures(desc):
    return " ".join(f"{r}={desc.get(r, '-')}" for r in RESOURCES)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map")
    ap.add_argument("--identical", help="kernels whose name matches this regex must be identical")
    args = ap.parse_args()
    rules = []
    if args.map:
        for line in open(args.map):
            line = line.rstrip("\n")
            if line.strip() and not line.lstrip().startswith("#"):
                pat, _, repl = line.partition(" => ")
                rules.append((re.compile(pat), repl))
    sides = []
    for spec in (args.old, args.new):
        kernels = parse(spec.split(","))
        names = demangle(list(kernels))
        sides.append({names[k]: v for k, v in kernels.items()})
    old = {}
    for name, v in sides[0].items():
        for pat, repl in rules:
            name = pat.sub(repl, name)
        old[name] = v
    new = sides[1]
    same = differ = must = 0
    for name in sorted(set(old) & set(new)):
        (oi, od), (ni, nd) = old[name], new[name]
        if oi == ni and od == nd:
            same += 1
            print(f"identical  {name}")
            continue
        differ += 1
        bad = bool(args.identical and re.search(args.identical, name))
        must += bad
        what = "instructions" if oi != ni else "resources only"
        print(f"differs    {name}   [{what}]{'   <-- must be identical' if bad else ''}")
        print(f"    old: {len(oi)} instructions  {figures(od)}")
        print(f"    new: {len(ni)} instructions  {figures(nd)}")
        for k in sorted(set(od) | set(nd)):
            if k not in RESOURCES and od.get(k) != nd.get(k):
                print(f"    .amdhsa_{k}: {od.get(k)} -> {nd.get(k)}")
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    for name in only_old:
        print(f"only old   {name}")
    for name in only_new:
        print(f"only new   {name}")
    print(f"{len(sides[0])} kernels before, {len(new)} after: {same + differ} paired, {same} identical, {differ} differ, "
          f"{len(only_old)} only old, {len(only_new)} only new")
    return 1 if (only_old or only_new or must or len(old) != len(sides[0])) else 0


if __name__ == "__main__":
    sys.exit(main())
