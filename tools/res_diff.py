#!/usr/bin/env python3
"""Two sets of *.res resource reports (hipcc -Rpass-analysis=kernel-resource-usage, kept by the Makefile) kernel by kernel:
VGPRs, SGPRs, scratch and occupancy of each kernel before and after a change.

    res_diff.py --old OLD.res [OLD2.res ...] --new NEW.res [...] [--map 'old<A,B>=new<A,A,B,true>' ...]

Kernels are matched on their demangled name and template arguments.  A --map rule renames a template of the old set before
matching: the names left of `=` bind the old kernel's arguments in order, the right side is the new kernel with those names
substituted (anything else, `true` or `32`, stands for itself).  Exit status 1 if a kernel has no twin, uses scratch, has more
VGPRs or a lower occupancy than its twin."""
import argparse
import re
import sys

FIELDS = (("VGPR", r"VGPRs"), ("SGPR", r"TotalSGPRs"), ("scr", r"ScratchSize \[bytes/lane\]"), ("occ", r"Occupancy \[waves/SIMD\]"))


def split_template(name):
    """'k<a, b<c, d>, 3>' -> ('k', ['a', 'b<c, d>', '3']); no template: ('k', [])."""
    if "<" not in name:
        return name, []
    base, rest = name.split("<", 1)
    args, depth, cur = [], 0, ""
    for ch in rest[:rest.rindex(">")]:
        depth += (ch == "<") - (ch == ">")
        if ch == "," and depth == 0:
            args.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return base, args + [cur.strip()]


BUILTIN = {"DF16_": "_Float16", "DF16b": "__bf16", "f": "float", "d": "double", "i": "int", "j": "unsigned", "b": "bool", "l": "long"}


def demangle(sym):
    """The kernel's name with its template arguments, without namespaces and parameters: all a kernel of this library needs
    (builtin types, integer and bool constants); an older c++filt does not know _Float16 and __bf16.
    Anything else comes back as it is."""
    pos, names = 2 + sym.startswith("_ZN"), []
    while (m := re.match(r"\d+", sym[pos:])):
        n = int(m.group())
        names.append(sym[pos + len(m.group()):pos + len(m.group()) + n])
        pos += len(m.group()) + n
    if not names:
        return sym
    if sym[pos:pos + 1] != "I":
        return names[-1]
    pos, args = pos + 1, []
    while sym[pos:pos + 1] != "E":
        if (m := re.match(r"L([a-z])(n?\d+)E", sym[pos:])):
            args.append({"0": "false", "1": "true"}[m.group(2)] if m.group(1) == "b" else m.group(2).replace("n", "-"))
            pos += len(m.group())
        elif (code := next((c for c in BUILTIN if sym.startswith(c, pos)), None)):
            args.append(BUILTIN[code])
            pos += len(code)
        else:
            return sym
    return f"{names[-1]}<{', '.join(args)}>"


def kernels(paths):
    """{demangled kernel: {field: int}}"""
    blocks = [b for p in paths for b in re.split(r"remark: Function Name: ", open(p).read())[1:]]
    return {demangle(b.split()[0]): {k: int(re.search(pat + r": (\d+)", b).group(1)) for k, pat in FIELDS} for b in blocks}


def rename(name, rules):
    base, args = split_template(name)
    for old, new in rules:
        obase, onames = split_template(old)
        if obase == base and len(onames) == len(args):
            bound = dict(zip(onames, args))
            nbase, nargs = split_template(new)
            return f"{nbase}<{', '.join(bound.get(a, a) for a in nargs)}>"
    return name


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--map", action="append", default=[])
    a = ap.parse_args()
    rules = [m.split("=", 1) for m in a.map]
    old = {rename(k, rules): v for k, v in kernels(a.old).items()}
    new = kernels(a.new)
    bad = 0
    print(f"{len(old)} kernels before, {len(new)} after")
    print("kernel".ljust(78) + "".join(f"{k:>10}" for k, _ in FIELDS))
    for name in sorted(set(old) | set(new)):
        o, n = old.get(name), new.get(name)
        if o is None or n is None:
            print(name.ljust(78) + ("  only before" if n is None else "  only after"))
            bad += 1
            continue
        worse = n["scr"] > 0 or n["VGPR"] > o["VGPR"] or n["occ"] < o["occ"]
        bad += worse
        print(name.ljust(78) + "".join(f"{o[k]:>5}→{n[k]:<4}" if o[k] != n[k] else f"{n[k]:>10}" for k, _ in FIELDS) + ("  WORSE" if worse else ""))
    print(f"{bad} kernels without a twin, with scratch, more VGPRs or a lower occupancy" if bad else
          "every kernel has a twin, scratch 0, no more VGPRs and no lower occupancy than before")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
