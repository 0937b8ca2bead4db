#!/usr/bin/env python3
"""Compares the per-kernel gfx950 instruction streams of hipcc -S listings, kernel by kernel, by symbol name.

usage: tools/isa_kernel_diff.py [--map OLD=NEW]... <before.s> <after.s>
       tools/isa_kernel_diff.py [--map OLD=NEW]... <before.s> ... -- <after.s> ...

Each side is one listing or several (code that moved between translation units: a kernel's symbol does not depend on the
file that defines it); the kernels of a side's listings are taken together.

A kernel's body is every instruction from its symbol to its .Lfunc_end label, with comments removed and
local labels (.LBB*, .Ltmp*) renamed by order of appearance, so that code that only moved inside the file
compares equal; its .amdhsa_* descriptor (registers, LDS, scratch) is compared as well.  Prints one line per
kernel that differs, one per kernel present on one side only, and a summary; exit status 1 when anything
differs.

--map OLD=NEW pairs a renamed kernel: OLD is a substring of exactly one symbol before, NEW of exactly one after (mangled names:
"k_scan_tilesILi256EjE" picks k_scan_tiles<256, uint32_t>), and the two are compared as one kernel, body and descriptor.

Listings are made with the Makefile's FLAGS, e.g.

  hipcc $(FLAGS) --cuda-device-only -S distance.hip -o distance.s
"""
import re
import sys

LABEL = re.compile(r"\.L(BB|tmp)[0-9_]+")


def kernels(path):
    lines = open(path).read().split("\n")
    names = [m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m]
    out = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.split(";", 1)[0].strip() == name + ":")
        body, labels = [], {}
        for l in lines[start + 1:]:
            if l.startswith(".Lfunc_end"):
                break
            t = l.split(";", 1)[0].rstrip()
            if not t.strip() or re.match(r"^\.L\w+:", t) or t.strip().startswith("."):
                continue
            body.append(LABEL.sub(lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), t.strip()))
        k = lines.index("\t.amdhsa_kernel " + name)
        desc = []
        for l in lines[k + 1:]:
            if ".end_amdhsa_kernel" in l:
                break
            desc.append(l.strip())
        out[name] = (body, desc)   # desc starts after the .amdhsa_kernel line: it does not hold the name
    return out


def side(paths):
    out = {}
    for path in paths:
        for name, k in kernels(path).items():
            if name in out:
                sys.exit("%s: %s is defined by another listing of the same side too" % (path, name))
            out[name] = k
    return out


def one_symbol(names, sub, which):
    hits = [n for n in names if sub in n]
    if len(hits) != 1:
        sys.exit("--map: '%s' matches %d symbols %s, not one: %s" % (sub, len(hits), which, ", ".join(hits)))
    return hits[0]


def main():
    args = sys.argv[1:]
    maps = []
    while "--map" in args:
        i = args.index("--map")
        if i + 1 >= len(args) or "=" not in args[i + 1]:
            sys.exit(__doc__)
        maps.append(args[i + 1].split("=", 1))
        del args[i:i + 2]
    cut = args.index("--") if "--" in args else 1
    before, after = args[:cut], [p for p in args[cut:] if p != "--"]
    if not before or not after:
        sys.exit(__doc__)
    a, b = side(before), side(after)
    for was, now in [(one_symbol(a, old, "before"), one_symbol(b, new, "after")) for old, new in maps]:
        if now in a and now != was:
            sys.exit("--map: %s exists before as well" % now)
        a[now] = a.pop(was)
    differ = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("only in %s: %s" % ("after" if name in b else "before", name))
            differ += 1
        elif a[name] != b[name]:
            print("differs (%d / %d instructions): %s" % (len(a[name][0]), len(b[name][0]), name))
            differ += 1
    same = len(set(a) & set(b)) - sum(1 for n in set(a) & set(b) if a[n] != b[n])
    print("%d kernels before, %d after: %d identical, %d differ or are missing" % (len(a), len(b), same, differ))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
