#!/usr/bin/env python3
"""Compare the kernels of two sets of AMDGPU assembly files, function by function.

    hipcc <the Makefile's flags> --cuda-device-only -S -Rpass-analysis=kernel-resource-usage a.hip -o a.s 2> a.usage
    tools/kernel_asm_diff.py --a old.s --b new1.s new2.s [--usage-a old.usage --usage-b new1.usage new2.usage]

Every function of side A must appear exactly once on side B, and the other way round, with the same text once comments are
dropped and local labels (.L...) are numbered by first appearance.  The text of a function runs from its label to its
.Lfunc_end, so it includes the kernel descriptor (.amdhsa_* : registers, LDS, scratch).  With --usage-*, the figures of the
-Rpass-analysis=kernel-resource-usage remarks are compared too.  Exit status 0 when both sides agree.
"""
import argparse
import collections
import re
import sys


def functions(paths):
    """name -> list of normalised bodies (one per definition found)"""
    out = collections.defaultdict(list)
    for path in paths:
        types = set()
        name, body = None, []
        for line in open(path):
            m = re.match(r"\s*\.type\s+([^,\s]+),@function", line)
            if m:
                types.add(m.group(1))
                continue
            m = re.match(r"([A-Za-z_$][\w$.]*):", line)
            if name is None:
                if m and m.group(1) in types:
                    name, body = m.group(1), []
                continue
            if re.match(r"\.Lfunc_end\d+:", line):
                out[name].append(normalise(body))
                name = None
                continue
            body.append(line)
    return out


def normalise(lines):
    labels = {}

    def number(m):
        return labels.setdefault(m.group(0), ".L%d" % len(labels))

    text = []
    for line in lines:
        line = line.split(";", 1)[0].rstrip()
        if line.strip():
            text.append(re.sub(r"\.L[\w$.]+", number, line))
    return "\n".join(text)


def usage(paths):
    """name -> {figure: value} from the resource-usage remarks"""
    out, cur = {}, None
    for path in paths:
        for line in open(path, errors="replace"):
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                cur = out.setdefault(m.group(1), {})
                continue
            m = re.search(r"remark:\s+([^:]+): (\S+) \[-Rpass-analysis", line)
            if m and cur is not None:
                cur[m.group(1).strip()] = m.group(2)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--a", nargs="+", required=True)
    ap.add_argument("--b", nargs="+", required=True)
    ap.add_argument("--usage-a", nargs="*", default=[])
    ap.add_argument("--usage-b", nargs="*", default=[])
    args = ap.parse_args()
    fa, fb = functions(args.a), functions(args.b)
    bad = 0
    for name in sorted(set(fa) | set(fb)):
        na, nb = len(fa.get(name, [])), len(fb.get(name, []))
        if na != 1 or nb != 1:
            print("COUNT   %s: %d in a, %d in b" % (name, na, nb))
            bad += 1
        elif fa[name][0] != fb[name][0]:
            la, lb = fa[name][0].split("\n"), fb[name][0].split("\n")
            first = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            print("DIFFERS %s: %d / %d lines, first at %d" % (name, len(la), len(lb), first))
            print("    a: %s\n    b: %s" % (la[first] if first < len(la) else "<end>", lb[first] if first < len(lb) else "<end>"))
            bad += 1
    print("%d functions in a, %d in b, %d not identical" % (len(fa), len(fb), bad))
    if args.usage_a or args.usage_b:
        ua, ub = usage(args.usage_a), usage(args.usage_b)
        ubad = 0
        for name in sorted(set(ua) | set(ub)):
            if ua.get(name) != ub.get(name):
                print("USAGE   %s:\n    a: %s\n    b: %s" % (name, ua.get(name), ub.get(name)))
                ubad += 1
        print("resource usage: %d kernels in a, %d in b, %d not identical" % (len(ua), len(ub), ubad))
        bad += ubad
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
