#!/usr/bin/env python3
"""tools/isa_compare.py <old.s> <new.s> <regex> : do the kernels whose mangled name matches <regex> have the same code in
two assembly files of the device code?  The files come from the compile line of csrc/Makefile with `-S --cuda-device-only`
in the place of `-c` (for the PCM edges: the rest part, -DR8B_TU_NOPAIR=8), once in a checkout of the old commit and once
here.  A kernel's text runs from its label to its .Lfunc_end, kernel descriptor included; comments, the numbers of local
labels (they count the functions in front) and .amdhsa_kernarg_size (it changes with every field a launch descriptor
gains, the offsets of the old fields do not) are left out of the comparison.  Prints one line per kernel and the kernels
only the new file has; exit status 1 if any kernel differs or is missing."""
import re
import sys


def kernels(path):
    out, cur, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            cur, body = m.group(1), []
        elif cur is not None:
            body.append(line)
            if line.startswith(".Lfunc_end"):
                out[cur], cur = body, None
    return out


def norm(body):
    r = []
    for line in body:
        line = re.sub(r"\s*;.*$", "", line.rstrip())
        line = re.sub(r"\.LBB\d+_", ".LBB_", line)
        line = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", line)
        if line.strip() and ".amdhsa_kernarg_size" not in line:
            r.append(line)
    return r


old, new, pat = kernels(sys.argv[1]), kernels(sys.argv[2]), re.compile(sys.argv[3])
bad = 0
for k in sorted(old):
    if not pat.search(k):
        continue
    if k not in new:
        print("MISSING             %s" % k)
        bad += 1
        continue
    a, b = norm(old[k]), norm(new[k])
    print("%s %6d lines  %s" % ("same     " if a == b else "DIFFERENT", len(a), k))
    bad += a != b
print("only in the new file:", ", ".join(sorted(k for k in new if k not in old and pat.search(k))) or "none")
sys.exit(1 if bad else 0)
