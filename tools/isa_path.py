#!/usr/bin/env python3
"""tools/isa_path.py <kernel.s> <start> <end> [decisions] : instruction classes along ONE path through a kernel's assembly
(the file tools/isa_dev.sh writes, /tmp/kdev_<mode>_kernel.s), where isa_dev.sh's own table counts every instruction of a
barrier section once -- the tail-copy, first-block and fault paths of the pair kernel included.

  start, end   a label (.LBB17_211) or a line number of the file; the walk begins at `start` and stops in front of `end`
  decisions    one letter per CONDITIONAL branch in the order the walk meets them: t = taken, n = not taken; when the
               string runs out the rest are not taken.  s_branch is followed.  A loop is walked as often as its back edge
               is marked t.

Prints the classes isa_dev.sh uses (fp64, other VALU, SALU, SMEM, LDS, VMEM, waits, barriers) and every branch met with the
decision applied, so that a path can be written down step by step and checked against the source.  The counts are what one
wave ISSUES on that path; they say nothing about cycles (tools/stamps_probe.py) and are anchored by the whole-kernel
counters of tools/pmc_summary.py (SQ_INSTS_VALU, SQ_INSTS_SALU per SQ_WAVES)."""
import collections
import re
import sys


def classify(op):
    if op == "s_barrier": return "barrier"
    if op.startswith("v_") and "f64" in op: return "fp64"
    if op.startswith("v_"): return "valu_other"
    if op.startswith("s_waitcnt") or op.startswith("s_nop"): return "wait"
    if op.startswith("s_load") or op.startswith("s_buffer_load"): return "smem"
    if op.startswith("s_"): return "salu"
    if op.startswith("ds_"): return "lds"
    if op.startswith(("global_", "scratch_", "buffer")): return "vmem"
    return "other"


def main():
    if len(sys.argv) < 4:
        raise SystemExit(__doc__)
    lines = open(sys.argv[1]).read().split("\n")
    labels = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r"^(\.L\w+):", l)] if m}

    def where(s):
        return int(s) - 1 if s.isdigit() else labels[s]

    pc, end = where(sys.argv[2]), where(sys.argv[3])
    dec = list(sys.argv[4]) if len(sys.argv) > 4 else []
    cnt = collections.Counter()
    steps = 0
    while pc != end:
        if pc >= len(lines) or steps > 1000000:
            raise SystemExit("the walk left the kernel without reaching %s" % sys.argv[3])
        steps += 1
        m = re.match(r"\s+([a-z_0-9]+)\s*(\S*)", lines[pc])
        pc += 1
        if not m:
            continue
        op, arg = m.group(1), m.group(2)
        cnt[classify(op)] += 1
        if op == "s_endpgm":
            break
        if op == "s_branch":
            pc = labels[arg]
        elif op.startswith("s_cbranch"):
            d = dec.pop(0) if dec else "n"
            print("line %5d  %-20s %-14s %s" % (pc, op, arg, "taken" if d == "t" else "not taken"))
            if d == "t":
                pc = labels[arg]
    print("%6s %10s %6s %6s %6s %6s %6s %8s" % ("fp64", "valu_other", "salu", "smem", "lds", "vmem", "wait", "barrier"))
    print("%6d %10d %6d %6d %6d %6d %6d %8d" % tuple(cnt[k] for k in ("fp64", "valu_other", "salu", "smem", "lds", "vmem", "wait", "barrier")))


if __name__ == "__main__":
    main()
