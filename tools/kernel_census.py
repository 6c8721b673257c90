#!/usr/bin/env python3
"""tools/kernel_census.py -- authors and checks tests/kernel_census.py, the table with one entry per compiled instance of
the compile-time-sized convolver kernels (k_convp, k_convp_walk, k_convq, k_convx).

  --list LIB   the instances a built library holds, one symbol per line as stage_symbols() prints them.  Only symbol
               NAMES are read (nm -C): the device library's host stubs (__device_stub__k_convp<...>), or, for the host
               emulation (tests/emul/_build/libr8bsrc_emul.so), the per-instance name strings of r8b_dispatch.h
               (convp_run<...>::sym, convx_run<...>::sym).
  --sweep      under the host emulation: walks the grid below, chain by chain, and records for every symbol the first
               configuration that launched it.  Prints proposed table entries (the lines of tests/kernel_census.py
               RUNS) and the instances no chain of the grid reached.  A chain the library built that then fails in a
               call -- a launcher refusing an instance as "not built", any other exception -- is printed as FAILED and
               makes the exit status 1: no chain is passed over.  --jobs N processes (default: the CPUs at hand,
               16 at most); --only SUBSTRING prints the symbols that contain it; --part coarse|fine: one part of the grid.

The grid (GRID_*): ratios covering every io= class of tests/cases.py -- 2/1 alone and fused, 2/1 with In > Out, 1/1
fused, 1/2, 1/3, 2/3, 3/2, 3/4, 3/1, 4/1 and 16/1 behind half-band decimators, interpolator-first chains, half-band
cascades behind, the polynomial bank --; transition bands from 45 % down to 0.5 %; attenuations from 49 to 218 dB;
both phases; and the option sets of OPTION_SETS: the defaults first, then one opt-in or opt-out form each (unfused 1:1
is `fuse = 0`) -- the coarse part; and a fine part (FINE_*, --part fine): ratios whose whole-step interpolator has few
phases, on finer bands and attenuations, under the defaults and the walk form.  A symbol is credited to the cheapest
chain whose CONVOLVER stage launched it: default options before option sets, linear before minimum phase, a
minimum-phase filter the reference does not delay its input for before one it does (input_delayed), then the shortest
stream.  Chains with a polynomial interpolator run, but are credited with nothing (the reference's depends on the cut
into calls).  Every chain runs with the forms pinned (half = half_fused = walk = 0 unless the set says otherwise), three channels
and whole calls of MaxInLen until every convolver has had a few blocks."""
import argparse
import math
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FAMILIES = ("k_convp", "k_convp_walk", "k_convq", "k_convx")


def _norm(args):
    return ", ".join(a.strip() for a in args.split(","))


def list_instances(lib):
    """the sorted symbols of the four families in a built library (device library or host emulation)"""
    out = subprocess.run(["nm", "-C", lib], check=True, stdout=subprocess.PIPE, text=True).stdout
    found = set()
    seen_run = set()
    for line in out.splitlines():
        m = re.search(r"__device_stub__(k_convp_walk|k_convp|k_convx)<([-\d, ]+)>\(", line)
        if m:
            found.add("%s<%s>" % (m.group(1), _norm(m.group(2))))
            continue
        if re.search(r"__device_stub__k_convq\(", line) or re.search(r"\bconvq_body<", line):
            found.add("k_convq")
            continue
        # the emulation: the launcher's name strings.  convp_run holds two of them, for the plain and for the walk form (the
        # second exists only where convp_walk_ok): a repeated name is the walk instance
        m = re.search(r"\b(convp_run|convx_run)<([-\d, ]+), r8bhip::EmulLaunch>\(.*\)::sym$", line)
        if m and " guard variable " not in line:
            args = _norm(m.group(2))
            if m.group(1) == "convx_run":
                found.add("k_convx<%s>" % args)
            elif args in seen_run:
                found.add("k_convp_walk<%s>" % args)
            else:
                seen_run.add(args)
                found.add("k_convp<%s>" % args)
    return sorted(found, key=sort_key)


def sort_key(sym):
    m = re.match(r"(\w+)(?:<(-?\d+), (-?\d+), (\d+), (\d+)>)?$", sym)
    return (FAMILIES.index(m.group(1)),) + tuple(int(v) for v in m.groups()[1:] if v is not None)


# ---------------------------------------------------------------- the grid
GRID_RATIOS = [
    (44100.0, 88200.0), (44100.0, 96000.0), (48000.0, 44100.0), (96000.0, 44100.0), (88200.0, 44100.0),
    (96000.0, 32000.0), (48000.0, 32000.0), (32000.0, 48000.0), (64000.0, 48000.0), (44100.0, 132300.0),
    (176400.0, 44100.0), (2822400.0, 176400.0), (192000.0, 44100.0), (11025.0, 96000.0), (44100.0, 192000.0),
    (8000.0, 44100.0), (44100.0, 176400.0), (44100.0, 529200.0), (44100.0, 44101.0), (32000.0, 44100.0),
    (88200.0, 48000.0), (16000.0, 44100.0), (288000.0, 48000.0), (96000.0, 16000.0),
]
GRID_TB = [45.0, 30.0, 20.0, 10.0, 5.0, 3.0, 2.0, 1.4, 1.0, 0.7, 0.5]
GRID_ATT = [49.0, 60.0, 80.0, 109.56, 136.45, 160.0, 180.15, 206.91, 218.0]
GRID_PHASE = [0, 1]
# the fine part: whole-step interpolators of FEW phases behind the convolver (steps 3/2, 6/5, 8/3, 12/5, 5/3, 7/4, 5/2,
# 7/2), where the interpolator's run fits the short blocks' arrays and the fused two-phase forms reach the small
# geometries -- each only in a narrow window of filter lengths, hence the finer bands and attenuations
FINE_RATIOS = [
    (48000.0, 64000.0), (44100.0, 73500.0), (48000.0, 36000.0), (48000.0, 40000.0), (48000.0, 57600.0),
    (44100.0, 50400.0), (100000.0, 40000.0), (96000.0, 36000.0), (50000.0, 20000.0), (70000.0, 20000.0),
    # (3/2 once more: the finer grid holds minimum-phase filters of EVEN latency on every block length -- input_delayed)
    (32000.0, 48000.0),
]
FINE_TB = [45.0, 40.0, 35.0, 30.0, 25.0, 20.0, 15.0, 10.0, 7.0, 5.0, 3.0, 2.0]
FINE_ATT = [49.0, 55.0, 60.0, 70.0, 80.0, 90.0, 100.0, 109.56, 120.0, 136.45, 150.0, 160.0, 180.15, 206.91]
FINE_SETS = [0, 6]     # of OPTION_SETS: the defaults and the walk form
PIN = {"half": 0, "half_fused": 0, "walk": 0}
# (options, MaxInLen or None for the default): the defaults, then every opt-in / opt-out form on its own
OPTION_SETS = [
    ({}, None),
    ({"pair_two": 0}, None),
    ({"fuse": 0}, None),
    ({"half": 2, "half_fused": 2}, None),
    ({"half": 2, "half_fused": 0}, None),
    ({"quad": 1}, None),
    ({"walk": 2, "walk_len": 3}, 16384),
    ({"up3_poly": 0}, None),
    ({"fuse_hbconv": 1}, None),
    ({"fuse_latency": 0}, None),
    ({"pair_conv": 0}, None),
    ({"pair_solo": 0}, None),
    ({"pair_split": 0}, None),
    ({"pair_conv": 0, "fuse": 0}, None),
    ({"fuse_hbd": 0}, None),
]


def default_maxin(src, dst, tb):
    m = 4096 if tb >= 2.0 else 8192
    r = src / dst
    while r >= 3.5:
        m, r = m * 2, r / 2.0
    return m


_EMUL = None


def _emul():
    global _EMUL
    if _EMUL is None:
        import cases
        _EMUL = cases.emul_lib(test_hooks=True)
    return _EMUL


def launched(src, dst, maxin, tb, att, phase, opts, nch=3, with_poly=False):
    """[(stage, symbol)] of the fast-path launches of whole calls of noise, and the samples fed per channel; None where
    the library refuses to BUILD the chain (or the chain cannot serve the census).  A chain that was built and then fails in a call -- a launcher that refuses
    an instance as not built, or any other exception -- raises ChainFailed: the sweep counts it, never passes it over"""
    import importlib
    import numpy as np
    from nonfinite_cases import chain_geometry
    r8b = importlib.import_module("r8brain-free-src_amd")
    try:
        b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=nch, phase=phase, lib=_emul())
        for k, v in opts.items():
            b.set_option(k, v)
        b.set_option("timing", 1)
        desc = b.describe()
        if "BlockConvolver" not in desc:
            return None
        # (the reference's polynomial interpolator depends on the cut into calls by 1e-11, and the engine follows it call by
        # call: such a chain cannot serve the census' second-cut check.  It runs all the same -- it must not fail -- and
        # what it launched is reported only with with_poly set)
        credit = with_poly or "whole=0" not in desc
        lines = [l for l in desc.splitlines() if l.strip()]
        delayed = phase == 1 and input_delayed(lines, att)
        block_src, _, _ = chain_geometry(desc, src)
    except (RuntimeError, AssertionError):
        return None
    ncalls = max(2, int(math.ceil(3.2 * block_src / maxin)))
    rng = np.random.default_rng(5)
    seen = set()
    try:
        for _ in range(ncalls):
            b.process_host(rng.uniform(-1.0, 1.0, (nch, maxin)))
            for s, sym in enumerate(b.stage_symbols()):
                # (a stage's symbol is its convolver's; the half-band front -- mode 20 -- reports at the decimator it took in)
                if sym.startswith(FAMILIES) and (lines[s].startswith("BlockConvolver") or
                                                 (opts.get("fuse_hbconv") and ", 20, " in sym)):
                    seen.add((s, sym))
    except Exception as e:
        raise ChainFailed("%r -> %r MaxInLen %d tb %r att %r phase %d options %r: %s: %s" % (
            src, dst, maxin, tb, att, phase, opts, type(e).__name__, e))
    return (sorted(seen), ncalls * maxin, delayed) if credit else None


class ChainFailed(Exception):
    """a chain the library built that did not run: the message names the chain and what the launcher said"""


def input_delayed(lines, att):
    """a minimum-phase chain whose FIRST stage is a convolver that decimates by 2 or 4 in the spectrum: whether the filter's
    latency is no multiple of the factor.  The reference then delays its input (CDSPBlockConvolver.h:124-138, InputDelay),
    which moves its blocks against the engine's and with them the residue of the spectrum truncation -- at the filter's
    stop-band level, far above 1e-15 for the short filters.  Such a chain serves the census only where no other reaches
    the instance, and its entry carries input_delay=True (the stated exception of test_emul.run_minphase_reference_taps)"""
    import ctypes as C
    m = re.match(r"BlockConvolver: .* io=(\d+)/(\d+) .* nfreq=([\d.e-]+) tb=([\d.e-]+) gain=([\d.e-]+)", lines[0])
    if not m:
        return False
    down = int(m.group(2))
    if down not in (2, 4):
        return False
    bb, la, lf = C.c_int(), C.c_int(), C.c_double()
    _emul().r8b_design_lpfilter_ex(float(m.group(3)), float(m.group(4)), att, float(m.group(5)), 1, bb, la, lf, None, 0)
    return la.value % down != 0


def _work(job):
    fine, oi, ri = job
    opts, maxin_o = OPTION_SETS[oi]
    src, dst = (FINE_RATIOS if fine else GRID_RATIOS)[ri]
    o = dict(PIN)
    o.update(opts)
    best, chains, failed = {}, 0, []
    for phase in GRID_PHASE:
        for tb in FINE_TB if fine else GRID_TB:
            for att in FINE_ATT if fine else GRID_ATT:
                maxin = maxin_o or default_maxin(src, dst, tb)
                chains += 1
                try:
                    res = launched(src, dst, maxin, tb, att, phase, o)
                except ChainFailed as e:
                    failed.append(str(e))
                    continue
                if res is None:
                    continue
                for s, sym in res[0]:
                    key = (oi, phase, res[2], res[1] * max(1.0, dst / src), fine, ri)
                    if sym not in best or key < best[sym][0]:
                        best[sym] = (key, (sym, src, dst, maxin, tb, att, phase, opts, s, res[2]))
    return best, chains, failed


def sweep(jobs, part="all"):
    import multiprocessing as mp
    import time
    _emul()   # (built once, before the workers start)
    t0 = time.time()
    work = []
    if part in ("all", "coarse"):
        work += [(0, oi, ri) for oi in range(len(OPTION_SETS)) for ri in range(len(GRID_RATIOS))]
    if part in ("all", "fine"):
        work += [(1, oi, ri) for oi in FINE_SETS for ri in range(len(FINE_RATIOS))]
    best, chains, failed = {}, 0, []
    with mp.Pool(jobs) as pool:
        for b, n, f in pool.imap_unordered(_work, work):
            chains += n
            failed += f
            for sym, v in b.items():
                if sym not in best or v[0] < best[sym][0]:
                    best[sym] = v
    return best, chains, failed, time.time() - t0


def entry_line(e):
    sym, src, dst, maxin, tb, att, phase, opts, s, delayed = e
    o = ", {%s}" % ", ".join('"%s": %d' % kv for kv in sorted(opts.items())) if opts else ""
    if delayed:
        o = (o or ", None") + ", input_delay=True"
    return '    _run("%s", %r, %r, %d, %r, %r, %d, %d%s),' % (sym, src, dst, maxin, tb, att, phase, s, o)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--list", metavar="LIB")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--jobs", type=int, default=min(16, len(os.sched_getaffinity(0))))
    ap.add_argument("--only")
    ap.add_argument("--part", choices=("all", "coarse", "fine"), default="all")
    a = ap.parse_args()
    if a.list:
        for s in list_instances(a.list):
            print(s)
        return 0
    if a.sweep:
        best, chains, failed, secs = sweep(a.jobs, a.part)
        built = list_instances(os.path.join(ROOT, "tests", "emul", "_build", "libr8bsrc_emul.so"))
        print("# %d chains in %.0f s on %d processes" % (chains, secs, a.jobs))
        for sym in sorted(best, key=sort_key):
            if a.only is None or a.only in sym:
                print(entry_line(best[sym][1]))
        missed = [s for s in built if s not in best]
        print("# not reached: %d of %d" % (len(missed), len(built)))
        for s in missed:
            print("#   " + s)
        extra = [s for s in best if s not in built]
        if extra:
            print("# launched but not listed by --list: %s" % extra)
        print("# chains that were built and did not run: %d" % len(failed))
        for f in failed:
            print("#   FAILED " + f)
        return 1 if failed else 0
    ap.print_help()
    return 2


if __name__ == "__main__":
    sys.exit(main())
