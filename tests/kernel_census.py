"""The census of the compile-time-sized convolver kernels: one entry per compiled instance of k_convp<LN, UL, MODE, FLENP>,
k_convp_walk<...>, k_convq and k_convx<LOGN, UPLOG, MODE, FLENP> (r8b_dispatch.h decides which of them a launch runs;
Engine::resolve_forms() which mode a stage asks for).  Shared by the emulation tier (CPU) and the GPU tier
(tests/test_kernel_census.py) and, through --dump, by the sanitizer program tests/cxx_kernel_census.cpp.

An entry is one of two kinds:
  RUNS         a chain that launches the instance: the symbol exactly as stage_symbols() prints it, src, dst, MaxInLen,
               transition band, attenuation, phase, the stage that runs it, engine options.  Default options wherever
               the instance is what a chain runs by default; an entry with options is an opt-in (or opt-out) form and
               names the option.  Every entry pins half / half_fused / walk (_PIN), so that it does not depend on the
               channel count.  Authored by `python tools/kernel_census.py --sweep`.
  NOT_BUILT    an instance the dispatchers' geometry and mode lists name that no chain launches: the sweep's grid reaches
               it in no chain, and the cited rule excludes it for every geometry / mode the planner (r8b_design.cpp
               build_topology) and Engine::resolve_forms() produce.  r8b_dispatch.h convp_instance_built /
               convx_instance_built state the same rules, so no kernel is compiled for it and the launcher refuses it
               by its symbol ("... is not built"); the list keeps the reasons and checks that none comes back.

check_instance() runs one RUNS entry -- see its docstring.

python tests/kernel_census.py --dump   the RUNS entries as lines symbol|src|dst|maxin|tb|atten|phase|stage|options"""
import math
import re
import sys

# every form pinned by its options whatever the channel count (large objects take the half-array forms by default)
_PIN = {"half": 0, "half_fused": 0, "walk": 0}


def _run(symbol, src, dst, maxin, tb, att, phase, stage, opts=None, input_delay=False):
    o = dict(_PIN)
    o.update(opts or {})
    return dict(symbol=symbol, src=src, dst=dst, maxin=maxin, tb=tb, att=att, phase=phase, stage=stage, opts=o,
                opt_in=dict(opts or {}), input_delay=input_delay)


def _not_built(symbols, reason, cite):
    return [dict(symbol=s, reason=reason, cite=cite) for s in symbols]


def _syms(base, lns, ul, modes, flenp=24):
    return ["%s<%d, %d, %d, %d>" % (base, ln, ul, m, flenp) for ln in lns for m in modes]


# symbol, src, dst, MaxInLen, transition band, attenuation, phase (1: minimum phase), stage[, the options of an opt-in form]
RUNS = [
    _run("k_convp<5, 1, 0, 24>", 48000.0, 44100.0, 4096, 45.0, 49.0, 0, 0),
    _run("k_convp<5, 1, 3, 24>", 48000.0, 32000.0, 4096, 45.0, 49.0, 0, 0),
    _run("k_convp<5, 1, 6, 24>", 48000.0, 44100.0, 4096, 45.0, 49.0, 1, 0),
    _run("k_convp<5, 1, 7, 24>", 48000.0, 32000.0, 4096, 45.0, 49.0, 1, 0),
    _run("k_convp<6, -1, 0, 24>", 88200.0, 44100.0, 4096, 45.0, 49.0, 0, 0),
    _run("k_convp<6, -1, 3, 24>", 32000.0, 48000.0, 4096, 45.0, 49.0, 0, 0),
    _run("k_convp<6, -1, 6, 24>", 88200.0, 44100.0, 4096, 45.0, 80.0, 1, 0),
    _run("k_convp<6, -1, 7, 24>", 32000.0, 48000.0, 4096, 40.0, 49.0, 1, 0),
    _run("k_convp<6, 0, 0, 24>", 96000.0, 44100.0, 4096, 45.0, 49.0, 0, 0),
    _run("k_convp<6, 0, 3, 24>", 96000.0, 32000.0, 4096, 45.0, 49.0, 0, 0),
    _run("k_convp<6, 0, 6, 24>", 96000.0, 44100.0, 4096, 45.0, 49.0, 1, 0),
    _run("k_convp<6, 0, 7, 24>", 96000.0, 32000.0, 4096, 45.0, 49.0, 1, 0),
    _run("k_convp<6, 1, 0, 24>", 48000.0, 44100.0, 4096, 45.0, 160.0, 0, 0),
    _run("k_convp<6, 1, 1, 24>", 48000.0, 44100.0, 4096, 45.0, 109.56, 0, 0),
    _run("k_convp<6, 1, 3, 24>", 48000.0, 32000.0, 4096, 45.0, 60.0, 0, 0),
    _run("k_convp<6, 1, 6, 24>", 48000.0, 44100.0, 4096, 45.0, 109.56, 1, 0),
    _run("k_convp<6, 1, 7, 24>", 48000.0, 32000.0, 4096, 45.0, 60.0, 1, 0),
    _run("k_convp<7, -2, 3, 24>", 64000.0, 48000.0, 4096, 45.0, 49.0, 0, 0),
    _run("k_convp<7, -2, 7, 24>", 64000.0, 48000.0, 4096, 45.0, 60.0, 1, 0),
    _run("k_convp<7, -1, 0, 24>", 88200.0, 44100.0, 4096, 45.0, 109.56, 0, 0),
    _run("k_convp<7, -1, 3, 24>", 32000.0, 48000.0, 4096, 45.0, 60.0, 0, 0),
    _run("k_convp<7, -1, 6, 24>", 88200.0, 44100.0, 4096, 45.0, 136.45, 1, 0),
    _run("k_convp<7, -1, 7, 24>", 32000.0, 48000.0, 4096, 45.0, 60.0, 1, 0),
    _run("k_convp<7, 0, 0, 24>", 96000.0, 44100.0, 4096, 45.0, 160.0, 0, 0),
    _run("k_convp<7, 0, 1, 24>", 96000.0, 44100.0, 4096, 45.0, 109.56, 0, 0),
    _run("k_convp<7, 0, 3, 24>", 96000.0, 32000.0, 4096, 45.0, 60.0, 0, 0),
    _run("k_convp<7, 0, 6, 24>", 96000.0, 44100.0, 4096, 45.0, 109.56, 1, 0),
    _run("k_convp<7, 0, 7, 24>", 96000.0, 32000.0, 4096, 45.0, 60.0, 1, 0),
    _run("k_convp<7, 1, 0, 24>", 44100.0, 88200.0, 4096, 45.0, 206.91, 0, 0),
    _run("k_convp<7, 1, 1, 24>", 48000.0, 44100.0, 4096, 45.0, 180.15, 0, 0),
    _run("k_convp<7, 1, 1, 32>", 48000.0, 44100.0, 4096, 45.0, 206.91, 0, 0),
    _run("k_convp<7, 1, 3, 24>", 48000.0, 32000.0, 4096, 45.0, 136.45, 0, 0),
    _run("k_convp<7, 1, 4, 24>", 48000.0, 57600.0, 4096, 30.0, 180.15, 0, 0),
    _run("k_convp<7, 1, 5, 24>", 48000.0, 40000.0, 4096, 35.0, 180.15, 0, 0),
    _run("k_convp<7, 1, 6, 24>", 48000.0, 44100.0, 4096, 45.0, 180.15, 1, 0),
    _run("k_convp<7, 1, 7, 24>", 48000.0, 32000.0, 4096, 45.0, 136.45, 1, 0),
    _run("k_convp<7, 1, 16, 24>", 48000.0, 57600.0, 4096, 30.0, 180.15, 1, 0),
    _run("k_convp<7, 1, 17, 24>", 48000.0, 40000.0, 4096, 35.0, 180.15, 1, 0),
    _run("k_convp<8, -2, 3, 24>", 64000.0, 48000.0, 4096, 45.0, 109.56, 0, 0),
    _run("k_convp<8, -2, 7, 24>", 64000.0, 48000.0, 4096, 45.0, 136.45, 1, 0),
    _run("k_convp<8, -1, 0, 24>", 88200.0, 44100.0, 4096, 45.0, 206.91, 0, 0),
    _run("k_convp<8, -1, 3, 24>", 32000.0, 48000.0, 4096, 45.0, 136.45, 0, 0),
    _run("k_convp<8, -1, 6, 24>", 88200.0, 44100.0, 4096, 45.0, 206.91, 1, 0),
    _run("k_convp<8, -1, 7, 24>", 32000.0, 48000.0, 4096, 45.0, 120.0, 1, 0),
    _run("k_convp<8, 0, 0, 24>", 96000.0, 44100.0, 4096, 45.0, 180.15, 0, 0, {"fuse": 0}),
    _run("k_convp<8, 0, 1, 24>", 96000.0, 44100.0, 4096, 45.0, 180.15, 0, 0),
    _run("k_convp<8, 0, 1, 32>", 96000.0, 44100.0, 4096, 45.0, 206.91, 0, 0),
    _run("k_convp<8, 0, 3, 24>", 96000.0, 32000.0, 4096, 45.0, 136.45, 0, 0),
    _run("k_convp<8, 0, 5, 24>", 100000.0, 40000.0, 4096, 40.0, 180.15, 0, 0),
    _run("k_convp<8, 0, 6, 24>", 96000.0, 44100.0, 4096, 45.0, 180.15, 1, 0),
    _run("k_convp<8, 0, 7, 24>", 96000.0, 32000.0, 4096, 45.0, 136.45, 1, 0),
    _run("k_convp<8, 0, 17, 24>", 100000.0, 40000.0, 4096, 40.0, 180.15, 1, 0),
    _run("k_convp<8, 1, 0, 24>", 44100.0, 88200.0, 4096, 20.0, 180.15, 0, 0),
    _run("k_convp<8, 1, 1, 24>", 48000.0, 44100.0, 4096, 20.0, 160.0, 0, 0),
    _run("k_convp<8, 1, 1, 32>", 48000.0, 44100.0, 4096, 20.0, 206.91, 0, 0),
    _run("k_convp<8, 1, 3, 24>", 48000.0, 32000.0, 4096, 30.0, 180.15, 0, 0),
    _run("k_convp<8, 1, 4, 24>", 48000.0, 57600.0, 4096, 20.0, 180.15, 0, 0),
    _run("k_convp<8, 1, 5, 24>", 48000.0, 40000.0, 4096, 25.0, 180.15, 0, 0),
    _run("k_convp<8, 1, 6, 24>", 48000.0, 44100.0, 4096, 20.0, 160.0, 1, 0),
    _run("k_convp<8, 1, 7, 24>", 48000.0, 32000.0, 4096, 30.0, 180.15, 1, 0),
    _run("k_convp<8, 1, 16, 24>", 48000.0, 57600.0, 4096, 20.0, 180.15, 1, 0),
    _run("k_convp<8, 1, 17, 24>", 48000.0, 40000.0, 4096, 25.0, 180.15, 1, 0),
    _run("k_convp<9, -2, 3, 24>", 64000.0, 48000.0, 4096, 45.0, 206.91, 0, 0),
    _run("k_convp<9, -2, 7, 24>", 64000.0, 48000.0, 4096, 45.0, 218.0, 1, 0),
    _run("k_convp<9, -1, 0, 24>", 88200.0, 44100.0, 4096, 20.0, 180.15, 0, 0),
    _run("k_convp<9, -1, 3, 24>", 32000.0, 48000.0, 4096, 30.0, 180.15, 0, 0),
    _run("k_convp<9, -1, 6, 24>", 88200.0, 44100.0, 4096, 20.0, 180.15, 1, 0),
    _run("k_convp<9, -1, 7, 24>", 32000.0, 48000.0, 4096, 30.0, 180.15, 1, 0),
    _run("k_convp<9, 0, 0, 24>", 96000.0, 44100.0, 4096, 20.0, 160.0, 0, 0, {"fuse": 0}),
    _run("k_convp<9, 0, 1, 24>", 96000.0, 44100.0, 4096, 20.0, 160.0, 0, 0),
    _run("k_convp<9, 0, 1, 32>", 96000.0, 44100.0, 4096, 20.0, 206.91, 0, 0),
    _run("k_convp<9, 0, 3, 24>", 96000.0, 32000.0, 4096, 30.0, 180.15, 0, 0),
    _run("k_convp<9, 0, 5, 24>", 100000.0, 40000.0, 4096, 25.0, 180.15, 0, 0),
    _run("k_convp<9, 0, 6, 24>", 96000.0, 44100.0, 4096, 20.0, 160.0, 1, 0),
    _run("k_convp<9, 0, 7, 24>", 96000.0, 32000.0, 4096, 30.0, 180.15, 1, 0),
    _run("k_convp<9, 0, 17, 24>", 100000.0, 40000.0, 4096, 25.0, 180.15, 1, 0),
    _run("k_convp<9, 1, 0, 24>", 44100.0, 88200.0, 4096, 10.0, 180.15, 0, 0),
    _run("k_convp<9, 1, 1, 24>", 48000.0, 44100.0, 4096, 10.0, 160.0, 0, 0),
    _run("k_convp<9, 1, 1, 32>", 48000.0, 44100.0, 4096, 10.0, 206.91, 0, 0),
    _run("k_convp<9, 1, 3, 24>", 48000.0, 32000.0, 4096, 20.0, 218.0, 0, 0),
    _run("k_convp<9, 1, 4, 24>", 48000.0, 57600.0, 4096, 10.0, 180.15, 0, 0),
    _run("k_convp<9, 1, 5, 24>", 48000.0, 40000.0, 4096, 10.0, 136.45, 0, 0),
    _run("k_convp<9, 1, 6, 24>", 48000.0, 44100.0, 4096, 10.0, 160.0, 1, 0),
    _run("k_convp<9, 1, 7, 24>", 48000.0, 32000.0, 4096, 20.0, 218.0, 1, 0),
    _run("k_convp<9, 1, 16, 24>", 48000.0, 57600.0, 4096, 10.0, 180.15, 1, 0),
    _run("k_convp<9, 1, 17, 24>", 48000.0, 40000.0, 4096, 10.0, 136.45, 1, 0),
    _run("k_convp<10, -2, 3, 24>", 64000.0, 48000.0, 4096, 20.0, 180.15, 0, 0),
    _run("k_convp<10, -2, 7, 24>", 64000.0, 48000.0, 4096, 5.0, 49.0, 1, 0),
    _run("k_convp<10, -1, 0, 24>", 88200.0, 44100.0, 4096, 10.0, 180.15, 0, 0),
    _run("k_convp<10, -1, 3, 24>", 32000.0, 48000.0, 4096, 20.0, 218.0, 0, 0),
    _run("k_convp<10, -1, 6, 24>", 88200.0, 44100.0, 4096, 10.0, 180.15, 1, 0),
    _run("k_convp<10, -1, 7, 24>", 32000.0, 48000.0, 4096, 20.0, 218.0, 1, 0),
    _run("k_convp<10, 0, 0, 24>", 96000.0, 44100.0, 4096, 10.0, 160.0, 0, 0, {"fuse": 0}),
    _run("k_convp<10, 0, 1, 24>", 96000.0, 44100.0, 4096, 10.0, 160.0, 0, 0),
    _run("k_convp<10, 0, 1, 32>", 96000.0, 44100.0, 4096, 10.0, 206.91, 0, 0),
    _run("k_convp<10, 0, 3, 24>", 96000.0, 32000.0, 4096, 20.0, 218.0, 0, 0),
    _run("k_convp<10, 0, 5, 24>", 100000.0, 40000.0, 4096, 10.0, 136.45, 0, 0),
    _run("k_convp<10, 0, 6, 24>", 96000.0, 44100.0, 4096, 10.0, 160.0, 1, 0),
    _run("k_convp<10, 0, 7, 24>", 96000.0, 32000.0, 4096, 20.0, 218.0, 1, 0),
    _run("k_convp<10, 0, 17, 24>", 100000.0, 40000.0, 4096, 10.0, 136.45, 1, 0),
    _run("k_convp<10, 0, 19, 24>", 44100.0, 132300.0, 4096, 3.0, 136.45, 0, 0),
    _run("k_convp<10, 1, 0, 24>", 44100.0, 88200.0, 4096, 5.0, 180.15, 0, 0),
    _run("k_convp<10, 1, 1, 24>", 48000.0, 44100.0, 4096, 5.0, 160.0, 0, 0),
    _run("k_convp<10, 1, 1, 32>", 48000.0, 44100.0, 4096, 5.0, 206.91, 0, 0),
    _run("k_convp<10, 1, 3, 24>", 48000.0, 32000.0, 4096, 10.0, 218.0, 0, 0),
    _run("k_convp<10, 1, 4, 24>", 48000.0, 57600.0, 4096, 5.0, 180.15, 0, 0),
    _run("k_convp<10, 1, 5, 24>", 48000.0, 44100.0, 4096, 3.0, 136.45, 0, 0),
    _run("k_convp<10, 1, 6, 24>", 48000.0, 44100.0, 4096, 5.0, 160.0, 1, 0),
    _run("k_convp<10, 1, 7, 24>", 48000.0, 32000.0, 4096, 10.0, 218.0, 1, 0),
    _run("k_convp<10, 1, 16, 24>", 48000.0, 57600.0, 4096, 5.0, 180.15, 1, 0),
    _run("k_convp<10, 1, 17, 24>", 48000.0, 44100.0, 4096, 3.0, 136.45, 1, 0),
    _run("k_convp<11, -2, 3, 24>", 64000.0, 48000.0, 4096, 10.0, 180.15, 0, 0),
    _run("k_convp<11, -2, 7, 24>", 64000.0, 48000.0, 4096, 10.0, 180.15, 1, 0),
    _run("k_convp<11, -1, 0, 24>", 88200.0, 44100.0, 4096, 5.0, 180.15, 0, 0),
    _run("k_convp<11, -1, 3, 24>", 32000.0, 48000.0, 4096, 10.0, 218.0, 0, 0),
    _run("k_convp<11, -1, 6, 24>", 88200.0, 44100.0, 4096, 5.0, 180.15, 1, 0),
    _run("k_convp<11, -1, 7, 24>", 32000.0, 48000.0, 4096, 10.0, 218.0, 1, 0),
    _run("k_convp<11, 0, 0, 24>", 96000.0, 44100.0, 4096, 5.0, 160.0, 0, 0, {"fuse": 0}),
    _run("k_convp<11, 0, 1, 24>", 96000.0, 44100.0, 4096, 5.0, 160.0, 0, 0),
    _run("k_convp<11, 0, 1, 32>", 96000.0, 44100.0, 4096, 5.0, 206.91, 0, 0),
    _run("k_convp<11, 0, 3, 24>", 96000.0, 32000.0, 4096, 10.0, 218.0, 0, 0),
    _run("k_convp<11, 0, 5, 24>", 96000.0, 44100.0, 4096, 3.0, 136.45, 0, 0),
    _run("k_convp<11, 0, 6, 24>", 96000.0, 44100.0, 4096, 5.0, 160.0, 1, 0),
    _run("k_convp<11, 0, 7, 24>", 96000.0, 32000.0, 4096, 10.0, 218.0, 1, 0),
    _run("k_convp<11, 0, 17, 24>", 96000.0, 44100.0, 4096, 3.0, 136.45, 1, 0),
    _run("k_convp<11, 0, 19, 24>", 44100.0, 132300.0, 4096, 2.0, 180.15, 0, 0),
    _run("k_convp<11, 1, 0, 24>", 44100.0, 88200.0, 4096, 3.0, 206.91, 0, 0),
    _run("k_convp<11, 1, 1, 24>", 88200.0, 48000.0, 4096, 5.0, 180.15, 0, 0),
    _run("k_convp<11, 1, 1, 32>", 48000.0, 44100.0, 4096, 3.0, 206.91, 0, 0),
    _run("k_convp<11, 1, 3, 24>", 48000.0, 32000.0, 4096, 3.0, 136.45, 0, 0),
    _run("k_convp<11, 1, 4, 24>", 48000.0, 57600.0, 4096, 2.0, 136.45, 0, 0),
    _run("k_convp<11, 1, 5, 24>", 48000.0, 44100.0, 4096, 3.0, 180.15, 0, 0),
    _run("k_convp<11, 1, 6, 24>", 48000.0, 44100.0, 4096, 3.0, 206.91, 1, 0),
    _run("k_convp<11, 1, 7, 24>", 48000.0, 32000.0, 4096, 3.0, 136.45, 1, 0),
    _run("k_convp<11, 1, 16, 24>", 48000.0, 57600.0, 4096, 2.0, 136.45, 1, 0),
    _run("k_convp<11, 1, 17, 24>", 48000.0, 44100.0, 4096, 3.0, 180.15, 1, 0),
    _run("k_convp<11, 1, 21, 24>", 44100.0, 88200.0, 4096, 3.0, 206.91, 0, 0, {"half": 2, "half_fused": 2}),
    _run("k_convp<11, 1, 22, 24>", 48000.0, 32000.0, 4096, 3.0, 136.45, 0, 0, {"half": 2, "half_fused": 2}),
    _run("k_convp<11, 1, 23, 24>", 44100.0, 96000.0, 4096, 2.0, 160.0, 0, 0, {"half": 2, "half_fused": 2}),
    _run("k_convp<11, 1, 25, 24>", 48000.0, 44100.0, 4096, 2.0, 180.15, 0, 0, {"half": 2, "half_fused": 2}),
    _run("k_convp<11, 1, 29, 24>", 44100.0, 96000.0, 4096, 2.0, 160.0, 1, 0, {"half": 2, "half_fused": 2}),
    _run("k_convp<11, 1, 30, 24>", 48000.0, 44100.0, 4096, 2.0, 180.15, 1, 0, {"half": 2, "half_fused": 2}),
    _run("k_convp<11, 1, 31, 24>", 48000.0, 44100.0, 4096, 3.0, 206.91, 1, 0, {"half": 2, "half_fused": 2}),
    _run("k_convp<11, 1, 32, 24>", 48000.0, 32000.0, 4096, 3.0, 136.45, 1, 0, {"half": 2, "half_fused": 2}),
    _run("k_convp<12, -2, 3, 24>", 64000.0, 48000.0, 4096, 5.0, 180.15, 0, 0),
    _run("k_convp<12, -2, 7, 24>", 64000.0, 48000.0, 4096, 5.0, 180.15, 1, 0),
    _run("k_convp<12, -1, 0, 24>", 88200.0, 44100.0, 4096, 2.0, 206.91, 0, 0),
    _run("k_convp<12, -1, 3, 24>", 32000.0, 48000.0, 4096, 3.0, 136.45, 0, 0),
    _run("k_convp<12, -1, 6, 24>", 88200.0, 44100.0, 4096, 2.0, 136.45, 1, 0),
    _run("k_convp<12, -1, 7, 24>", 32000.0, 48000.0, 4096, 3.0, 180.15, 1, 0),
    _run("k_convp<12, -1, 20, 24>", 176400.0, 44100.0, 8192, 2.0, 206.91, 0, 0, {"fuse_hbconv": 1}),
    _run("k_convp<12, -1, 27, 24>", 88200.0, 44100.0, 4096, 2.0, 206.91, 0, 0, {"half": 2, "half_fused": 2}),
    _run("k_convp<12, -1, 28, 24>", 32000.0, 48000.0, 4096, 3.0, 136.45, 0, 0, {"half": 2, "half_fused": 2}),
    _run("k_convp<12, 0, 0, 24>", 96000.0, 44100.0, 4096, 2.0, 180.15, 0, 0, {"fuse": 0}),
    _run("k_convp<12, 0, 1, 24>", 96000.0, 44100.0, 4096, 2.0, 180.15, 0, 0, {"pair_two": 0}),
    _run("k_convp<12, 0, 1, 32>", 96000.0, 44100.0, 4096, 2.0, 206.91, 0, 0),
    _run("k_convp<12, 0, 3, 24>", 96000.0, 32000.0, 4096, 3.0, 206.91, 0, 0),
    _run("k_convp<12, 0, 5, 24>", 96000.0, 44100.0, 4096, 2.0, 180.15, 0, 0),
    _run("k_convp<12, 0, 6, 24>", 96000.0, 44100.0, 4096, 2.0, 206.91, 1, 0),
    _run("k_convp<12, 0, 7, 24>", 96000.0, 32000.0, 4096, 3.0, 206.91, 1, 0),
    _run("k_convp<12, 0, 17, 24>", 96000.0, 44100.0, 4096, 2.0, 180.15, 1, 0),
    _run("k_convp<12, 0, 19, 24>", 44100.0, 132300.0, 8192, 1.0, 180.15, 0, 0),
    _run("k_convp<12, 0, 33, 24>", 96000.0, 44100.0, 4096, 2.0, 180.15, 0, 0, {"half": 2, "half_fused": 2}),
    _run("k_convp<12, 1, 0, 24>", 44100.0, 88200.0, 8192, 1.4, 206.91, 0, 0),
    _run("k_convp<12, 1, 1, 24>", 88200.0, 48000.0, 4096, 2.0, 160.0, 0, 0),
    _run("k_convp<12, 1, 1, 32>", 88200.0, 48000.0, 4096, 2.0, 218.0, 0, 0),
    _run("k_convp<12, 1, 3, 24>", 48000.0, 32000.0, 4096, 2.0, 180.15, 0, 0),
    _run("k_convp<12, 1, 4, 24>", 44100.0, 96000.0, 8192, 1.0, 136.45, 0, 0),
    _run("k_convp<12, 1, 5, 24>", 48000.0, 44100.0, 8192, 1.4, 180.15, 0, 0),
    _run("k_convp<12, 1, 6, 24>", 88200.0, 48000.0, 4096, 2.0, 218.0, 1, 0),
    _run("k_convp<12, 1, 7, 24>", 48000.0, 32000.0, 4096, 2.0, 180.15, 1, 0),
    _run("k_convp<12, 1, 16, 24>", 44100.0, 96000.0, 8192, 1.0, 136.45, 1, 0),
    _run("k_convp<12, 1, 17, 24>", 48000.0, 44100.0, 8192, 1.4, 180.15, 1, 0),
    _run("k_convp<12, 1, 21, 24>", 44100.0, 88200.0, 8192, 1.4, 206.91, 0, 0, {"half": 2, "half_fused": 2}),
    _run("k_convp<12, 1, 22, 24>", 48000.0, 32000.0, 4096, 2.0, 180.15, 0, 0, {"half": 2, "half_fused": 2}),
    _run("k_convp<12, 1, 31, 24>", 88200.0, 48000.0, 4096, 2.0, 218.0, 1, 0, {"half": 2, "half_fused": 2}),
    _run("k_convp<12, 1, 32, 24>", 48000.0, 32000.0, 4096, 2.0, 180.15, 1, 0, {"half": 2, "half_fused": 2}),
    _run("k_convp<13, -2, 3, 24>", 64000.0, 48000.0, 4096, 3.0, 206.91, 0, 0),
    _run("k_convp<13, -2, 7, 24>", 64000.0, 48000.0, 4096, 2.0, 136.45, 1, 0),
    _run("k_convp<13, -2, 11, 24>", 64000.0, 48000.0, 8192, 1.4, 206.91, 0, 0),
    _run("k_convp<13, -1, 0, 24>", 88200.0, 44100.0, 8192, 1.0, 206.91, 0, 0),
    _run("k_convp<13, -1, 3, 24>", 32000.0, 48000.0, 4096, 2.0, 180.15, 0, 0),
    _run("k_convp<13, -1, 6, 24>", 88200.0, 44100.0, 8192, 1.0, 218.0, 1, 0),
    _run("k_convp<13, -1, 7, 24>", 32000.0, 48000.0, 4096, 2.0, 180.15, 1, 0),
    _run("k_convp<13, -1, 10, 24>", 88200.0, 44100.0, 8192, 0.5, 206.91, 0, 0),
    _run("k_convp<13, -1, 11, 24>", 32000.0, 48000.0, 8192, 1.0, 180.15, 0, 0),
    _run("k_convp<13, -1, 14, 24>", 88200.0, 44100.0, 8192, 0.5, 206.91, 1, 0),
    _run("k_convp<13, -1, 15, 24>", 32000.0, 48000.0, 8192, 0.7, 136.45, 1, 0),
    _run("k_convp<13, 0, 0, 24>", 96000.0, 44100.0, 8192, 1.0, 180.15, 0, 0, {"fuse": 0}),
    _run("k_convp<13, 0, 1, 24>", 96000.0, 44100.0, 8192, 1.0, 180.15, 0, 0, {"pair_two": 0}),
    _run("k_convp<13, 0, 1, 32>", 96000.0, 44100.0, 8192, 1.0, 206.91, 0, 0),
    _run("k_convp<13, 0, 3, 24>", 96000.0, 32000.0, 8192, 1.4, 206.91, 0, 0),
    _run("k_convp<13, 0, 5, 24>", 96000.0, 44100.0, 8192, 1.0, 180.15, 0, 0),
    _run("k_convp<13, 0, 6, 24>", 96000.0, 44100.0, 8192, 1.0, 206.91, 1, 0),
    _run("k_convp<13, 0, 7, 24>", 96000.0, 32000.0, 8192, 1.4, 206.91, 1, 0),
    _run("k_convp<13, 0, 8, 24>", 48000.0, 44100.0, 8192, 0.5, 180.15, 0, 0),
    _run("k_convp<13, 0, 9, 24>", 48000.0, 32000.0, 8192, 0.7, 206.91, 0, 0),
    _run("k_convp<13, 0, 10, 24>", 96000.0, 44100.0, 8192, 0.5, 180.15, 0, 0, {"fuse": 0}),
    _run("k_convp<13, 0, 11, 24>", 96000.0, 32000.0, 8192, 0.7, 206.91, 0, 0),
    _run("k_convp<13, 0, 12, 24>", 48000.0, 44100.0, 8192, 0.5, 180.15, 1, 0),
    _run("k_convp<13, 0, 13, 24>", 48000.0, 32000.0, 8192, 0.7, 206.91, 1, 0),
    _run("k_convp<13, 0, 14, 24>", 96000.0, 44100.0, 8192, 0.5, 180.15, 1, 0),
    _run("k_convp<13, 0, 15, 24>", 96000.0, 32000.0, 8192, 0.7, 206.91, 1, 0),
    _run("k_convp<13, 0, 17, 24>", 96000.0, 44100.0, 8192, 1.0, 180.15, 1, 0),
    _run("k_convp<13, 0, 18, 24>", 96000.0, 44100.0, 8192, 0.5, 180.15, 0, 0),
    _run("k_convp<13, 0, 18, 32>", 96000.0, 44100.0, 8192, 0.5, 206.91, 0, 0),
    _run("k_convp_walk<11, 1, 4, 24>", 48000.0, 64000.0, 16384, 2.0, 136.45, 0, 0, {"walk": 2, "walk_len": 3}),
    _run("k_convp_walk<11, 1, 5, 24>", 44100.0, 50400.0, 16384, 2.0, 136.45, 0, 0, {"walk": 2, "walk_len": 3}),
    _run("k_convp_walk<11, 1, 16, 24>", 48000.0, 64000.0, 16384, 2.0, 136.45, 1, 0, {"walk": 2, "walk_len": 3}),
    _run("k_convp_walk<11, 1, 17, 24>", 44100.0, 50400.0, 16384, 2.0, 136.45, 1, 0, {"walk": 2, "walk_len": 3}),
    _run("k_convq", 44100.0, 88200.0, 4096, 3.0, 206.91, 0, 0, {"quad": 1}),
    _run("k_convx<8, -1, 0, 24>", 88200.0, 44100.0, 4096, 20.0, 180.15, 0, 0, {"pair_conv": 0}),
    _run("k_convx<8, -1, 3, 24>", 32000.0, 48000.0, 4096, 30.0, 180.15, 0, 0, {"pair_conv": 0}),
    _run("k_convx<8, 1, 0, 24>", 32000.0, 44100.0, 4096, 10.0, 180.15, 0, 0, {"pair_conv": 0}),
    _run("k_convx<8, 1, 1, 24>", 48000.0, 44100.0, 4096, 10.0, 160.0, 0, 0, {"pair_conv": 0}),
    _run("k_convx<8, 1, 1, 32>", 48000.0, 44100.0, 4096, 10.0, 206.91, 0, 0, {"pair_conv": 0}),
    _run("k_convx<8, 1, 3, 24>", 48000.0, 32000.0, 4096, 20.0, 218.0, 0, 0, {"pair_conv": 0}),
    _run("k_convx<9, -1, 0, 24>", 88200.0, 44100.0, 4096, 10.0, 180.15, 0, 0, {"pair_conv": 0}),
    _run("k_convx<9, -1, 3, 24>", 32000.0, 48000.0, 4096, 20.0, 218.0, 0, 0, {"pair_conv": 0}),
    _run("k_convx<9, 0, 0, 24>", 96000.0, 44100.0, 4096, 10.0, 160.0, 0, 0, {"fuse": 0, "pair_conv": 0}),
    _run("k_convx<9, 0, 1, 24>", 96000.0, 44100.0, 4096, 10.0, 160.0, 0, 0, {"pair_conv": 0}),
    _run("k_convx<9, 0, 1, 32>", 96000.0, 44100.0, 4096, 10.0, 206.91, 0, 0, {"pair_conv": 0}),
    _run("k_convx<9, 0, 3, 24>", 96000.0, 32000.0, 4096, 20.0, 218.0, 0, 0, {"pair_conv": 0}),
    _run("k_convx<9, 1, 0, 24>", 32000.0, 44100.0, 4096, 5.0, 180.15, 0, 0, {"pair_conv": 0}),
    _run("k_convx<9, 1, 1, 24>", 48000.0, 44100.0, 4096, 5.0, 160.0, 0, 0, {"pair_conv": 0}),
    _run("k_convx<9, 1, 1, 32>", 48000.0, 44100.0, 4096, 5.0, 206.91, 0, 0, {"pair_conv": 0}),
    _run("k_convx<9, 1, 3, 24>", 48000.0, 32000.0, 4096, 10.0, 218.0, 0, 0, {"pair_conv": 0}),
    _run("k_convx<10, -2, 3, 24>", 64000.0, 48000.0, 4096, 10.0, 180.15, 0, 0, {"pair_conv": 0}),
    _run("k_convx<10, -1, 0, 24>", 88200.0, 44100.0, 4096, 5.0, 180.15, 0, 0, {"pair_conv": 0}),
    _run("k_convx<10, -1, 3, 24>", 32000.0, 48000.0, 4096, 10.0, 218.0, 0, 0, {"pair_conv": 0}),
    _run("k_convx<10, 0, 0, 24>", 96000.0, 44100.0, 4096, 5.0, 160.0, 0, 0, {"fuse": 0, "pair_conv": 0}),
    _run("k_convx<10, 0, 1, 24>", 96000.0, 44100.0, 4096, 5.0, 160.0, 0, 0, {"pair_conv": 0}),
    _run("k_convx<10, 0, 1, 32>", 96000.0, 44100.0, 4096, 5.0, 206.91, 0, 0, {"pair_conv": 0}),
    _run("k_convx<10, 0, 3, 24>", 96000.0, 32000.0, 4096, 10.0, 218.0, 0, 0, {"pair_conv": 0}),
    _run("k_convx<10, 1, 0, 24>", 32000.0, 44100.0, 4096, 3.0, 206.91, 0, 0, {"pair_conv": 0}),
    _run("k_convx<10, 1, 1, 24>", 48000.0, 44100.0, 4096, 3.0, 180.15, 0, 0, {"pair_conv": 0}),
    _run("k_convx<10, 1, 1, 32>", 48000.0, 44100.0, 4096, 3.0, 206.91, 0, 0, {"pair_conv": 0}),
    _run("k_convx<10, 1, 3, 24>", 48000.0, 32000.0, 4096, 3.0, 136.45, 0, 0, {"pair_conv": 0}),
    _run("k_convx<11, -2, 3, 24>", 64000.0, 48000.0, 4096, 5.0, 180.15, 0, 0, {"pair_conv": 0}),
    _run("k_convx<11, -1, 0, 24>", 88200.0, 44100.0, 4096, 2.0, 206.91, 0, 0, {"pair_conv": 0}),
    _run("k_convx<11, -1, 3, 24>", 32000.0, 48000.0, 4096, 3.0, 136.45, 0, 0, {"pair_conv": 0}),
    _run("k_convx<11, 0, 0, 24>", 96000.0, 44100.0, 4096, 2.0, 180.15, 0, 0, {"fuse": 0, "pair_conv": 0}),
    _run("k_convx<11, 0, 1, 24>", 96000.0, 44100.0, 4096, 2.0, 180.15, 0, 0, {"pair_conv": 0}),
    _run("k_convx<11, 0, 1, 32>", 96000.0, 44100.0, 4096, 2.0, 206.91, 0, 0, {"pair_conv": 0}),
    _run("k_convx<11, 0, 3, 24>", 96000.0, 32000.0, 4096, 3.0, 206.91, 0, 0, {"pair_conv": 0}),
    _run("k_convx<11, 1, 0, 24>", 32000.0, 44100.0, 8192, 1.4, 206.91, 0, 0, {"pair_conv": 0}),
    _run("k_convx<11, 1, 1, 24>", 88200.0, 48000.0, 4096, 2.0, 160.0, 0, 0, {"pair_conv": 0}),
    _run("k_convx<11, 1, 1, 32>", 88200.0, 48000.0, 4096, 2.0, 218.0, 0, 0, {"pair_conv": 0}),
    _run("k_convx<11, 1, 3, 24>", 48000.0, 32000.0, 4096, 2.0, 180.15, 0, 0, {"pair_conv": 0}),
    _run("k_convx<12, -2, 3, 24>", 64000.0, 48000.0, 4096, 3.0, 206.91, 0, 0, {"pair_conv": 0}),
    _run("k_convx<12, -1, 0, 24>", 88200.0, 44100.0, 8192, 1.0, 206.91, 0, 0, {"pair_conv": 0}),
    _run("k_convx<12, -1, 3, 24>", 32000.0, 48000.0, 4096, 2.0, 180.15, 0, 0, {"pair_conv": 0}),
    _run("k_convx<12, 0, 0, 24>", 96000.0, 44100.0, 8192, 1.0, 180.15, 0, 0, {"fuse": 0, "pair_conv": 0}),
    _run("k_convx<12, 0, 1, 24>", 96000.0, 44100.0, 8192, 1.0, 180.15, 0, 0, {"pair_conv": 0}),
    _run("k_convx<12, 0, 1, 32>", 96000.0, 44100.0, 8192, 1.0, 206.91, 0, 0, {"pair_conv": 0}),
    _run("k_convx<12, 0, 3, 24>", 96000.0, 32000.0, 8192, 1.4, 206.91, 0, 0, {"pair_conv": 0}),
    _run("k_convx<12, 1, 0, 24>", 32000.0, 44100.0, 8192, 0.5, 206.91, 0, 0, {"pair_conv": 0}),
    _run("k_convx<12, 1, 1, 24>", 48000.0, 44100.0, 8192, 0.5, 180.15, 0, 0, {"pair_conv": 0}),
    _run("k_convx<12, 1, 1, 32>", 48000.0, 44100.0, 8192, 0.5, 206.91, 0, 0, {"pair_conv": 0}),
    _run("k_convx<12, 1, 3, 24>", 48000.0, 32000.0, 8192, 0.7, 206.91, 0, 0, {"pair_conv": 0}),
    _run("k_convx<13, -2, 3, 24>", 64000.0, 48000.0, 8192, 1.4, 206.91, 0, 0, {"pair_conv": 0}),
    _run("k_convx<13, -1, 0, 24>", 88200.0, 44100.0, 8192, 0.5, 206.91, 0, 0, {"pair_conv": 0}),
    _run("k_convx<13, -1, 3, 24>", 32000.0, 48000.0, 8192, 1.0, 180.15, 0, 0, {"pair_conv": 0}),
    _run("k_convx<13, 0, 0, 24>", 96000.0, 44100.0, 8192, 0.5, 180.15, 0, 0, {"fuse": 0, "pair_conv": 0}),
    _run("k_convx<13, 0, 1, 24>", 96000.0, 44100.0, 8192, 0.5, 180.15, 0, 0, {"pair_conv": 0}),
    _run("k_convx<13, 0, 1, 32>", 96000.0, 44100.0, 8192, 0.5, 206.91, 0, 0, {"pair_conv": 0}),
    _run("k_convx<13, 0, 3, 24>", 96000.0, 32000.0, 8192, 0.7, 206.91, 0, 0, {"pair_conv": 0}),
]

_ALL_LN = range(6, 14)
NOT_BUILT = (
    # 21: decimation by 4 in the spectrum WITHOUT the 3x zero stuffing in front
    _not_built(
        _syms("k_convp", _ALL_LN, -2, (0, 6)) + ["k_convp<13, -2, 10, 24>"] + _syms("k_convx", range(10, 14), -2, (0,)),
        "the planner decimates by 4 only in the ratio 3/4 (r8b_design.cpp build_topology: of the one-convolver ratios 1/2, "
        "1/3, 2/3, 3/2, 3/4 only the last has a down factor of 4, and every other chain's convolver has down <= 3), and a "
        "convolver with up = 3 takes the radix-3 edge modes 3 / 7 / 11",
        "Engine::conv_path(): `if (opt(kPairConv) && pair_edge3(g)) return kPathPair3`, the kTabSoloDown case `up3 ? "
        "kPathPair3 : kPathPair` and `if (convx_edge3(g)) return kPathConvx3` come before the plain paths; "
        "resolve_forms() gives kPathPair3 / kPathConvx3 the kBackEdge3 modes, so convp_down's `convp_run<LN, -DL, 0, 24>` "
        "/ `<.., 6, ..>` / `<13, -2, 10>` and convx_dispatch's `convx_run<LN, -DL, kBackConv, 24>` never see DL = 2")
    # 2: 64 -> 16-point blocks
    + _not_built(
        ["k_convp<6, -2, 3, 24>", "k_convp<6, -2, 7, 24>"],
        "a 64-point block takes a filter of 32 taps at most (r8b_plan.cpp: bl2 = 2 << block_len_bits), and the shortest "
        "quarter-band filter the designer makes -- transition band 45 %, 49 dB, the limits of both parameters -- has 35: "
        "ratio 3/4 starts at 128 -> 32 points, k_convp<7, -2, 3, 24>",
        "convp_down(): `if (ln != LN) return false` with LN = 6 and X.c.down == 4")
    # 16: 25-tap windows on a 1:1 geometry
    + _not_built(
        _syms("k_convp", _ALL_LN, 0, (4, 16)),
        "a 1:1 convolver stands in front of a whole-step interpolator only in the planner's strong down-sampling chains, "
        "where the interpolator takes In / Out = src / (dst * 2^c) in [2, 4) inputs per output: the window starts of a "
        "phase pair are 2 or 3 samples apart, which is the 27-tap form (modes 5 / 17)",
        "Engine::resolve_forms() case kFusedPair2: `taps2 == 27 ? kBackWhole2W : kBackWhole2` (prepare_two_phase: T2 = "
        "maxdl <= 1 ? 25 : 27, and maxdl >= floor(In / Out) >= 2)")
    # 10: the interpolator fused into 64-point blocks
    + _not_built(
        _syms("k_convp", (5,), 1, (1, 4, 5, 16, 17)) + ["k_convp<5, 1, 1, 32>"] +
        _syms("k_convp", (6,), 0, (1, 5, 17)) + ["k_convp<6, 0, 1, 32>"],
        "a 64-point block has a filter of 31 taps at most (odd lengths, bl2 = 2 << block_len_bits), so 34 new samples at "
        "least: the interpolator's run and the zeros behind it do not fit the block's part of the array, the pair is not "
        "fused",
        "Engine::fused_form(): `if (pair && g.in_len + 32 > g.n_out) return kFusedNone`")
    # 2: 32-tap windows on 128-point blocks
    + _not_built(
        ["k_convp<6, 1, 1, 32>", "k_convp<7, 0, 1, 32>"],
        "a 128-point block (filters of 33 ... 63 taps) has 96 new samples at most, an interpolator of more than 24 taps "
        "asks for 100 at least",
        "Engine::fused_form(): `w.flen > 32 || g.in_len < 4 * w.flen` returns kFusedNone")
    # 6: two phases per thread on 128-point blocks
    + _not_built(
        _syms("k_convp", (6,), 1, (4, 5, 16, 17)) + _syms("k_convp", (7,), 0, (5, 17)),
        "a 128-point block has 64 new samples at least, and the two-phase form's run starts 32 elements into the array at "
        "least and needs 48 behind it: 32 + 64 + in_step + 48 > 128, the pair runs with one phase per thread (mode 1) or, "
        "with a complex spectrum, unfused",
        "Engine::fused_form(): `run_fits = run_off + g.in_len + w.in_step + 32 + 16 <= g.n_out` is false, so the last "
        "line returns kFusedPair1 (and `latency_chain_ && !(pair && run_fits && ...)` kFusedNone)")
)

RUN = {e["symbol"]: e for e in RUNS}
SYMBOLS = sorted(e["symbol"] for e in RUNS)
assert len(RUN) == len(RUNS) and len(set(SYMBOLS)) == len(SYMBOLS), "an instance is listed twice"

# the channels of check_instance(): a full-scale pair partner beside 1e-6 of full scale (the level exchange), silence
# beside full scale (the silence path), and a fifth, full-scale channel without a partner.  The one-channel forms and
# k_convx have no partners: they see a quiet and a silent channel all the same
LEVELS = (1.0, 1e-6, 0.0, 1.0, 1.0)
NCH = len(LEVELS)


def blocks_per_workgroup(symbol):
    """ConvpGeom<LN, UL>::SUB (r8b_convp.h): block pairs a workgroup of the pair kernel carries; 1 for k_convq, k_convx"""
    m = re.match(r"k_convp(?:_walk)?<(\d+), (-?\d+), ", symbol)
    if not m:
        return 1
    ln, ul = int(m.group(1)), int(m.group(2))
    nt = (1 << max(ln, ln + ul)) // 16
    return max(nt, 256) // nt


def stage_block_src(desc, src, stage):
    """new input samples per block of the convolver at `stage` (a line of describe() per stage), in SOURCE samples; the
    first convolver's is nonfinite_cases.chain_geometry's"""
    from nonfinite_cases import chain_geometry
    lines = [l for l in desc.splitlines() if re.match(r"(BlockConvolver|HBDownsampler|HBUpsampler|FracInterpolator)", l)]
    if lines[stage].startswith("HBDownsampler") and lines[stage + 1].startswith("BlockConvolver"):
        stage += 1      # (the half-band front, mode 20: the launch reports at the decimator it took in)
    assert lines[stage].startswith("BlockConvolver"), (stage, desc)
    first = [i for i, l in enumerate(lines) if l.startswith("BlockConvolver")][0]
    if stage == first:
        return chain_geometry(desc, src)[0]
    rate = float(src)
    for i, l in enumerate(lines):
        if l.startswith("HBDownsampler"):
            rate /= 2.0
        elif l.startswith("HBUpsampler"):
            rate *= 2.0
        elif l.startswith("FracInterpolator"):
            rate = float(re.search(r"([\d.]+)->([\d.]+)", l).group(2))
        else:
            up, down = map(int, re.search(r"io=(\d+)/(\d+)", l).groups())
            if i == stage:
                return int(re.search(r"in_len=(\d+)", l).group(1)) / up * (src / rate)
            rate = rate * up / down
    raise AssertionError(desc)


def first_cut(n, maxin):
    """ragged calls in the pattern of cases.check_parked_outputs: whole calls of MaxInLen, a third, a few samples, one sample"""
    pattern = [maxin, maxin // 3, 300 % maxin + 1, 1, 1, 2, maxin, 17, 1, maxin - 5, 2500 % maxin + 1, maxin, 40]
    lens, i = [], 0
    while sum(lens) < n:
        lens.append(max(1, min(pattern[i % len(pattern)], n - sum(lens))))
        i += 1
    return lens


class HostTier:
    """the host emulation: numpy arrays through process_host"""
    gpu = False

    def put(self, x):
        return x

    def call(self, b, x):
        return b.process_host(x)

    def cat(self, ys):
        import numpy as np
        return np.concatenate(ys, axis=1)

    def host(self, y):
        return y

    def same_bits(self, a, b):
        import numpy as np
        from nonfinite_cases import _bits
        return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


class DeviceTier(HostTier):
    """the device: torch tensors through process(); the bitwise comparison stays on the device"""
    gpu = True

    def __init__(self, torch):
        from lone_sample_cases import DeviceRunner
        self.t, self.r = torch, DeviceRunner(torch)

    def put(self, x):
        import numpy as np
        return self.r.put(np.array(x))     # (a writable copy: the shared input stays read-only)

    def call(self, b, x):
        return b.process(x).clone()

    def cat(self, ys):
        return self.t.cat(ys, dim=1)

    def host(self, y):
        return y.cpu().numpy()

    def same_bits(self, a, b):
        return self.r.same_bits(a, b)


_INPUT = {}


def census_input(n):
    """NCH rows of splitmix noise at LEVELS, computed once per length and left unchanged"""
    import numpy as np
    import r8b_oracle as O
    if n not in _INPUT:
        x = np.stack([lv * O.splitmix_uniform(301 + c, n) for c, lv in enumerate(LEVELS)])
        x.setflags(write=False)
        _INPUT[n] = x
    return _INPUT[n]


def _stream(tier, b, xd, lens, stage):
    ys, pos, seen = [], 0, set()
    for l in lens:
        ys.append(tier.call(b, xd[:, pos:pos + l]))
        seen.add(b.stage_symbols()[stage])     # (names the stage's LATEST launch: collected call by call)
        pos += l
    assert pos == xd.shape[1]
    return tier.cat(ys), [int(y.shape[1]) for y in ys], seen


def check_instance(make, tier, e, refwrap=None, provider=None):
    """`make()` builds a fresh NCH-channel object of the entry's chain with its options set and timing on.  refwrap: the
    compiled reference (oracle/refwrap.py) where oracle/_ref was built, else None -- the numpy oracle then stands in for
    linear-phase chains.  provider: the active test_emul.reference_minphase_taps context of a minimum-phase entry.

    The stream: max(6, two full block groups and a partly filled one) blocks of the entry's convolver and two whole calls
    at least, cut into ragged calls (first_cut: a whole MaxInLen call, one-sample calls, calls that end inside a block).
      1. the entry's symbol is among the symbols its stage ran;
      2. per-call counts equal the reference's, and every channel is within cases.RMS_TOL / PEAK_TOL times its OWN level
         times cases.tol_scale of its stream (minimum-phase entries flagged input_delay: 3e-12 / 2e-10, the stated
         exception of test_emul.run_minphase_reference_taps, and the flag is verified against the reference's latency);
      3. the silent channel is exact zeros;
      4. another cut of the stream into calls (nonfinite_cases._lens around the middle of the fourth block, a one-sample
         call behind it) gives the same bits.
    A minimum-phase entry without the compiled reference has no reference to run on (the numpy oracle designs no
    minimum-phase filter): 1, 3 and 4 are checked.  Returns the worst own-level (rms, peak)."""
    import numpy as np
    from cases import PEAK_TOL, RMS_TOL, tol_scale
    from nonfinite_cases import _lens
    src, dst, maxin, tb, att, phase, stage = (e[k] for k in ("src", "dst", "maxin", "tb", "att", "phase", "stage"))
    b = make()
    desc = b.describe()
    block_src = stage_block_src(desc, src, stage)
    sub = blocks_per_workgroup(e["symbol"])
    nblocks = max(6, 2 * sub + 1)
    n = max(int(math.ceil((nblocks + 0.5) * block_src)) + b.getInLenBeforeOutPos(0), 2 * maxin + 59)
    x = census_input(n)
    xd = tier.put(x)
    lens = first_cut(n, maxin)
    assert sum(lens) == n and maxin in lens and 1 in lens
    yd, counts, seen = _stream(tier, b, xd, lens, stage)
    # 1.
    assert e["symbol"] in seen, (e["symbol"], sorted(seen), desc)
    y = tier.host(yd)
    assert y.shape[0] == NCH and y.shape[1] > 0 and np.isfinite(y).all()
    # 3.
    assert not y[2].any(), "silence in, %g out" % float(np.abs(y[2]).max())
    # 2.
    worst = None
    loud = [c for c, lv in enumerate(LEVELS) if lv > 0.0]
    if refwrap is not None or phase == 0:
        if refwrap is not None:
            r, p = refwrap.batch_check(src, dst, maxin, lens, x, y, counts, tb, att, phase=phase)
        else:
            import r8b_oracle as O
            r, p = np.zeros(NCH), np.zeros(NCH)
            for c in loud:
                o = O.OracleResampler(src, dst, maxin, tb, att)
                yo, pos = [], 0
                for l in lens:
                    yo.append(o.process(x[c, pos:pos + l]))
                    pos += l
                assert [len(v) for v in yo] == counts, (c, counts)
                d = y[c] - np.concatenate(yo)
                r[c], p[c] = math.sqrt(float(np.mean(d * d))), float(np.abs(d).max())
        delayed = False
        if phase == 1 and provider is not None:
            delayed = reference_input_delay(desc, stage, provider)
            assert delayed == e["input_delay"], "input_delay flag %s, the reference's latency says %s" % (e["input_delay"], delayed)
        else:
            assert not e["input_delay"]
        rt, pt = (3e-12, 2e-10) if delayed else (RMS_TOL, PEAK_TOL)
        worst = (0.0, 0.0)
        for c in loud:
            # (the stream's own power, at its level: it is the reference's to 1e-15)
            sc = tol_scale(float(np.sum((y[c] / LEVELS[c]) ** 2)), y.shape[1])
            rr, pp = r[c] / LEVELS[c], p[c] / LEVELS[c]
            worst = (max(worst[0], rr / sc), max(worst[1], pp / sc))
            assert rr <= rt * sc and pp <= pt * sc, "%s channel %d (level %g): rms %.3g peak %.3g of its level, scale %.2f" % (
                e["symbol"], c, LEVELS[c], rr, pp, sc)
    # 4.
    lens2, at = _lens(n, maxin, int(3.5 * block_src) + 1)
    assert at is not None and at + 1 < len(lens2)
    if lens2[at + 1] > 1:
        lens2[at + 1:at + 2] = [1, lens2[at + 1] - 1]
    assert sum(lens2) == n and 1 in lens2 and lens2 != lens
    y2, _, seen2 = _stream(tier, make(), xd, lens2, stage)
    assert e["symbol"] in seen2, (e["symbol"], sorted(seen2))
    if not tier.same_bits(yd, y2):
        y2 = tier.host(y2)
        c, j = np.nonzero(y != y2) if y.shape == y2.shape else ([-1], [-1])
        raise AssertionError("%s: the output depends on the cut into calls, first (channel, output): (%d, %d) of %d" % (
            e["symbol"], c[0], j[0], len(c)))
    return worst


def reference_input_delay(desc, stage, provider):
    """whether the reference delays the input of the convolver at `stage` (CDSPBlockConvolver.h:124-138: InputDelay =
    DownFactor - InLatency mod DownFactor where it decimates by a power of two in the spectrum), from the latency of the
    reference's own minimum-phase filter as the provider handed it over.  Single-convolver chains without stages in
    front (no inherited latency): the flag is allowed nowhere else."""
    lines = [l for l in desc.splitlines() if re.match(r"(BlockConvolver|HBDownsampler|HBUpsampler|FracInterpolator)", l)]
    up, down = map(int, re.search(r"io=(\d+)/(\d+)", lines[stage]).groups())
    if stage != 0 or down < 2 or down & (down - 1):
        return False
    assert len(provider.calls) >= 1
    latency, latency_frac = provider.calls[0][5], provider.calls[0][6]
    return (int(latency_frac) + latency) % down != 0


def dump(out):
    for e in RUNS:
        out.write("%s|%r|%r|%d|%r|%r|%d|%d|%s\n" % (e["symbol"], e["src"], e["dst"], e["maxin"], e["tb"], e["att"], e["phase"],
                                                    e["stage"], ",".join("%s=%d" % kv for kv in sorted(e["opts"].items()))))


if __name__ == "__main__":
    if sys.argv[1:] == ["--dump"]:
        dump(sys.stdout)
    else:
        sys.exit("usage: python tests/kernel_census.py --dump")
