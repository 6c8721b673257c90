"""Cost of the one-byte PCM formats' row kernels (profiles/pcm8_ab.txt), by the method of tools/clip_packed_ab.py: HIP
events around a whole call, the variants alternating call by call after a warm-up; median, minimum and maximum of the
repetitions.  Every object is a pass-through one (Src == Dst: no stages), so a call is the ingest kernel, the copy of
the staging rows and the egress kernel -- the two kernels under test and nothing of the resampler.

  rows   r8b_batch_process_pcm, planar, --rows x --frames per call:
           X -> F64   the ingest of format X (the egress is the F64 row kernel in every variant)
           F64 -> X   the egress of format X
           X -> X     both
  clips  r8b_batch_resample_clips_packed on the clip batch of tools/clip_packed_ab.py case (b): --rows mono clips of
         lengths uniform in [T/4, T], T = 8 x --frames, packed end to end on both sides, X -> X

--parent names the PARENT commit's libr8bsrc_hip.so: its S16 calls on the same shapes are the yardstick, measured on two
objects (the A/A pair, whose difference is the run's spread).  An S16 side moves 2 + 8 bytes per sample through its
kernel, a one-byte side 1 + 8: the one-byte kernels should take no longer.  This tree's own S16 call ("S16, tree") shows
what the added formats cost the existing ones.  --variant NAME=LIBRARY (repeatable) adds builds of the library from trees
whose one-byte row form differs (csrc/r8b_pcm.h kPcm8Lane, the samples a lane takes: 1 and 8 were built that way beside
the 4 that was kept), each measured on U8 / ULAW / ALAW beside this tree's own library ("tree").
    python tools/pcm8_ab.py --parent ../parent/r8brain-free-src_amd/libr8bsrc_hip.so [--variant k4=lib_k4.so] [--out FILE]"""
import argparse
import ctypes as C
import importlib
import os
import random
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

r8b = importlib.import_module("r8brain-free-src_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None)
ap.add_argument("--variant", action="append", default=[], metavar="NAME=LIBRARY")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rows", type=int, default=1024)
ap.add_argument("--frames", type=int, default=16384)
ap.add_argument("--formats", default="u8,ulaw,alaw")
ap.add_argument("--skip-clips", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()

RATE, ATT = 48000.0, 180.15
F64, S16 = r8b.PCM_F64, r8b.PCM_S16
FORMATS = {"u8": r8b.PCM_U8, "ulaw": r8b.PCM_ULAW, "alaw": r8b.PCM_ALAW}
DTYPE = {F64: torch.float64, S16: torch.int16}
n, L = args.rows, args.frames


def bind(path):
    lib = C.CDLL(os.path.abspath(path))
    for name, res, argt in r8b._capi.PROTOTYPES:
        if hasattr(lib, name):
            getattr(lib, name).restype, getattr(lib, name).argtypes = res, argt
    return lib


libs = {"tree": r8b.load()}
for v in args.variant:
    name, path = v.split("=", 1)
    libs[name] = bind(path)
parent = bind(args.parent) if args.parent else None
stream = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device="cuda")
g.manual_seed(7)


def ll(v):
    return (C.c_longlong * len(v))(*v)


def samples(fmt, count):
    """`count` samples of a format on the device: every code of a one-byte format, noise otherwise"""
    if fmt == F64:
        return torch.rand(count, generator=g, device="cuda", dtype=torch.float64) * 2 - 1
    if fmt == S16:
        return (torch.rand(count, generator=g, device="cuda") * 65536 - 32768).floor().clamp(-32768, 32767).to(torch.int16)
    return (torch.rand(count, generator=g, device="cuda") * 256).floor().clamp(0, 255).to(torch.uint8)


def alternate(runs):
    """runs: [(label, fn)] -> lines; the calls alternate, one of each per repetition"""
    times = {label: [] for label, _ in runs}
    for rep in range(args.warmup + args.reps):
        for label, fn in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                times[label].append(e0.elapsed_time(e1))
    return ["  %-44s median %8.3f ms  (min %8.3f, max %8.3f)" % (label, statistics.median(t), min(t), max(t))
            for label, t in times.items()]


def yardsticks():
    """[(label, library)]: the parent's library twice (A, A'), or this tree's when none was given"""
    lib, who = (parent, "parent") if parent is not None else (libs["tree"], "tree (NO parent given)")
    return [("S16, %s library (A)" % who, lib), ("S16, %s library (A')" % who, lib)]


def rows_case(title, side):
    """side: "in" (X -> F64), "out" (F64 -> X), "both" (X -> X)"""
    handles, runs = [], []

    def add(label, lib, fmt):
        fi, fo = (fmt if side != "out" else F64), (fmt if side != "in" else F64)
        h = lib.r8b_batch_create(RATE, RATE, L, 2.0, ATT, n, -1)
        assert h, lib.r8b_last_error()
        handles.append((lib, h))
        x = samples(fi, n * L)
        out = torch.zeros(n * L, dtype=DTYPE.get(fo, torch.uint8), device="cuda")

        def call():
            got = lib.r8b_batch_process_pcm(h, C.c_void_p(x.data_ptr()), fi, 0, L, L, C.c_void_p(out.data_ptr()), fo, 0, L,
                                            C.c_void_p(stream))
            assert got == L, lib.r8b_last_error()
        runs.append((label, call))

    for label, lib in yardsticks() + [("S16, tree", libs["tree"])]:
        add(label, lib, S16)
    for fname in args.formats.split(","):
        for vname, lib in libs.items():
            add("%s, %s" % (fname.upper(), vname), lib, FORMATS[fname])
    lines = [title] + alternate(runs)
    for lib, h in handles:
        lib.r8b_batch_delete(h)
    return lines


def clips_case(title):
    T = L * 8
    rnd = random.Random(11)
    lens = [rnd.randint(T // 4, T) for _ in range(n)]
    tree = libs["tree"]
    off = (C.c_longlong * n)()
    total = tree.r8b_clip_pack_offsets(n, ll(lens), 1, 1, off)
    off = list(off)
    handles, runs = [], []

    def add(label, lib, fmt):
        h = lib.r8b_batch_create(RATE, RATE, L, 2.0, ATT, n, -1)
        assert h, lib.r8b_last_error()
        handles.append((lib, h))
        x = samples(fmt, total)
        out = torch.zeros(total, dtype=DTYPE.get(fmt, torch.uint8), device="cuda")

        def call():
            p = lib.r8b_batch_resample_clips_packed(h, 0, 1, None, C.c_void_p(x.data_ptr()), fmt, 0, 0, ll(off), ll(lens),
                                                    C.c_void_p(out.data_ptr()), fmt, 0, 0, ll(off), ll(lens), C.c_void_p(stream))
            assert p == max(lens), lib.r8b_last_error()
        runs.append((label, call))

    for label, lib in yardsticks() + [("S16, tree", libs["tree"])]:
        add(label, lib, S16)
    for fname in args.formats.split(","):
        for vname, lib in libs.items():
            add("%s, %s" % (fname.upper(), vname), lib, FORMATS[fname])
    lines = [title, "  %d clips, %d frames in all (%.3f of the padded batch)" % (n, total, total / (n * T))] + alternate(runs)
    for lib, h in handles:
        lib.r8b_batch_delete(h)
    return lines


lines = ["pass-through objects (%g -> %g), %d rows, MaxInLen %d, %d repetitions after %d warm-up calls; parent library: %s; "
         "variants: %s" % (RATE, RATE, n, L, args.reps, args.warmup, "given" if parent else "NOT given", ", ".join(libs))]
lines += rows_case("rows, ingest: X -> F64, %d x %d frames per call" % (n, L), "in")
lines += rows_case("rows, egress: F64 -> X, %d x %d frames per call" % (n, L), "out")
lines += rows_case("rows, both sides: X -> X, %d x %d frames per call" % (n, L), "both")
if not args.skip_clips:
    lines += clips_case("clips packed on both sides, X -> X (the batch of tools/clip_packed_ab.py case (b))")
print("\n".join(lines))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
