"""Cost of the true-peak meter (profiles/true_peak_ab.txt), by the method of tools/pcm8_ab.py: HIP events around a whole
r8b_batch_process_pcm call, the variants alternating call by call after a warm-up; median, minimum and maximum of the
repetitions.  Workload: --rows channels x --frames per call, 44100 -> 96000, F64 planar in, S16 planar out, meters on.

  (a) the PARENT commit's library (--parent), twice (the A/A' pair, whose difference is the run's spread), against this
      tree's library with the true-peak meter never enabled, and enabled and switched off again: these must agree
      within that spread, or the off path is not inert
  (b) this tree with the meter ON: the call's total; the kernel's share of it as the difference of the medians, beside
      its two floors -- the bytes k_truepeak reads (8 per frame and row, the 11-frame halo of every tile with them) over
      the HBM rate, and its 36 multiply-adds per frame over the fp64 vector rate (78.6 TFLOP/s = 39.3e12 FMA/s; HBM 8.0
      TB/s by the data sheet, 6.29 TB/s measured by a copy)
--profile N: nothing of the above -- N calls with the meter on after the warm-up, for a run under
    rocprofv3 --kernel-trace --stats -- python tools/true_peak_ab.py --profile 20
whose kernel statistics give k_truepeak's own time.
    python tools/true_peak_ab.py --parent ../parent/r8brain-free-src_amd/libr8bsrc_hip.so [--out FILE]"""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

r8b = importlib.import_module("r8brain-free-src_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None)
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rows", type=int, default=1024)
ap.add_argument("--frames", type=int, default=16384)
ap.add_argument("--profile", type=int, default=0, metavar="N")
ap.add_argument("--out", default=None)
args = ap.parse_args()

SRC, DST, ATT = 44100.0, 96000.0, 180.15
F64, S16 = r8b.PCM_F64, r8b.PCM_S16
TILE, HALO = 2048, 11
HBM_SPEC, HBM_COPY, FMA_RATE = 8.0e12, 6.29e12, 39.3e12
n, L = args.rows, args.frames


def bind(path):
    lib = C.CDLL(os.path.abspath(path))
    for name, res, argt in r8b._capi.PROTOTYPES:
        if hasattr(lib, name):
            getattr(lib, name).restype, getattr(lib, name).argtypes = res, argt
    return lib


tree = r8b.load()
parent = bind(args.parent) if args.parent else None
stream = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device="cuda")
g.manual_seed(7)
x = torch.rand(n * L, generator=g, device="cuda", dtype=torch.float64) * 1.8 - 0.9
handles, out_frames = [], []


def variant(lib, true_peak):
    """a stream of its own: -> the call.  true_peak: None never enabled, False enabled and off again, True on"""
    h = lib.r8b_batch_create(SRC, DST, L, 2.0, ATT, n, -1)
    assert h, lib.r8b_last_error()
    handles.append((lib, h))
    assert lib.r8b_batch_meter_enable(h, 1) == 0
    if true_peak is not None:
        assert lib.r8b_batch_true_peak_enable(h, 1) == 0
        assert lib.r8b_batch_true_peak_enable(h, 1 if true_peak else 0) == 0
    cap = lib.r8b_batch_max_out_len(h)
    out = torch.zeros(n * cap, dtype=torch.int16, device="cuda")

    def call():
        got = lib.r8b_batch_process_pcm(h, C.c_void_p(x.data_ptr()), F64, 0, L, L, C.c_void_p(out.data_ptr()), S16, 0, cap,
                                        C.c_void_p(stream))
        assert got >= 0, lib.r8b_last_error()
        out_frames.append(got)
    return call


def alternate(runs):
    """one call of each variant per repetition, the order rotating from repetition to repetition, so that no variant
    always runs behind the same neighbour"""
    times = {label: [] for label, _ in runs}
    for rep in range(args.warmup + args.reps):
        for label, fn in runs[rep % len(runs):] + runs[:rep % len(runs)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                times[label].append(e0.elapsed_time(e1))
    return times


if args.profile:
    on = variant(tree, True)
    for _ in range(args.warmup + args.profile):
        on()
    torch.cuda.synchronize()
    print("%d calls with the true-peak meter on, %d rows x %d frames in, %d frames out in the last" %
          (args.warmup + args.profile, n, L, out_frames[-1]))
    sys.exit(0)

yard = parent if parent is not None else tree
who = "parent" if parent is not None else "tree (NO parent given)"
runs = [("%s library (A)" % who, variant(yard, None)), ("%s library (A')" % who, variant(yard, None)),
        ("tree, true peak never enabled", variant(tree, None)), ("tree, true peak enabled, then off", variant(tree, False)),
        ("tree, true peak ON", variant(tree, True))]
times = alternate(runs)
med = {k: statistics.median(v) for k, v in times.items()}
frames = out_frames[-1]
lines = ["%g -> %g, %d rows x %d frames per call (%d out), F64 planar in, S16 planar out, meters on; %d repetitions after %d "
         "warm-up calls, the variants alternating; parent library: %s" %
         (SRC, DST, n, L, frames, args.reps, args.warmup, "given" if parent else "NOT given")]
lines += ["  %-38s median %8.3f ms  (min %8.3f, max %8.3f)" % (k, med[k], min(v), max(v)) for k, v in times.items()]
a, a2 = med["%s library (A)" % who], med["%s library (A')" % who]
q = statistics.quantiles(times["%s library (A)" % who], n=4)
lines.append("(a) spread of the yardstick: |A - A'| of the medians %.3f ms, A's own quartiles %.3f .. %.3f ms; tree with the "
             "meter off against A: never enabled %+.3f ms, off again %+.3f ms" %
             (abs(a - a2), q[0], q[2], med["tree, true peak never enabled"] - a, med["tree, true peak enabled, then off"] - a))
tiles = (frames + TILE - 1) // TILE
nbytes = 8.0 * n * (frames + HALO * tiles)
fmas = 36.0 * n * frames
kern = med["tree, true peak ON"] - med["tree, true peak never enabled"]
lines.append("(b) call with the meter on %.3f ms; on - off = %.3f ms for k_truepeak's %d workgroups" %
             (med["tree, true peak ON"], kern, tiles * n))
lines.append("    floors: %.1f MB read -> %.3f ms at 8.0 TB/s (%.3f ms at the 6.29 TB/s of a copy); %.2f G multiply-adds -> %.3f ms "
             "at 39.3e12 FMA/s" % (nbytes / 1e6, nbytes / HBM_SPEC * 1e3, nbytes / HBM_COPY * 1e3, fmas / 1e9, fmas / FMA_RATE * 1e3))
print("\n".join(lines))
for lib, h in handles:
    lib.r8b_batch_delete(h)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
