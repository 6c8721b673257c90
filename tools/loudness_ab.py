"""Cost of the loudness meter (profiles/loudness_ab.txt), by the protocol of tools/true_peak_ab.py: HIP events around a whole
r8b_batch_process_pcm call, the variants alternating call by call after a warm-up; median, minimum and maximum of the
repetitions.  Workload: --rows channels x --frames per call, 44100 -> 96000, F64 planar in, S16 planar out, meters on.

  (a) the PARENT commit's library (--parent), twice (the A/A' pair, whose difference is the run's spread), against this
      tree's library with the loudness meter never enabled, and enabled and switched off again: these must agree within
      that spread, or the off path is not inert
  (b) this tree with the loudness meter ON, and, in the same run, with the true-peak meter ON instead: each call's total
      and the kernel's share of it as the difference of the medians, beside k_loudness's two floors -- the bytes it reads
      (8 per frame and row, once) over the HBM rate, and its fp64 operations (two passes of 12, one energy fma and a
      share of the hand-off per frame) over the fp64 vector rate (39.3e12 FMA/s; HBM 8.0 TB/s by the data sheet, 6.29
      TB/s measured by a copy)
--profile N: nothing of the above -- N calls with BOTH meters on after the warm-up, for a run under
    rocprofv3 --kernel-trace --stats -- python tools/loudness_ab.py --profile 20
whose kernel statistics give k_loudness's own time next to k_truepeak's.
    python tools/loudness_ab.py --parent ../parent/r8brain-free-src_amd/libr8bsrc_hip.so [--out FILE]"""
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
HBM_SPEC, HBM_COPY, FMA_RATE = 8.0e12, 6.29e12, 39.3e12
n, L = args.rows, args.frames
CALLS = args.warmup + args.reps + args.profile + 2


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


def variant(lib, loudness, true_peak=False):
    """a stream of its own: -> the call.  loudness: None never enabled, False enabled and off again, True on"""
    h = lib.r8b_batch_create(SRC, DST, L, 2.0, ATT, n, -1)
    assert h, lib.r8b_last_error()
    handles.append((lib, h))
    assert lib.r8b_batch_meter_enable(h, 1) == 0
    cap = lib.r8b_batch_max_out_len(h)
    if loudness is not None:
        # (a store that takes the whole run: no draining read between the timed calls)
        blocks = CALLS * (cap // int(DST / 10 + 0.5) + 1)
        assert lib.r8b_batch_loudness_enable(h, 1, blocks) == 0, lib.r8b_last_error()
        assert lib.r8b_batch_loudness_enable(h, 1 if loudness else 0, blocks) == 0
    if true_peak:
        assert lib.r8b_batch_true_peak_enable(h, 1) == 0
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
    on = variant(tree, True, True)
    for _ in range(args.warmup + args.profile):
        on()
    torch.cuda.synchronize()
    print("%d calls with the loudness and the true-peak meter on, %d rows x %d frames in, %d frames out in the last" %
          (args.warmup + args.profile, n, L, out_frames[-1]))
    sys.exit(0)

yard = parent if parent is not None else tree
who = "parent" if parent is not None else "tree (NO parent given)"
OFF, ON, TP = "tree, loudness never enabled", "tree, loudness ON", "tree, true peak ON (loudness never enabled)"
runs = [("%s library (A)" % who, variant(yard, None)), ("%s library (A')" % who, variant(yard, None)),
        (OFF, variant(tree, None)), ("tree, loudness enabled, then off", variant(tree, False)),
        (ON, variant(tree, True)), (TP, variant(tree, None, True))]
times = alternate(runs)
med = {k: statistics.median(v) for k, v in times.items()}
frames = out_frames[-1]
lines = ["%g -> %g, %d rows x %d frames per call (%d out), F64 planar in, S16 planar out, meters on; %d repetitions after %d "
         "warm-up calls, the variants alternating; parent library: %s" %
         (SRC, DST, n, L, frames, args.reps, args.warmup, "given" if parent else "NOT given")]
lines += ["  %-44s median %8.3f ms  (min %8.3f, max %8.3f)" % (k, med[k], min(v), max(v)) for k, v in times.items()]
a, a2 = med["%s library (A)" % who], med["%s library (A')" % who]
q = statistics.quantiles(times["%s library (A)" % who], n=4)
lines.append("(a) spread of the yardstick: |A - A'| of the medians %.3f ms, A's own quartiles %.3f .. %.3f ms; tree with the "
             "meter off against A: never enabled %+.3f ms, off again %+.3f ms" %
             (abs(a - a2), q[0], q[2], med[OFF] - a, med["tree, loudness enabled, then off"] - a))
nbytes = 8.0 * n * frames
ops = (2 * 12 + 1 + 16.0 / 64) * n * frames
lines.append("(b) call with the loudness meter on %.3f ms; on - off = %.3f ms for k_loudness's %d workgroups of one wave; the "
             "true-peak meter in its place: %.3f ms, on - off = %.3f ms" %
             (med[ON], med[ON] - med[OFF], n, med[TP], med[TP] - med[OFF]))
lines.append("    floors: %.1f MB read -> %.3f ms at 8.0 TB/s (%.3f ms at the 6.29 TB/s of a copy); %.2f G fp64 operations -> %.3f ms "
             "at 39.3e12 per second" % (nbytes / 1e6, nbytes / HBM_SPEC * 1e3, nbytes / HBM_COPY * 1e3, ops / 1e9, ops / FMA_RATE * 1e3))
print("\n".join(lines))
for lib, h in handles:
    lib.r8b_batch_delete(h)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
