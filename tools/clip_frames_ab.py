"""Cost of r8b_batch_resample_clips_ex on interleaved clips (profiles/clip_frames_ab.txt), by the method and on the workload
of tools/clips_ab.py so that the lines compare: 1024 object channels, 16384 x 8 frames per clip, 44100 -> 96000
(180.15 dB), MaxInLen 16384, option "timing" 0, as 512 stereo clips and as 128 eight-channel clips, S16 interleaved ->
F32 interleaved.  HIP events around a whole batch; the variants alternate batch by batch after a warm-up, the median of
the repetitions is reported:
  (a) the _ex call on the interleaved buffers;
  (b) the planar call on rows that are de-interleaved already, same build: the same bytes moved, the floor;
  (c) what a host does without the call: torch permute(...).contiguous() on both sides around the planar call.
    python tools/clip_frames_ab.py [--tile NAME=/path/to/libr8bsrc_hip.so ...] [--reps 7]
--tile: (a) once more on another BUILD of the library (csrc/r8b_clip_frames.h R8B_CLIP_TILE_SAMPLES: other tiles),
same process."""
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
ap.add_argument("--tile", action="append", default=[])
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--channels", type=int, default=1024)
ap.add_argument("--calls", type=int, default=8)
ap.add_argument("--clip-channels", type=int, nargs="+", default=[2, 8])
args = ap.parse_args()

SRC, DST, L, ATT = 44100.0, 96000.0, 16384, 180.15
nch, T = args.channels, L * args.calls
new = r8b.load()
builds = [("this build", new)] + [(t.rpartition("=")[0], r8b.bind(t.rpartition("=")[2])) for t in args.tile]
P = new.r8b_clip_out_len(SRC, DST, T)
stream = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device="cuda")
g.manual_seed(7)
S16, F32 = r8b.PCM_S16, r8b.PCM_F32


def make(lib):
    h = lib.r8b_batch_create(SRC, DST, L, 2.0, ATT, nch, -1)
    assert h, lib.r8b_last_error()
    return h


def run_ex(lib, h, K, x, out):
    n = nch // K
    lens, outs = (C.c_longlong * n)(*([T] * n)), (C.c_longlong * n)(*([P] * n))
    p = lib.r8b_batch_resample_clips_ex(h, K, C.c_void_p(x.data_ptr()), S16, 1, x.stride(0), lens,
                                        C.c_void_p(out.data_ptr()), F32, 1, out.stride(0), outs, C.c_void_p(stream))
    assert p == P, lib.r8b_last_error()


def run_planar(lib, h, x, out):
    lens, outs = (C.c_longlong * nch)(*([T] * nch)), (C.c_longlong * nch)(*([P] * nch))
    p = lib.r8b_batch_resample_clips(h, C.c_void_p(x.data_ptr()), S16, x.stride(0), lens, C.c_void_p(out.data_ptr()), F32,
                                     out.stride(0), outs, C.c_void_p(stream))
    assert p == P, lib.r8b_last_error()


for K in args.clip_channels:
    n = nch // K
    x = (torch.rand((n, T, K), generator=g, device="cuda") * 65536 - 32768).floor().clamp(-32768, 32767).to(torch.int16)
    rows = x.permute(0, 2, 1).contiguous().view(nch, T)
    out_a = torch.zeros((n, P, K), dtype=torch.float32, device="cuda")
    out_b = torch.zeros((nch, P), dtype=torch.float32, device="cuda")
    out_c = [None]

    def host_today(lib, h):
        planar = x.permute(0, 2, 1).contiguous().view(nch, T)
        run_planar(lib, h, planar, out_b)
        out_c[0] = out_b.view(n, K, P).permute(0, 2, 1).contiguous()

    variants = [("(a) _ex, %s" % name, lib, make(lib), lambda lib, h: run_ex(lib, h, K, x, out_a)) for name, lib in builds]
    variants.append(("(b) planar call, rows ready", new, make(new), lambda lib, h: run_planar(lib, h, rows, out_b)))
    variants.append(("(c) permute + planar call + permute", new, make(new), host_today))
    times = {v[0]: [] for v in variants}
    for rep in range(args.warmup + args.reps):
        for name, lib, h, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(lib, h)
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                times[name].append(e0.elapsed_time(e1))
    # (the three computed the same frames)
    same = bool(torch.equal(out_a, out_c[0])) and bool(torch.equal(out_a, out_b.view(n, K, P).permute(0, 2, 1)))
    print("S16 interleaved -> F32 interleaved, %d clips x %d channels x %d frames -> %d frames each, %d repetitions after "
          "%d warm-up batches; outputs equal: %s" % (n, K, T, P, args.reps, args.warmup, same))
    for name in times:
        t = times[name]
        print("  %-40s median %8.3f ms  (min %8.3f, max %8.3f)" % (name, statistics.median(t), min(t), max(t)))
    for _, lib, h, _ in variants:
        lib.r8b_batch_delete(h)
    del x, rows, out_a, out_b, out_c, variants
