"""Cost of r8b_batch_resample_clips_mix against what a host does without it (profiles/clip_mix_ab.txt), by the method of
tools/clip_frames_ab.py: 512 stereo clips of 16384 x 8 frames, S16 interleaved in, F32 planar out, 44100 -> 96000
(180.15 dB), MaxInLen 16384, option "timing" 0, mix [0.5 0.5].  HIP events around a whole batch; the variants alternate
batch by batch after a warm-up; median, minimum and maximum of the repetitions:
  (a) the mix call on a 512-channel object;
  (b) equal output today: the _ex call with K = 2 on a 1024-channel object, then a torch mean over the channel pair;
  (c) a torch mix to F64 rows, then r8b_batch_resample_clips on 512 channels;
  (d) the floor: r8b_batch_resample_clips on 512 mono S16 rows that are ready.
    python tools/clip_mix_ab.py [--reps 7] [--out profiles/clip_mix_ab_run.txt]"""
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
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--clips", type=int, default=512)
ap.add_argument("--calls", type=int, default=8)
ap.add_argument("--out", default=None)
args = ap.parse_args()

SRC, DST, L, ATT = 44100.0, 96000.0, 16384, 180.15
n, T = args.clips, L * args.calls
lib = r8b.load()
P = lib.r8b_clip_out_len(SRC, DST, T)
stream = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device="cuda")
g.manual_seed(7)
S16, F32, F64 = r8b.PCM_S16, r8b.PCM_F32, r8b.PCM_F64
MIX = (C.c_double * 2)(0.5, 0.5)


def make(nch):
    h = lib.r8b_batch_create(SRC, DST, L, 2.0, ATT, nch, -1)
    assert h, lib.r8b_last_error()
    return h


def lens(count, v):
    return (C.c_longlong * count)(*([v] * count))


def run_mix(h, x, out):
    p = lib.r8b_batch_resample_clips_mix(h, 2, 1, MIX, C.c_void_p(x.data_ptr()), S16, 1, x.stride(0), lens(n, T),
                                         C.c_void_p(out.data_ptr()), F32, 0, out.stride(0), lens(n, P), C.c_void_p(stream))
    assert p == P, lib.r8b_last_error()


def run_ex(h, x, out):
    p = lib.r8b_batch_resample_clips_ex(h, 2, C.c_void_p(x.data_ptr()), S16, 1, x.stride(0), lens(n, T),
                                        C.c_void_p(out.data_ptr()), F32, 0, out.stride(0), lens(n, P), C.c_void_p(stream))
    assert p == P, lib.r8b_last_error()


def run_planar(h, x, fmt, out):
    p = lib.r8b_batch_resample_clips(h, C.c_void_p(x.data_ptr()), fmt, x.stride(0), lens(n, T), C.c_void_p(out.data_ptr()),
                                     F32, out.stride(0), lens(n, P), C.c_void_p(stream))
    assert p == P, lib.r8b_last_error()


x = (torch.rand((n, T, 2), generator=g, device="cuda") * 65536 - 32768).floor().clamp(-32768, 32767).to(torch.int16)
mono = x[:, :, 0].contiguous()
out_a = torch.zeros((n, P), dtype=torch.float32, device="cuda")
out_b2 = torch.zeros((2 * n, P), dtype=torch.float32, device="cuda")
out_c = torch.zeros((n, P), dtype=torch.float32, device="cuda")
out_d = torch.zeros((n, P), dtype=torch.float32, device="cuda")
out_b = [None]


def today_resample_all(h):
    run_ex(h, x, out_b2)
    out_b[0] = out_b2.view(n, 2, P).mean(dim=1)


def today_mix_first(h):
    rows = x.to(torch.float64).sum(dim=2) * (0.5 / 32768.0)
    run_planar(h, rows, F64, out_c)


variants = [("(a) mix call, 512 channels", make(n), lambda h: run_mix(h, x, out_a)),
            ("(b) _ex on 1024 channels + torch mean", make(2 * n), today_resample_all),
            ("(c) torch mix to F64 + planar call", make(n), today_mix_first),
            ("(d) planar call, mono S16 rows ready", make(n), lambda h: run_planar(h, mono, S16, out_d))]
times = {v[0]: [] for v in variants}
for rep in range(args.warmup + args.reps):
    for name, h, fn in variants:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(h)
        e1.record()
        e1.synchronize()
        if rep >= args.warmup:
            times[name].append(e0.elapsed_time(e1))
lines = ["S16 interleaved -> F32 planar, %d stereo clips x %d frames -> %d frames each, mix [0.5 0.5], %d repetitions after %d "
         "warm-up batches" % (n, T, P, args.reps, args.warmup),
         "  (a) equals (c) bit for bit: %s; largest |(a) - (b)|: %.3g (the mean behind the resampler rounds elsewhere)" %
         (bool(torch.equal(out_a, out_c)), float((out_a - out_b[0]).abs().max()))]
for name in times:
    t = times[name]
    lines.append("  %-40s median %8.3f ms  (min %8.3f, max %8.3f)" % (name, statistics.median(t), min(t), max(t)))
print("\n".join(lines))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
for _, h, _ in variants:
    lib.r8b_batch_delete(h)
