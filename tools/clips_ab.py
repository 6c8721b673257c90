"""Cost of r8b_batch_resample_clips against the loop a host writes around r8b_batch_process_pcm / r8b_batch_process
(profiles/clips_ab.txt): 1024 clips of equal length 16384 x 8 frames, 44100 -> 96000 (180.15 dB), MaxInLen 16384, planar
rows, option "timing" 0.  HIP events around the whole loop of one batch; the variants alternate batch by batch after a
warm-up, the median of the repetitions is reported.
    python tools/clips_ab.py [--parent /path/to/another/build/libr8bsrc_hip.so] [--reps 7]
--parent: the host loops once more on another build of the library (the commit before the clips call), same process."""
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
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--channels", type=int, default=1024)
ap.add_argument("--calls", type=int, default=8)
args = ap.parse_args()

SRC, DST, L, ATT = 44100.0, 96000.0, 16384, 180.15
nch, T = args.channels, L * args.calls


def bind_some(path):
    """another build of the library: the prototypes of the symbols it has"""
    lib = C.CDLL(path)
    for name, res, argtypes in r8b.PROTOTYPES:
        if hasattr(lib, name):
            f = getattr(lib, name)
            f.restype, f.argtypes = res, argtypes
    return lib


new = r8b.load()
libs = [("this build", new)] + ([("parent build", bind_some(args.parent))] if args.parent else [])
P = new.r8b_clip_out_len(SRC, DST, T)
stream = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device="cuda")
g.manual_seed(7)
x64 = torch.rand((nch, T), generator=g, dtype=torch.float64, device="cuda") * 2 - 1
x32 = x64.to(torch.float32)
FMT = {torch.float32: r8b.PCM_F32, torch.float64: r8b.PCM_F64}


def make(lib):
    h = lib.r8b_batch_create(SRC, DST, L, 2.0, ATT, nch, -1)
    assert h, lib.r8b_last_error()
    return h


def run_clips(lib, h, x, out):
    lens = (C.c_longlong * nch)(*([T] * nch))
    outs = (C.c_longlong * nch)(*([P] * nch))
    p = lib.r8b_batch_resample_clips(h, C.c_void_p(x.data_ptr()), FMT[x.dtype], x.stride(0), lens,
                                     C.c_void_p(out.data_ptr()), FMT[out.dtype], out.stride(0), outs, C.c_void_p(stream))
    assert p == P, lib.r8b_last_error()


def run_loop(lib, h, x, out, zeros):
    """what a host does today: MaxInLen frames per call, zeros once the clips have ended, until P outputs exist (the last
    call's surplus lands in the slack columns of `out`)"""
    pcm = x.dtype != torch.float64
    B = x.element_size()
    done, pos = 0, 0
    while done < P:
        src, stride = (x.data_ptr() + pos * B, x.stride(0)) if pos < T else (zeros.data_ptr(), zeros.stride(0))
        dst = out.data_ptr() + done * out.element_size()
        if pcm:
            n = lib.r8b_batch_process_pcm(h, C.c_void_p(src), FMT[x.dtype], 0, stride, L, C.c_void_p(dst),
                                          FMT[out.dtype], 0, out.stride(0), C.c_void_p(stream))
        else:
            n = lib.r8b_batch_process(h, C.c_void_p(src), stride, L, C.c_void_p(dst), out.stride(0), C.c_void_p(stream))
        assert n >= 0, lib.r8b_last_error()
        done += n
        pos += L
    lib.r8b_batch_clear(h)


results = {}
for dtype, label in ((torch.float32, "F32 -> F32"), (torch.float64, "F64 -> F64")):
    x = x32 if dtype == torch.float32 else x64
    cap = new.r8b_batch_max_out_len(make(new))
    out_a = torch.zeros((nch, P + cap), dtype=dtype, device="cuda")
    out_b = torch.zeros((nch, P + cap), dtype=dtype, device="cuda")
    zeros = torch.zeros((nch, L), dtype=dtype, device="cuda")
    variants = [("resample_clips, this build", new, make(new), lambda lib, h: run_clips(lib, h, x, out_a))]
    for name, lib in libs:
        variants.append(("%s loop, %s" % ("process_pcm" if dtype == torch.float32 else "process", name), lib, make(lib),
                         lambda lib, h: run_loop(lib, h, x, out_b, zeros)))
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
    # (the two paths computed the same frames)
    same = bool(torch.equal(out_a[:, :P], out_b[:, :P]))
    print("%s, %d clips x %d frames -> %d frames each, %d repetitions after %d warm-up batches; outputs equal: %s" %
          (label, nch, T, P, args.reps, args.warmup, same))
    for name in times:
        t = times[name]
        print("  %-36s median %8.3f ms  (min %8.3f, max %8.3f)" % (name, statistics.median(t), min(t), max(t)))
    for _, lib, h, _ in variants:
        lib.r8b_batch_delete(h)
    del out_a, out_b, zeros
