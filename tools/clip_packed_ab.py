"""Cost of r8b_batch_resample_clips_packed against the strided clip call (profiles/clip_packed_ab.txt), by the method of
tools/clip_mix_ab.py: mono S16 clips -> F32, 44100 -> 96000 (180.15 dB), MaxInLen 16384, option "timing" 0, HIP events
around a whole call, the variants alternating call by call after a warm-up; median, minimum and maximum of the
repetitions.  --parent names the PARENT commit's libr8bsrc_hip.so (built from a checkout of it); its strided call is
the yardstick, measured twice on two objects (the A/A pair) next to this tree's packed call.  Without --parent this
tree's own strided call stands in and the output says so.
  case (a)  equal lengths: every clip T frames; the packed call does the work the strided one does.
  case (b)  lengths uniform in [T/4, T] (seeded): the bytes of the buffers packed and padded, the whole call, and the
            ingest and egress ALONE -- a pass-through object (Src == Dst: no stages, a call is the ingest kernel and the
            egress kernel per step).
--variants picks the variants to run (a profiler run wants the parent's strided and this tree's packed kernels alone:
--variants parent_a,packed, whose kernels have different names -- k_clip_rows_* / k_clip_packed_rows_*).
    python tools/clip_packed_ab.py --parent ../parent/r8brain-free-src_amd/libr8bsrc_hip.so [--reps 9] [--out FILE]"""
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
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--clips", type=int, default=1024)
ap.add_argument("--calls", type=int, default=8)
ap.add_argument("--variants", default="parent_a,parent_b,strided,packed")
ap.add_argument("--out", default=None)
args = ap.parse_args()

SRC, DST, L, ATT = 44100.0, 96000.0, 16384, 180.15
S16, F32 = r8b.PCM_S16, r8b.PCM_F32
n, T = args.clips, L * args.calls
cand = r8b.load()
# (the parent library has no packed entry: only the prototypes it needs)
parent = None
if args.parent:
    parent = C.CDLL(os.path.abspath(args.parent))
    for name, res, argt in r8b._capi.PROTOTYPES:
        if hasattr(parent, name):
            getattr(parent, name).restype, getattr(parent, name).argtypes = res, argt
    assert not hasattr(parent, "r8b_batch_resample_clips_packed"), "--parent is not the parent commit's library"
stream = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device="cuda")
g.manual_seed(7)
want = args.variants.split(",")


def ll(v):
    return (C.c_longlong * len(v))(*v)


def strided_call(lib, h, x, stride_in, in_len, out, stride_out, out_len):
    p = lib.r8b_batch_resample_clips(h, C.c_void_p(x.data_ptr()), S16, stride_in, ll(in_len), C.c_void_p(out.data_ptr()), F32,
                                     stride_out, ll(out_len), C.c_void_p(stream))
    assert p == max(out_len), lib.r8b_last_error()


def packed_call(h, x, in_off, in_len, out, out_off, out_len):
    p = cand.r8b_batch_resample_clips_packed(h, 0, 1, None, C.c_void_p(x.data_ptr()), S16, 0, 0, ll(in_off), ll(in_len),
                                             C.c_void_p(out.data_ptr()), F32, 0, 0, ll(out_off), ll(out_len),
                                             C.c_void_p(stream))
    assert p == max(out_len), cand.r8b_last_error()


def _offsets(lens):
    off = (C.c_longlong * len(lens))()
    total = cand.r8b_clip_pack_offsets(len(lens), ll(lens), 1, 1, off)
    return list(off), total


def measure(title, src, dst, in_len):
    """the variants on one set of lengths -> lines of text"""
    out_len = [cand.r8b_clip_out_len(src, dst, v) for v in in_len]
    Tm, P = max(in_len), max(out_len)
    in_off, in_total = _offsets(in_len)
    out_off, out_total = _offsets(out_len)
    padded = (torch.rand((n, Tm), generator=g, device="cuda") * 65536 - 32768).floor().clamp(-32768, 32767).to(torch.int16)
    packed = torch.cat([padded[i, :v] for i, v in enumerate(in_len)])
    assert packed.numel() == in_total
    libs = {"parent_a": parent or cand, "parent_b": parent or cand, "strided": cand}
    outs, runs = {}, []
    for name in want:
        lib = cand if name == "packed" else libs[name]
        h = lib.r8b_batch_create(src, dst, L, 2.0, ATT, n, -1)
        assert h, lib.r8b_last_error()
        if name == "packed":
            outs[name] = torch.zeros(out_total, dtype=torch.float32, device="cuda")
            runs.append((name, lib, h, lambda h, o=outs[name]: packed_call(h, packed, in_off, in_len, o, out_off, out_len)))
        else:
            outs[name] = torch.zeros((n, P), dtype=torch.float32, device="cuda")
            runs.append((name, lib, h, lambda h, lib=lib, o=outs[name]: strided_call(lib, h, padded, Tm, in_len, o, P, out_len)))
    times = {r[0]: [] for r in runs}
    for rep in range(args.warmup + args.reps):
        for name, _, h, fn in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(h)
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                times[name].append(e0.elapsed_time(e1))
    lines = [title,
             "  input  S16: packed %d B, padded %d B (%.3f); output F32: packed %d B, padded %d B (%.3f)" %
             (in_total * 2, n * Tm * 2, in_total / (n * Tm), out_total * 4, n * P * 4, out_total / (n * P))]
    if "packed" in outs:
        ref = next((outs[k] for k in ("parent_a", "strided", "parent_b") if k in outs), None)
        if ref is not None:
            same = all(torch.equal(outs["packed"][out_off[i]:out_off[i] + v], ref[i, :v]) for i, v in enumerate(out_len))
            lines.append("  every clip's packed region equals the strided call's valid frames bit for bit: %s" % same)
    label = {"parent_a": "strided call, parent library (A)", "parent_b": "strided call, parent library (A')",
             "strided": "strided call, this tree", "packed": "packed call, this tree"}
    for name in times:
        t = times[name]
        lines.append("  %-36s median %8.3f ms  (min %8.3f, max %8.3f)" % (label[name], statistics.median(t), min(t), max(t)))
    for _, lib, h, _ in runs:
        lib.r8b_batch_delete(h)
    return lines


rnd = random.Random(11)
spread = [rnd.randint(T // 4, T) for _ in range(n)]
lines = ["S16 -> F32, %d mono clips, T = %d frames, MaxInLen %d, %d repetitions after %d warm-up calls; parent library: %s" %
         (n, T, L, args.reps, args.warmup, "given" if parent else "NOT given (this tree's strided call stands in)")]
lines += measure("case (a): equal lengths, %g -> %g" % (SRC, DST), SRC, DST, [T] * n)
lines += measure("case (b): lengths uniform in [T/4, T], %g -> %g" % (SRC, DST), SRC, DST, spread)
lines += measure("case (b), ingest and egress alone (%g -> %g: no stages)" % (SRC, SRC), SRC, SRC, spread)
print("\n".join(lines))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
