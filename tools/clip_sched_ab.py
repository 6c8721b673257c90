"""Cost of r8b_batch_resample_clips_sched -- finished clips dropped from the later steps, clips riding longest first --
against the packed clip call of the parent commit (profiles/clip_sched_ab.txt), by the method and on the workload of
tools/clip_packed_ab.py: 1024 mono S16 clips -> F32, T = 131072 frames, 44100 -> 96000 (180.15 dB), MaxInLen 16384,
option "timing" 0, HIP events around a whole call, the variants alternating call by call after a warm-up; median,
minimum and maximum of the repetitions.  --parent names the PARENT commit's libr8bsrc_hip.so (built from a checkout of
it); its packed call is the yardstick, measured on two objects (the A/A pair) next to this tree's call with flags 0,
DROP_FINISHED, and DROP_FINISHED | LONGEST_FIRST.  Without --parent this tree's own packed entry stands in and the
output says so.
  case (a)  equal lengths: nothing can drop, nothing to sort.
  case (b)  lengths uniform in [T/4, T] (seeded), in random order.
  case (c)  one clip of T (the first) among clips of T/8.
Beside each variant of this tree: clip_channel_steps / (clip_steps * channels) of its object (r8b_batch_stat), the share
of the stage work the call had left, and whether its output equals the parent's bit for bit (flags 0 and DROP_FINISHED
must; LONGEST_FIRST pairs the channels differently and need not).
    python tools/clip_sched_ab.py --parent ../parent/r8brain-free-src_amd/libr8bsrc_hip.so [--reps 9] [--out FILE]"""
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
ap.add_argument("--variants", default="parent_a,parent_b,flags0,drop,drop_sorted")
ap.add_argument("--out", default=None)
args = ap.parse_args()

SRC, DST, L, ATT = 44100.0, 96000.0, 16384, 180.15
S16, F32 = r8b.PCM_S16, r8b.PCM_F32
FLAGS = {"flags0": 0, "drop": r8b.CLIPS_DROP_FINISHED, "drop_sorted": r8b.CLIPS_DROP_FINISHED | r8b.CLIPS_LONGEST_FIRST}
n, T = args.clips, L * args.calls
cand = r8b.load()
# (the parent library has no scheduled entry: only the prototypes it has)
parent = None
if args.parent:
    parent = C.CDLL(os.path.abspath(args.parent))
    for name, res, argt in r8b._capi.PROTOTYPES:
        if hasattr(parent, name):
            getattr(parent, name).restype, getattr(parent, name).argtypes = res, argt
    assert not hasattr(parent, "r8b_batch_resample_clips_sched"), "--parent is not the parent commit's library"
stream = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device="cuda")
g.manual_seed(7)
want = args.variants.split(",")


def ll(v):
    return (C.c_longlong * len(v))(*v)


def packed_call(lib, h, x, in_off, in_len, out, out_off, out_len):
    p = lib.r8b_batch_resample_clips_packed(h, 0, 1, None, C.c_void_p(x.data_ptr()), S16, 0, 0, ll(in_off), ll(in_len),
                                            C.c_void_p(out.data_ptr()), F32, 0, 0, ll(out_off), ll(out_len), C.c_void_p(stream))
    assert p == max(out_len), lib.r8b_last_error()


def sched_call(h, x, in_off, in_len, out, out_off, out_len, flags):
    p = cand.r8b_batch_resample_clips_sched(h, 0, 1, None, C.c_void_p(x.data_ptr()), S16, 0, 0, ll(in_off), ll(in_len),
                                            C.c_void_p(out.data_ptr()), F32, 0, 0, ll(out_off), ll(out_len), flags,
                                            C.c_void_p(stream))
    assert p == max(out_len), cand.r8b_last_error()


def _offsets(lens):
    off = (C.c_longlong * len(lens))()
    total = cand.r8b_clip_pack_offsets(len(lens), ll(lens), 1, 1, off)
    return list(off), total


def measure(title, in_len):
    """the variants on one set of lengths -> lines of text"""
    out_len = [cand.r8b_clip_out_len(SRC, DST, v) for v in in_len]
    in_off, in_total = _offsets(in_len)
    out_off, out_total = _offsets(out_len)
    packed = (torch.rand(in_total, generator=g, device="cuda") * 65536 - 32768).floor().clamp(-32768, 32767).to(torch.int16)
    outs, runs = {}, []
    for name in want:
        lib = cand if name in FLAGS else (parent or cand)
        h = lib.r8b_batch_create(SRC, DST, L, 2.0, ATT, n, -1)
        assert h, lib.r8b_last_error()
        outs[name] = torch.zeros(out_total, dtype=torch.float32, device="cuda")
        if name in FLAGS:
            runs.append((name, lib, h, lambda h, o=outs[name], f=FLAGS[name]: sched_call(h, packed, in_off, in_len, o, out_off, out_len, f)))
        else:
            runs.append((name, lib, h, lambda h, lib=lib, o=outs[name]: packed_call(lib, h, packed, in_off, in_len, o, out_off, out_len)))
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
    lines = [title, "  frames: sum of the lengths %d, clips x longest %d (%.3f)" % (sum(in_len), n * max(in_len), sum(in_len) / (n * max(in_len)))]
    label = {"parent_a": "packed call, parent library (A)", "parent_b": "packed call, parent library (A')",
             "flags0": "this tree, flags 0", "drop": "this tree, DROP_FINISHED", "drop_sorted": "this tree, DROP | LONGEST_FIRST"}
    if not parent:
        label["parent_a"], label["parent_b"] = "packed call, THIS tree (A)", "packed call, THIS tree (A')"
    ref = next((outs[k] for k in ("parent_a", "parent_b") if k in outs), None)
    base = statistics.median(times["parent_a"]) if "parent_a" in times else None
    for name, lib, h, _ in runs:
        t = times[name]
        line = "  %-34s median %8.3f ms  (min %8.3f, max %8.3f)" % (label[name], statistics.median(t), min(t), max(t))
        if name in FLAGS:
            steps, chans = lib.r8b_batch_stat(h, b"clip_steps"), lib.r8b_batch_stat(h, b"clip_channel_steps")
            line += "  stage share %.3f" % (chans / (steps * n))
            if base:
                line += "  time / A %.3f" % (statistics.median(t) / base)
            if ref is not None:
                same = torch.equal(outs[name], ref)
                line += "  bitwise A: %s" % same
                if not same:
                    line += " (max |diff| %.3g)" % float((outs[name] - ref).abs().max())
        lines.append(line)
    for _, lib, h, _ in runs:
        lib.r8b_batch_delete(h)
    return lines


rnd = random.Random(11)
spread = [rnd.randint(T // 4, T) for _ in range(n)]
lines = ["S16 -> F32, %d mono clips packed on both sides, T = %d frames, %g -> %g, MaxInLen %d, %d repetitions after %d warm-up "
         "calls; parent library: %s" % (n, T, SRC, DST, L, args.reps, args.warmup,
                                       "given" if parent else "NOT given (this tree's packed entry stands in)")]
lines += measure("case (a): equal lengths", [T] * n)
lines += measure("case (b): lengths uniform in [T/4, T], random order", spread)
lines += measure("case (c): one clip of T among clips of T/8", [T] + [T // 8] * (n - 1))
print("\n".join(lines))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
