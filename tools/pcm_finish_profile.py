"""Workload of the cost measurement: 1024 channels x 16384 frames, 44100 -> 96000 (180.15 dB), S16 out planar and
interleaved; plain egress, dither only, meters only, both.  Run under rocprofv3 --kernel-trace --stats: the variants are
different kernels, so one trace separates them (profiles/pcm_finish.md):
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- \
        python tools/pcm_finish_profile.py [input level, default 1.1]"""
import importlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
r8b = importlib.import_module("r8brain-free-src_amd")
nch, L, calls = 1024, 16384, 12
# input level (argument, default 1.1): uniform noise of that amplitude; 1.1 clips one output in ten at S16, 0.5 none
gain = float(sys.argv[1]) if len(sys.argv) > 1 else 1.1
g = torch.Generator(device="cuda"); g.manual_seed(3)
x = (torch.rand((nch, L), generator=g, dtype=torch.float64, device="cuda") * 2 - 1) * gain
for interleaved in (False, True):
    objs = []
    for dither, meter in ((0, 0), (1, 0), (0, 1), (1, 1)):
        a = r8b.BatchResampler(44100.0, 96000.0, L, 2.0, 180.15, nch=nch)
        if dither: a.set_dither(r8b.DITHER_TPDF, 12345)
        if meter: a.enable_meters()
        objs.append(a)
    cap = objs[0].max_out_len
    out = torch.zeros((cap, nch) if interleaved else (nch, cap), dtype=torch.int16, device="cuda")
    # alternate the variants call by call
    for i in range(calls):
        for a in objs:
            n = a.process_pcm_ptr(x.data_ptr(), r8b.PCM_F64, False, L, L, out.data_ptr(), r8b.PCM_S16, interleaved,
                                  nch if interleaved else cap)
    torch.cuda.synchronize()
    print("interleaved", interleaved, "outputs per call", n, flush=True)
    for a in objs[2:]:
        m = a.read_meters()
        print("meters: peak max %.4f clipped %d nonfinite %d" % (m["peak"].max(), m["clipped"].sum(), m["nonfinite"].sum()))
