"""Interleaved multichannel clips of unequal length in one call (include/r8bsrc.h r8b_batch_resample_clips_ex; kernels:
r8b_clip_frames.h; Python: BatchResampler.resample_clips(clip_channels=, interleaved=) / resample_clips_ex_ptr).

Every check runs on two tiers: the host emulation (tests/emul/Makefile; numpy buffers as "device" pointers) and
the product on the GPU (torch tensors).  The setup is tests/test_clips.py's: 44100 -> 48000 at 136.45 dB, MaxInLen 2000
(a step makes about 2177 outputs, so the windows cross the tiles' edges -- 2048 frames at K = 2, 1024 at K = 3, 256 at
K = 16, 64 at K = 64), six object channels, full-scale noise on the 16-bit grid (every format carries it exactly), NaN
(float formats) or the largest code (integer formats) past each clip's end and in the slack between clips, every output
byte pre-filled with a sentinel.  Interleaved clips lie T K + 1 samples apart on the input side and P K + 37 on the
output side, planar rows T + 1 and P + 37, so the bases sit at odd sample alignments.

The expectation everywhere is the EXISTING entry: a second object through r8b_batch_resample_clips on the
de-interleaved rows with every length repeated K times, re-interleaved in numpy and compared byte for byte, padding
zeros and untouched sentinels included.  No tolerance is involved (but for the one check against the compiled
reference, which has tests/cases.py's)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import cases
import r8b_oracle as O
from cases import PEAK_TOL, RMS_TOL
from conftest import ROOT

r8b = importlib.import_module("r8brain-free-src_amd")

BITS = {r8b.PCM_S16: 16, r8b.PCM_S24: 24, r8b.PCM_S32: 32}
NP_DTYPE = {r8b.PCM_F64: np.float64, r8b.PCM_F32: np.float32, r8b.PCM_S16: np.int16, r8b.PCM_S32: np.int32,
            r8b.PCM_S24: np.uint8}
BYTES = {r8b.PCM_F64: 8, r8b.PCM_F32: 4, r8b.PCM_S16: 2, r8b.PCM_S24: 3, r8b.PCM_S32: 4}
SEED = 0x5EEDC0DE12345678
SRC, DST, ATT, CHUNK = 44100.0, 48000.0, 136.45, 2000
NCH = 6
T = 6016            # frames per input clip / row
SENTINEL = 0xA5
SLACK = 37          # out_stride - P K (interleaved) / - P (planar)
LAYOUTS = [(True, True), (True, False), (False, True)]   # (input interleaved, output interleaved)


# ---------------------------------------------------------------- PCM bytes (as tests/test_clips.py has them)
def np_encode(v, fmt):
    if fmt in BITS:
        s = float(1 << (BITS[fmt] - 1))
        with np.errstate(invalid="ignore"):
            q = np.rint(v * s)
            q = np.where(np.isnan(q), 0.0, q)
            return np.clip(q, -s, s - 1.0).astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        return v.astype(np.float32) if fmt == r8b.PCM_F32 else v


def pack24(q):
    u = (q.astype(np.int64) & 0xFFFFFF)
    return np.stack([u & 255, (u >> 8) & 255, (u >> 16) & 255], axis=-1).astype(np.uint8)


def to_bytes(values, fmt):
    a = pack24(values) if fmt == r8b.PCM_S24 else np.ascontiguousarray(values.astype(NP_DTYPE[fmt]))
    return np.ascontiguousarray(a).view(np.uint8).reshape(values.shape[0], -1)


def encode_units(x, fmt, row_len):
    """fp64 rows [nch, T] -> the samples' bytes [nch, T, B]; past row_len[c]: NaN in the float formats, the largest code
    in the integer ones"""
    q = np.array(np_encode(np.where(np.isfinite(x), x, 0.0) if fmt in BITS else x, fmt))
    for c, n in enumerate(row_len):
        q[c, n:] = (1 << (BITS[fmt] - 1)) - 1 if fmt in BITS else np.nan
    return to_bytes(q, fmt).reshape(x.shape[0], x.shape[1], BYTES[fmt])


def signal(nch=NCH, variant=None):
    """full-scale noise on the 16-bit grid, [nch, T]; "hot": channel 4 times 1.5 and an Inf inside channel 3"""
    x = np.stack([O.splitmix_uniform(301 + c, T) for c in range(nch)])
    x = np.clip(np.rint(x * 32768.0), -32768.0, 32767.0) / 32768.0
    if variant == "hot":
        x[4] *= 1.5
        x[3, 700] = np.inf
    return x


def rows_of(per_clip, K):
    return [v for v in per_clip for _ in range(K)]


def lay_in(units, K, interleaved):
    """the caller's input buffer (bytes, 1-D) and its stride in samples; the slack holds the format's garbage"""
    nch, frames, B = units.shape
    garbage = units[0, frames - 1]   # (every clip is shorter than T)
    if interleaved:
        buf = np.empty((nch // K, frames * K + 1, B), dtype=np.uint8)
        buf[:] = garbage
        buf[:, :frames * K] = units.reshape(nch // K, K, frames, B).transpose(0, 2, 1, 3).reshape(nch // K, frames * K, B)
    else:
        buf = np.empty((nch, frames + 1, B), dtype=np.uint8)
        buf[:] = garbage
        buf[:, :frames] = units
    return buf.reshape(-1), buf.shape[1]


def lay_out(ref, K, P, B, interleaved):
    """the expected output buffer (bytes, 1-D) from the planar call's [nch, (P + SLACK) * B]"""
    assert np.all(ref[:, P * B:] == SENTINEL)
    if not interleaved:
        return ref.reshape(-1)
    nch = ref.shape[0]
    want = np.full((nch // K, P * K + SLACK, B), SENTINEL, dtype=np.uint8)
    want[:, :P * K] = ref[:, :P * B].reshape(nch // K, K, P, B).transpose(0, 2, 1, 3).reshape(nch // K, P * K, B)
    return want.reshape(-1)


# ---------------------------------------------------------------- the two tiers
@pytest.fixture(scope="module")
def emul():
    return cases.emul_lib()


class Tier:
    """lib: the emulation library (numpy buffers), or None: the product on the GPU (torch tensors)"""

    def __init__(self, lib):
        self.lib = lib
        self.gpu = lib is None

    def abi(self):
        return self.lib if self.lib is not None else r8b.load()

    def make(self, nch=NCH, src=SRC, dst=DST, dither=None, meters=False):
        a = r8b.BatchResampler(src, dst, CHUNK, 2.0, ATT, nch=nch, lib=self.lib)
        if dither is not None:
            a.set_dither(r8b.DITHER_TPDF, SEED, dither)
        if meters:
            a.enable_meters()
        return a

    def buf(self, host):
        host = np.ascontiguousarray(host)
        if not self.gpu:
            return host.copy()
        import torch
        return torch.from_numpy(host.view(np.uint8).reshape(-1).copy()).cuda()

    def sync(self):
        if self.gpu:
            import torch
            torch.cuda.synchronize()

    def ptr(self, b):
        return b.data_ptr() if self.gpu else b.ctypes.data

    def host(self, b):
        if not self.gpu:
            return b.view(np.uint8).reshape(-1)
        self.sync()
        return b.cpu().numpy()

    def out_len(self, in_len, src=SRC, dst=DST):
        return [self.abi().r8b_clip_out_len(src, dst, n) for n in in_len]

    def raw(self, a, K, xin, in_fmt, in_il, in_stride, in_len, out, out_fmt, out_il, out_stride, out_len, stream=0):
        """the C entry as it is: its return value"""
        return a._lib.r8b_batch_resample_clips_ex(
            a._h, K, C.c_void_p(self.ptr(xin)), in_fmt, int(in_il), in_stride, (C.c_longlong * len(in_len))(*in_len),
            C.c_void_p(self.ptr(out)), out_fmt, int(out_il), out_stride, (C.c_longlong * len(out_len))(*out_len),
            C.c_void_p(stream))

    def prepare_ex(self, K, units, in_il, out_fmt, out_il, out_len):
        """-> (input buffer, in_stride, output buffer full of sentinels, out_stride)"""
        xb, in_stride = lay_in(units, K, in_il)
        P = max(out_len)
        out_stride = P * K + SLACK if out_il else P + SLACK
        rows = units.shape[0] // K if out_il else units.shape[0]
        bufs = (self.buf(xb), in_stride, self.buf(np.full(rows * out_stride * BYTES[out_fmt], SENTINEL, dtype=np.uint8)),
                out_stride)
        self.sync()
        return bufs

    def enqueue_ex(self, a, K, bufs, in_fmt, in_il, in_len, out_fmt, out_il, out_len, stream=0):
        xin, in_stride, out, out_stride = bufs
        return a.resample_clips_ex_ptr(K, self.ptr(xin), in_fmt, in_il, in_stride, in_len, self.ptr(out), out_fmt, out_il,
                                       out_stride, out_len, stream)

    def run_ex(self, a, K, units, in_fmt, in_il, in_len, out_fmt, out_il, out_len):
        """-> (the whole output buffer's bytes, P)"""
        bufs = self.prepare_ex(K, units, in_il, out_fmt, out_il, out_len)
        p = self.enqueue_ex(a, K, bufs, in_fmt, in_il, in_len, out_fmt, out_il, out_len)
        return self.host(bufs[2]), p


_REF = {}


def reference(tier, K, x, key, in_fmt, in_len, out_fmt, out_len, src=SRC, dst=DST, dither=None, meters=False):
    """(bytes [nch, (P + SLACK) * B], meters or None) of the EXISTING r8b_batch_resample_clips on a second object: the
    de-interleaved rows, every length K times.  Computed once per tier and case and never modified.  key: names x"""
    nch = x.shape[0]
    k = (tier.gpu, K, nch, key, in_fmt, tuple(in_len), out_fmt, tuple(out_len), src, dst, dither, meters)
    if k not in _REF:
        rl, ro = rows_of(in_len, K), rows_of(out_len, K)
        units = encode_units(x, in_fmt, rl)
        P, B = max(ro), BYTES[out_fmt]
        b = tier.make(nch, src, dst, dither, meters)
        xin = tier.buf(units)
        out = tier.buf(np.full((nch, (P + SLACK) * B), SENTINEL, dtype=np.uint8))
        tier.sync()
        assert b.resample_clips_ptr(tier.ptr(xin), in_fmt, T, rl, tier.ptr(out), out_fmt, P + SLACK, ro) == P
        got = tier.host(out).reshape(nch, (P + SLACK) * B).copy()
        got.setflags(write=False)
        _REF[k] = (got, b.read_meters() if meters else None)
    return _REF[k]


def check_ex(tier, K, x, key, in_fmt, in_len, out_fmt, out_len, layouts=LAYOUTS, src=SRC, dst=DST, dither=None,
             meters=False):
    """the _ex call in each of the layouts against the planar reference: bytes, and meters if on"""
    ref, ref_m = reference(tier, K, x, key, in_fmt, in_len, out_fmt, out_len, src, dst, dither, meters)
    units = encode_units(x, in_fmt, rows_of(in_len, K))
    P, B = max(out_len), BYTES[out_fmt]
    for in_il, out_il in layouts:
        a = tier.make(x.shape[0], src, dst, dither, meters)
        got, p = tier.run_ex(a, K, units, in_fmt, in_il, in_len, out_fmt, out_il, out_len)
        assert p == P
        want = lay_out(ref, K, P, B, out_il)
        assert got.shape == want.shape
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, ("layout", in_il, out_il, "bytes differing", bad.size, "first at", int(bad[0]))
        if meters:
            m = a.read_meters()
            for name in ("peak", "clipped", "nonfinite"):
                assert np.array_equal(m[name], ref_m[name]), (name, in_il, out_il, m[name], ref_m[name])
    return ref, ref_m


# ---------------------------------------------------------------- 1. layouts x formats
IN_LEN = {2: {"a": [1, 2000, 6001], "b": [0, 1999, 4500]}, 3: {"a": [1999, 6001], "b": [0, 4500]}}


def out_len_case(tier, K, case):
    """natural lengths of the two input sets; "a_cut": one clip cut short, one zeroed, one 3000 frames past its natural
    end (K = 3 has two clips: zeroed and past in "a_cut", cut short in "a_short")"""
    in_len = IN_LEN[K][case[0]]
    nat = tier.out_len(in_len)
    if case in ("a", "b"):
        return in_len, nat
    if K == 2:
        assert case == "a_cut"
        return in_len, [0, nat[1] - 100, nat[2] + 3000]
    return in_len, ([0, nat[1] + 3000] if case == "a_cut" else [nat[0] - 100, nat[1]])


CASES = [(2, "a"), (2, "b"), (2, "a_cut"), (3, "a"), (3, "b"), (3, "a_cut"), (3, "a_short")]
FORMAT_PAIRS = [(f, f) for f in (r8b.PCM_F64, r8b.PCM_F32, r8b.PCM_S16, r8b.PCM_S24, r8b.PCM_S32)] + \
    [(r8b.PCM_S16, r8b.PCM_F32)]


def check_layouts(tier, K, case, fmts):
    in_len, out_len = out_len_case(tier, K, case)
    ref, _ = check_ex(tier, K, signal(), "noise", fmts[0], in_len, fmts[1], out_len)
    # (the rows are no silence: the longest clip's bytes differ from the encoded zero's)
    if max(out_len) > 1000:
        assert np.count_nonzero(ref[NCH - 1, :max(out_len) * BYTES[fmts[1]]]) > 1000


@pytest.mark.parametrize("fmts", FORMAT_PAIRS)
@pytest.mark.parametrize("K,case", CASES)
def test_layouts_emulated(emul, K, case, fmts):
    check_layouts(Tier(emul), K, case, fmts)


@pytest.mark.gpu
@pytest.mark.parametrize("fmts", FORMAT_PAIRS)
@pytest.mark.parametrize("K,case", CASES)
def test_layouts_gpu(K, case, fmts):
    check_layouts(Tier(None), K, case, fmts)


# ---------------------------------------------------------------- 2. dither and meters
def check_dither_and_meters(tier, K, fmt, first_channel):
    in_len, out_len = out_len_case(tier, K, "a_cut" if first_channel else "a")
    x = signal(variant="hot")
    ref, m = check_ex(tier, K, x, "hot", r8b.PCM_F64, in_len, fmt, out_len, dither=first_channel, meters=True)
    # (the dither did something, and so did the hot channel and the Inf)
    plain, _ = reference(tier, K, x, "hot", r8b.PCM_F64, in_len, fmt, out_len)
    assert not np.array_equal(ref, plain)
    assert m["clipped"][4] > 100 and m["nonfinite"][3] > 0 and m["peak"][4] > 1.0


@pytest.mark.parametrize("first_channel", [0, 5])
@pytest.mark.parametrize("fmt", [r8b.PCM_S16, r8b.PCM_S24])
@pytest.mark.parametrize("K", [2, 3])
def test_dither_and_meters_emulated(emul, K, fmt, first_channel):
    check_dither_and_meters(Tier(emul), K, fmt, first_channel)


@pytest.mark.gpu
@pytest.mark.parametrize("first_channel", [0, 5])
@pytest.mark.parametrize("fmt", [r8b.PCM_S16, r8b.PCM_S24])
@pytest.mark.parametrize("K", [2, 3])
def test_dither_and_meters_gpu(K, fmt, first_channel):
    check_dither_and_meters(Tier(None), K, fmt, first_channel)


# ---------------------------------------------------------------- 3. K = 1: a frame-major clip is a row
def check_single_channel_clips(tier):
    in_len = [0, 1, 1999, 2000, 4500, 6001]
    check_ex(tier, 1, signal(), "noise", r8b.PCM_S16, in_len, r8b.PCM_F32, tier.out_len(in_len),
             layouts=[(True, True), (False, False), (True, False)])


def test_single_channel_clips_emulated(emul):
    check_single_channel_clips(Tier(emul))


@pytest.mark.gpu
def test_single_channel_clips_gpu():
    check_single_channel_clips(Tier(None))


# ---------------------------------------------------------------- 4. wide clips
def check_wide(tier, K, nch, in_len):
    check_ex(tier, K, signal(nch), "noise%d" % nch, r8b.PCM_S16, in_len, r8b.PCM_F32, tier.out_len(in_len),
             layouts=[(True, True)])


def test_wide_16_emulated(emul):
    check_wide(Tier(emul), 16, 32, [700, 2500])


@pytest.mark.gpu
def test_wide_16_gpu():
    check_wide(Tier(None), 16, 32, [700, 2500])


@pytest.mark.gpu
def test_wide_64_gpu():
    check_wide(Tier(None), 64, 64, [2500])


def check_wide_metered(tier):
    """K = 33 on 66 channels, dither and meters on: a tile is 64 frames x 33 channels, so every step of a wave's walk is
    another channel (a commit per sample) and 33 * 64 is no multiple of 256 -- the waves of a workgroup leave the walk at
    different steps.  The emulation folds each thread's record on its own; the wave reduction runs on the device only"""
    in_len = [2500, 700]
    ref, m = check_ex(tier, 33, signal(66, "hot"), "hot66", r8b.PCM_F64, in_len, r8b.PCM_S16, tier.out_len(in_len),
                      layouts=[(True, True), (False, True)], dither=5, meters=True)
    assert m["clipped"][4] > 10 and m["nonfinite"][3] > 0 and m["peak"][4] > 1.0 and m["peak"][65] > 0.5


def test_wide_metered_emulated(emul):
    check_wide_metered(Tier(emul))


@pytest.mark.gpu
def test_wide_metered_gpu():
    check_wide_metered(Tier(None))


# ---------------------------------------------------------------- 5. Src == Dst: converts and masks
def check_pass_through(tier):
    x = signal()
    for in_len, out_len in (([5, 2048, 2049], [5, 2048, 2049]), ([7, 100, 0], [3, 150, 50])):
        check_ex(tier, 2, x, "noise", r8b.PCM_S16, in_len, r8b.PCM_F32, out_len, src=44100.0, dst=44100.0)


def test_pass_through_emulated(emul):
    check_pass_through(Tier(emul))


@pytest.mark.gpu
def test_pass_through_gpu():
    check_pass_through(Tier(None))


# ---------------------------------------------------------------- 6. errors
def check_errors(tier):
    K, F = 2, r8b.PCM_F64
    in_len, out_len = out_len_case(tier, K, "a")
    x = signal()
    units = encode_units(x, F, rows_of(in_len, K))
    P, max_in = max(out_len), max(in_len)
    want = {il: lay_out(reference(tier, K, x, "noise", F, in_len, F, out_len)[0], K, P, 8, il) for il in (True, False)}
    a = tier.make()
    for in_il, out_il in LAYOUTS:
        xin, in_stride, out, out_stride = tier.prepare_ex(K, units, in_il, F, out_il, out_len)

        def call(k=K, i_stride=in_stride, o_stride=out_stride, o_len=out_len, obj=a):
            return tier.raw(obj, k, xin, F, in_il, i_stride, in_len, out, F, out_il, o_stride, o_len)

        for bad_k in (0, -1, 4, 65, 128):
            assert call(k=bad_k) == -1, bad_k
            assert b"clip_channels" in a._lib.r8b_last_error()
        assert call(i_stride=max_in * (K if in_il else 1) - 1) == -1
        assert b"in_stride" in a._lib.r8b_last_error()
        assert call(o_stride=P * (K if out_il else 1) - 1) == -1
        assert b"out_stride" in a._lib.r8b_last_error()
        # an object in mid-stream
        b = tier.make()
        blk, res = tier.buf(np.zeros((NCH, CHUNK))), tier.buf(np.zeros((NCH, max(b.max_out_len, 1))))
        tier.sync()
        b.process_ptr(tier.ptr(blk), CHUNK, CHUNK, tier.ptr(res), max(b.max_out_len, 1))
        assert call(obj=b) == -1
        assert b"processed samples" in b._lib.r8b_last_error()
        # P == 0: nothing is launched
        assert call(o_len=[0] * len(out_len)) == 0
        assert np.all(tier.host(out) == SENTINEL)
        # ... none of which used the object up or changed it
        assert call() == P
        assert np.array_equal(tier.host(out), want[out_il])


def test_errors_emulated(emul):
    check_errors(Tier(emul))


@pytest.mark.gpu
def test_errors_gpu():
    check_errors(Tier(None))


# ---------------------------------------------------------------- 7. back to back on one stream
@pytest.mark.gpu
def test_back_to_back_on_one_stream_gpu():
    """two calls with different lengths enqueued on one non-default stream, nothing waits in between: each call's kernels
    read ITS lengths"""
    import torch
    tier, K = Tier(None), 2
    x = signal()
    calls = []
    for in_len, extra in (([1, 2000, 6001], 0), ([6001, 0, 1999], 40)):
        out_len = [n + extra for n in tier.out_len(in_len)]
        ref, _ = reference(tier, K, x, "noise", r8b.PCM_S16, in_len, r8b.PCM_F64, out_len)
        bufs = tier.prepare_ex(K, encode_units(x, r8b.PCM_S16, rows_of(in_len, K)), True, r8b.PCM_F64, True, out_len)
        calls.append((in_len, out_len, bufs, lay_out(ref, K, max(out_len), 8, True)))
    a = tier.make()
    s = torch.cuda.Stream()
    for in_len, out_len, bufs, _ in calls:
        assert tier.enqueue_ex(a, K, bufs, r8b.PCM_S16, True, in_len, r8b.PCM_F64, True, out_len,
                               s.cuda_stream) == max(out_len)
    s.synchronize()
    for _, _, bufs, want in calls:
        assert np.array_equal(tier.host(bufs[2]), want)


# ---------------------------------------------------------------- 8. the Python entry
@pytest.mark.gpu
def test_resample_clips_tensors_gpu():
    import torch
    tier, K = Tier(None), 2
    x = signal()
    in_len = [1, 2000, 6001]
    out_len = tier.out_len(in_len)
    P = max(out_len)
    ref, _ = reference(tier, K, x, "noise", r8b.PCM_S16, in_len, r8b.PCM_F32, out_len)
    rows = np.ascontiguousarray(ref[:, :P * 4]).view(np.float32)   # [NCH, P]
    units = encode_units(x, r8b.PCM_S16, rows_of(in_len, K))
    xt = torch.from_numpy(np.ascontiguousarray(units.reshape(3, K, T, 2).transpose(0, 2, 1, 3)).view(np.int16)
                          .reshape(3, T, K).copy()).cuda()
    a = tier.make()
    out, ol = a.resample_clips(xt, in_len, out_format=r8b.PCM_F32, clip_channels=K, interleaved=True)
    assert ol == out_len and tuple(out.shape) == (3, P, K) and out.dtype == torch.float32
    torch.cuda.synchronize()
    # (what the pointer entry wrote, by check_layouts: the planar rows re-interleaved)
    want = rows.reshape(3, K, P).transpose(0, 2, 1)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    got, p = tier.run_ex(a, K, units, r8b.PCM_S16, True, in_len, r8b.PCM_F32, True, out_len)
    assert p == P
    ptr_entry = got.reshape(3, (P * K + SLACK) * 4)[:, :P * K * 4].copy().view(np.float32).reshape(3, P, K)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ptr_entry.view(np.uint32))
    # planar out of interleaved in, into a given buffer
    buf = torch.full((NCH, P + SLACK), -7.0, dtype=torch.float32, device="cuda")
    res, _ = a.resample_clips(xt, in_len, out_format=r8b.PCM_F32, out=buf, clip_channels=K, interleaved=True,
                              out_interleaved=False)
    assert tuple(res.shape) == (NCH, P) and res.data_ptr() == buf.data_ptr()
    torch.cuda.synchronize()
    assert np.array_equal(res.cpu().numpy().view(np.uint32), rows.view(np.uint32))
    assert bool(torch.all(buf[:, P:] == -7.0))


# ---------------------------------------------------------------- 9. against the compiled reference
def check_against_reference(tier, refwrap):
    K, F = 2, r8b.PCM_F64
    in_len, out_len = out_len_case(tier, K, "a")
    x = signal()
    a = tier.make()
    got, p = tier.run_ex(a, K, encode_units(x, F, rows_of(in_len, K)), F, True, in_len, F, True, out_len)
    got = got.view(np.float64).reshape(NCH // K, p * K + SLACK)[:, :p * K].reshape(NCH // K, p, K)
    for c in range(NCH):
        n_in, n = in_len[c // K], out_len[c // K]
        ref = refwrap.RefResampler(SRC, DST, CHUNK, 2.0, ATT)
        feed = np.zeros((-(-max(n_in, 1) // CHUNK) + 6) * CHUNK)
        feed[:n_in] = x[c, :n_in]
        want = ref.stream(feed)
        assert len(want) >= n
        d = got[c // K, :n, c % K] - want[:n]
        r = float(np.sqrt(np.mean(d * d))) if n else 0.0
        pk = float(np.max(np.abs(d))) if n else 0.0
        print("channel %d: %d frames, rms %.3g peak %.3g" % (c, n, r, pk))
        assert r <= RMS_TOL and pk <= PEAK_TOL, (c, n, r, pk)


def test_against_reference_emulated(emul, refwrap):
    check_against_reference(Tier(emul), refwrap)


@pytest.mark.gpu
def test_against_reference_gpu(refwrap):
    check_against_reference(Tier(None), refwrap)
