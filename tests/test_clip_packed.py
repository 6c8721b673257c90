"""Clips packed end to end: offsets in the place of a stride (include/r8bsrc.h r8b_batch_resample_clips_packed,
r8b_clip_pack_offsets; kernels: r8b_clip_packed.h; Python: BatchResampler.resample_clips_packed / _packed_ptr).

Every check runs on two tiers: the host emulation (tests/emul/Makefile; numpy buffers as "device" pointers) and
the product on the GPU (torch tensors).  The setup and the helpers are tests/test_clip_frames.py's: 44100 -> 48000 at
136.45 dB, MaxInLen 2000 (a step makes about 2177 outputs), full-scale noise on the 16-bit grid.  An object takes six
clips of K channels, K in {1, 2, 3, 6, 33, 64}, of lengths {0, 1, 1999, 2000, 4500, 6001}: the windows of 2000 frames
and the tiles (2048 frames at K = 1, 1024 at 2, 512 at 3, 256 at 6, 64 at 33 and 64) are crossed at every K.

The expectation of every byte check is the EXISTING strided call (r8b_batch_resample_clips_ex / _mix) on a second
object, given the same clips laid out padded (planar rows of T frames).  Staging rows, codec, dither key and meters are
the same code, so the comparison is byte for byte and has no tolerance.

Packed buffers hold the clips in a permuted order with gaps of 0, 1 and 37 elements between them (and 37 behind the
last), so bases are odd and unaligned; NaN (float formats) or the largest code (integer formats) fills every input gap,
and every output byte is pre-filled with a sentinel, which must survive wherever no clip's region lies."""
import ctypes as C
import importlib

import numpy as np
import pytest

import test_clip_frames as F
import cases
from conftest import ROOT

r8b = importlib.import_module("r8brain-free-src_amd")

T, SLACK, SENTINEL, BYTES, CHUNK = F.T, F.SLACK, F.SENTINEL, F.BYTES, F.CHUNK
F64, F32, S16, S24, S32 = r8b.PCM_F64, r8b.PCM_F32, r8b.PCM_S16, r8b.PCM_S24, r8b.PCM_S32
LENGTHS = [0, 1, 1999, 2000, 4500, 6001]
NCLIPS = 6
KS = [1, 2, 3, 6, 33, 64]
GAPS = [0, 1, 37]
ORDER = [3, 0, 5, 1, 4, 2]          # the order in which the clips lie in a packed buffer
ALL_LAYOUTS = [(True, True), (True, False), (False, True), (False, False)]   # (input interleaved, output interleaved)


@pytest.fixture(scope="module")
def emul():
    return cases.emul_lib()


# ---------------------------------------------------------------- packed buffers
def pack_offsets(sizes, order=ORDER, gaps=GAPS):
    """element offsets of regions of `sizes` elements laid in `order` with the gaps in turn between them, and the
    buffer's size (a last gap of 37 behind the last region)"""
    off, pos = [0] * len(sizes), 0
    for j, i in enumerate(order):
        pos += gaps[j % len(gaps)] if j else 0
        off[i] = pos
        pos += sizes[i]
    return off, pos + 37


def region(rows, n, interleaved):
    """[Kc, >= n, B] -> the clip's n * Kc elements [n * Kc, B] in the layout"""
    r = rows[:, :n]
    return (r.transpose(1, 0, 2) if interleaved else r).reshape(-1, rows.shape[2])


def pack_in(units, Kc, interleaved, in_len, order=ORDER, gaps=GAPS):
    """units [nclips * Kc, T, B] -> (bytes of the packed input buffer, offsets); garbage between the regions"""
    off, total = pack_offsets([n * Kc for n in in_len], order, gaps)
    buf = np.empty((total, units.shape[2]), dtype=np.uint8)
    buf[:] = units[0, units.shape[1] - 1]        # (every clip is shorter than T: the format's garbage)
    for i, n in enumerate(in_len):
        buf[off[i]:off[i] + n * Kc] = region(units[i * Kc:(i + 1) * Kc], n, interleaved)
    return buf.reshape(-1), off


def pack_out(ref, K, B, interleaved, out_len, off, total):
    """the expected packed output buffer from the strided planar call's bytes [nclips * K, >= max(out_len) * B]"""
    want = np.full((total, B), SENTINEL, dtype=np.uint8)
    for i, n in enumerate(out_len):
        rows = ref[i * K:(i + 1) * K, :n * B].reshape(K, n, B)
        want[off[i]:off[i] + n * K] = region(rows, n, interleaved)
    return want.reshape(-1)


class Tier(F.Tier):
    """tests/test_clip_frames.py's tiers with the packed entry"""

    def sentinels(self, nbytes):
        b = self.buf(np.full(nbytes, SENTINEL, dtype=np.uint8))
        self.sync()
        return b

    def raw_packed(self, a, Kin, K, mix, xin, in_fmt, in_il, in_stride, in_off, in_len, out, out_fmt, out_il, out_stride,
                   out_off, out_len, stream=0):
        """the C entry as it is: its return value.  mix / in_off / out_off: sequences, or None for a NULL pointer"""
        def ll(v):
            return None if v is None else (C.c_longlong * len(v))(*v)
        m = None if mix is None else (C.c_double * len(mix))(*mix)
        return a._lib.r8b_batch_resample_clips_packed(
            a._h, Kin, K, m, C.c_void_p(self.ptr(xin)), in_fmt, int(in_il), in_stride, ll(in_off), ll(in_len),
            C.c_void_p(self.ptr(out)), out_fmt, int(out_il), out_stride, ll(out_off), ll(out_len), C.c_void_p(stream))


_REF = {}


def reference(tier, K, M, x, key, in_fmt, in_len, out_fmt, out_len, dither=None, meters=False):
    """(bytes [nclips * K, (P + SLACK) * B], meters or None) of the EXISTING strided call on a second object -- _ex, or
    _mix with the matrix M -- on planar rows of T frames, garbage past each clip's end.  Computed once per tier and
    case and never modified.  key: names x"""
    k = (tier.gpu, K, None if M is None else np.asarray(M).tobytes(), key, in_fmt, tuple(in_len), out_fmt, tuple(out_len),
         dither, meters)
    if k not in _REF:
        Kin = K if M is None else np.shape(M)[1]
        nclips = x.shape[0] // Kin
        units = F.encode_units(x, in_fmt, F.rows_of(in_len, Kin))
        P, B = max(out_len), BYTES[out_fmt]
        b = tier.make(nclips * K, dither=dither, meters=meters)
        xin = tier.buf(units)
        out = tier.sentinels(nclips * K * (P + SLACK) * B)
        if M is None:
            p = b.resample_clips_ex_ptr(K, tier.ptr(xin), in_fmt, False, T, in_len, tier.ptr(out), out_fmt, False, P + SLACK,
                                        out_len)
        else:
            p = b.resample_clips_mix_ptr(Kin, K, M, tier.ptr(xin), in_fmt, False, T, in_len, tier.ptr(out), out_fmt, False,
                                         P + SLACK, out_len)
        assert p == P
        got = tier.host(out).reshape(nclips * K, (P + SLACK) * B).copy()
        got.setflags(write=False)
        _REF[k] = (got, b.read_meters() if meters else None)
    return _REF[k]


_SIGNAL = {}


def signal(nch, variant=None):
    if (nch, variant) not in _SIGNAL:
        _SIGNAL[nch, variant] = F.signal(nch, variant)
        _SIGNAL[nch, variant].setflags(write=False)
    return _SIGNAL[nch, variant]


def assert_same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "bytes differing", bad.size, "first at", int(bad[0]))


def check_packed(tier, K, M, x, key, in_fmt, in_len, out_fmt, out_len, layouts, in_packed=True, out_packed=True, dither=None,
                 meters=False, order=ORDER):
    """the packed call in each layout pair against the strided reference: every byte of the output buffer (a packed
    side: each clip's region is the strided result's valid bytes and everything else still the sentinel; a strided
    one: the strided call's whole buffer, padding zeros included), and the meters if on"""
    ref, ref_m = reference(tier, K, M, x, key, in_fmt, in_len, out_fmt, out_len, dither, meters)
    Kin = K if M is None else np.shape(M)[1]
    nclips = len(in_len)
    units = F.encode_units(x, in_fmt, F.rows_of(in_len, Kin))
    P, B = max(out_len), BYTES[out_fmt]
    for in_il, out_il in layouts:
        if in_packed:
            xb, in_off = pack_in(units, Kin, in_il, in_len, order)
            in_stride = 0
        else:
            (xb, in_stride), in_off = F.lay_in(units, Kin, in_il), None
        if out_packed:
            out_off, total = pack_offsets([n * K for n in out_len], order[::-1], GAPS[::-1])
            want, out_stride = pack_out(ref, K, B, out_il, out_len, out_off, total), 0
        else:
            out_off, out_stride = None, (P * K + SLACK if out_il else P + SLACK)
            want = F.lay_out(ref, K, P, B, out_il)
        xin, out = tier.buf(xb), tier.sentinels(want.size)
        a = tier.make(nclips * K, dither=dither, meters=meters)
        p = a.resample_clips_packed_ptr(0 if M is None else Kin, K, M, tier.ptr(xin), in_fmt, in_il, in_stride, in_off,
                                        in_len, tier.ptr(out), out_fmt, out_il, out_stride, out_off, out_len)
        assert p == P
        assert_same(tier.host(out), want, ("layout", in_il, out_il))
        if meters:
            m = a.read_meters()
            for name in ("peak", "clipped", "nonfinite"):
                assert np.array_equal(m[name], ref_m[name]), (name, in_il, out_il, m[name], ref_m[name])
    return ref, ref_m


def out_lens(tier, in_len):
    """natural lengths, but one clip cut short and one 3000 frames past its natural end (the filter's tail, then zeros)"""
    nat = tier.out_len(in_len)
    nat[in_len.index(4500)] -= 100
    nat[in_len.index(2000)] += 3000
    return nat


# ---------------------------------------------------------------- 1. both sides packed
FORMAT_PAIRS = [(f, F64) for f in (F64, F32, S16, S24, S32)] + [(F64, f) for f in (F32, S16, S24, S32)] + [(S16, F32)]
# (the integer output that is dithered and metered at each K)
DITHERED = {1: S16, 2: S24, 3: S32, 6: S16, 33: S24, 64: S32}


def hot(K):
    """the noise with something for the meters: the longest clip's first channel times 1.5, an Inf inside the last
    channel of the 4500-frame clip (fp64 input carries both)"""
    if ("hot", K) not in _SIGNAL:
        x = signal(NCLIPS * K).copy()
        x[5 * K] *= 1.5
        x[4 * K + K - 1, 700] = np.inf
        x.setflags(write=False)
        _SIGNAL["hot", K] = x
    return _SIGNAL["hot", K]


def check_both_packed(tier, K, fmts):
    finished = fmts[0] == F64 and fmts[1] == DITHERED[K]
    ref, m = check_packed(tier, K, None, hot(K) if finished else signal(NCLIPS * K), "hot" if finished else "noise",
                          fmts[0], LENGTHS, fmts[1], out_lens(tier, LENGTHS), ALL_LAYOUTS, dither=5 if finished else None,
                          meters=finished)
    # (the rows are no silence: the longest clip's bytes differ from the encoded zero's)
    assert np.count_nonzero(ref[5 * K, :5000 * BYTES[fmts[1]]]) > 1000
    if finished:
        assert m["clipped"][5 * K] > 100 and m["nonfinite"][4 * K + K - 1] > 0 and m["peak"][5 * K] > 1.0


def pair_id(f):
    return "%dto%d" % f


@pytest.mark.parametrize("fmts", FORMAT_PAIRS, ids=pair_id)
@pytest.mark.parametrize("K", KS)
def test_both_packed_emulated(emul, K, fmts):
    check_both_packed(Tier(emul), K, fmts)


@pytest.mark.gpu
@pytest.mark.parametrize("fmts", FORMAT_PAIRS, ids=pair_id)
@pytest.mark.parametrize("K", KS)
def test_both_packed_gpu(K, fmts):
    check_both_packed(Tier(None), K, fmts)


# ---------------------------------------------------------------- 2. mixed sides
def check_mixed_sides(tier, K):
    x, out_len = signal(NCLIPS * K), out_lens(tier, LENGTHS)
    check_packed(tier, K, None, x, "noise", S16, LENGTHS, F32, out_len, ALL_LAYOUTS, out_packed=False)
    check_packed(tier, K, None, x, "noise", S16, LENGTHS, F32, out_len, ALL_LAYOUTS, in_packed=False)


@pytest.mark.parametrize("K", [1, 3, 33])
def test_mixed_sides_emulated(emul, K):
    check_mixed_sides(Tier(emul), K)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3, 33])
def test_mixed_sides_gpu(K):
    check_mixed_sides(Tier(None), K)


# ---------------------------------------------------------------- 3. with a mix
def eighths(K, Kin):
    """+-j / 8, |j| <= 8: with inputs n / 32768 every product and partial sum is exact in fp64, whatever the order"""
    j = (np.arange(K * Kin) * 7 + 3) % 17 - 8
    return (j / 8.0).reshape(K, Kin)


MIXES = {"loader": ([[.5, .5]], S16, F32, [(True, False)]), "6to2": (eighths(2, 6), F32, S16, [(False, False), (False, True)])}


def check_mix(tier, name):
    M, in_fmt, out_fmt, layouts = MIXES[name]
    M = np.asarray(M, dtype=np.float64)
    out_len = out_lens(tier, LENGTHS)
    x = signal(NCLIPS * M.shape[1])
    check_packed(tier, M.shape[0], M, x, "noise", in_fmt, LENGTHS, out_fmt, out_len, layouts)
    if name == "loader":
        # (... and the loader's padded rows out of packed clips)
        check_packed(tier, 1, M, x, "noise", in_fmt, LENGTHS, out_fmt, out_len, layouts, out_packed=False)


@pytest.mark.parametrize("name", sorted(MIXES))
def test_mix_emulated(emul, name):
    check_mix(Tier(emul), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MIXES))
def test_mix_gpu(name):
    check_mix(Tier(None), name)


# ---------------------------------------------------------------- 4. aliased inputs
def check_aliased(tier, K):
    """all six clips read from ONE offset with their six lengths -- windows of one interleaved recording: the rows are
    those of six copies of it.  The zero-length clip's output offset lies inside a neighbour's region, of which nothing
    is lost"""
    one = signal(K)
    out_len = tier.out_len(LENGTHS)
    ref, _ = reference(tier, K, None, np.concatenate([one] * NCLIPS), "copies", S16, LENGTHS, F32, out_len)
    # five elements of garbage, the recording's 6001 frames, garbage: nothing else
    units = F.encode_units(one, S16, [max(LENGTHS)] * K)
    xb = np.concatenate([units[0, -5:], region(units, max(LENGTHS), True), units[0, -37:]]).reshape(-1)
    out_off, total = pack_offsets([n * K for n in out_len])
    out_off[LENGTHS.index(0)] = out_off[5] + 11
    want = pack_out(ref, K, 4, False, out_len, out_off, total)
    xin, out = tier.buf(xb), tier.sentinels(want.size)
    a = tier.make(NCLIPS * K)
    assert a.resample_clips_packed_ptr(0, K, None, tier.ptr(xin), S16, True, 0, [5] * NCLIPS, LENGTHS, tier.ptr(out), F32,
                                       False, 0, out_off, out_len) == max(out_len)
    assert_same(tier.host(out), want, "aliased")


@pytest.mark.parametrize("K", [1, 2])
def test_aliased_inputs_emulated(emul, K):
    check_aliased(Tier(emul), K)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 2])
def test_aliased_inputs_gpu(K):
    check_aliased(Tier(None), K)


# ---------------------------------------------------------------- 5. refusals
def check_refusals(tier):
    K = 2
    x, in_len = signal(NCLIPS * K), LENGTHS
    out_len = tier.out_len(in_len)
    P, max_in = max(out_len), max(in_len)
    ref, _ = reference(tier, K, None, x, "noise", F64, in_len, F64, out_len)
    units = F.encode_units(x, F64, F.rows_of(in_len, K))
    xb, in_off = pack_in(units, K, True, in_len)
    out_off, total = pack_offsets([n * K for n in out_len])
    want = pack_out(ref, K, 8, True, out_len, out_off, total)
    xs, in_stride = F.lay_in(units, K, True)
    xin, xstr, out = tier.buf(xb), tier.buf(xs), tier.sentinels(want.size)
    a = tier.make(NCLIPS * K)
    err = a._lib.r8b_last_error

    def call(kin=0, mix=None, i_off=in_off, o_off=out_off, src=xin, i_stride=0, o_stride=0, obj=a):
        return tier.raw_packed(obj, kin, K, mix, src, F64, True, i_stride, i_off, in_len, out, F64, True, o_stride, o_off,
                               out_len)

    def refused(word, **kw):
        assert call(**kw) == -1, kw
        assert word in err(), (kw, err())
        assert np.all(tier.host(out) == SENTINEL), kw

    refused(b"in_offset", i_off=in_off[:2] + [-1] + in_off[3:])
    refused(b"out_offset", o_off=out_off[:4] + [-8] + out_off[5:])
    # (a zero-length clip's offset is looked at as far as its sign)
    refused(b"in_offset", i_off=[-1 if n == 0 else o for o, n in zip(in_off, in_len)])
    # overlapping by one element, and identical regions (clips 3 and 5, both non-empty)
    refused(b"out_offset", o_off=out_off[:3] + [out_off[5] + out_len[5] * K - 1] + out_off[4:])
    refused(b"out_offset", o_off=out_off[:3] + [out_off[5]] + out_off[4:])
    for bad in (1, 3, -1, 65):
        refused(b"in_channels", kin=bad)
    refused(b"in_channels", kin=65, mix=[0.5] * (65 * K))
    # a strided side still answers for its stride
    refused(b"in_stride", i_off=None, src=xstr, i_stride=max_in * K - 1)
    refused(b"out_stride", o_off=None, o_stride=P * K - 1)
    # an object in mid-stream
    b = tier.make(NCLIPS * K)
    blk, res = tier.buf(np.zeros((NCLIPS * K, CHUNK))), tier.buf(np.zeros((NCLIPS * K, max(b.max_out_len, 1))))
    tier.sync()
    b.process_ptr(tier.ptr(blk), CHUNK, CHUNK, tier.ptr(res), max(b.max_out_len, 1))
    refused(b"processed samples", obj=b)
    # ... none of which used the object up or changed it (in_channels == clip_channels without a matrix is no mix)
    assert call(kin=K) == P
    assert_same(tier.host(out), want, "after the refusals")


def test_refusals_emulated(emul):
    check_refusals(Tier(emul))


@pytest.mark.gpu
def test_refusals_gpu():
    check_refusals(Tier(None))


# ---------------------------------------------------------------- 6. slots: back to back on one stream
def check_back_to_back(tier, stream=0, wait=lambda: None):
    """five calls on one object and one stream, nothing waits in between: more calls than the object has slots, each
    with its own offsets and lengths, two of them with a mix -- every call's kernels read ITS bases"""
    Mx = np.array([[.5, .5]])
    rot = lambda v, r: v[r:] + v[:r]
    calls = []
    for j, M in enumerate([None, Mx, None, None, Mx]):
        Kin = 1 if M is None else 2
        in_len = rot(LENGTHS, j)
        out_len = [n + 7 * j for n in tier.out_len(in_len)]
        x = signal(NCLIPS * Kin)
        ref, _ = reference(tier, 1, M, x, "noise", S16, in_len, F64, out_len)
        order = rot(ORDER, j)
        xb, in_off = pack_in(F.encode_units(x, S16, F.rows_of(in_len, Kin)), Kin, True, in_len, order, rot(GAPS, j % 3))
        out_off, total = pack_offsets(out_len, order[::-1], rot(GAPS, (j + 1) % 3))
        want = pack_out(ref, 1, 8, False, out_len, out_off, total)
        calls.append((M, Kin, tier.buf(xb), in_off, in_len, tier.sentinels(want.size), out_off, out_len, want))
    tier.sync()
    a = tier.make(NCLIPS)
    for M, Kin, xin, in_off, in_len, out, out_off, out_len, _ in calls:
        assert a.resample_clips_packed_ptr(0 if M is None else Kin, 1, M, tier.ptr(xin), S16, True, 0, in_off, in_len,
                                           tier.ptr(out), F64, False, 0, out_off, out_len, stream) == max(out_len)
    wait()
    for j, call in enumerate(calls):
        assert_same(tier.host(call[5]), call[8], ("call", j))


def test_back_to_back_emulated(emul):
    check_back_to_back(Tier(emul))


@pytest.mark.gpu
def test_back_to_back_on_one_stream_gpu():
    import torch
    s = torch.cuda.Stream()
    check_back_to_back(Tier(None), s.cuda_stream, s.synchronize)


# ---------------------------------------------------------------- 7. both offset arrays NULL
def check_no_offsets(tier):
    """the call without offsets IS _ex / _mix: the whole strided buffer, padding zeros and slack included"""
    out_len = out_lens(tier, LENGTHS)
    check_packed(tier, 2, None, signal(NCLIPS * 2), "noise", S16, LENGTHS, F32, out_len, ALL_LAYOUTS, in_packed=False,
                 out_packed=False)
    M = np.asarray(MIXES["loader"][0])
    check_packed(tier, 1, M, signal(NCLIPS * 2), "noise", S16, LENGTHS, F32, out_len, [(True, False), (False, False)],
                 in_packed=False, out_packed=False)


def test_no_offsets_emulated(emul):
    check_no_offsets(Tier(emul))


@pytest.mark.gpu
def test_no_offsets_gpu():
    check_no_offsets(Tier(None))


# ---------------------------------------------------------------- 8. r8b_clip_pack_offsets (host only, product library)
def pack(lib, lens, channels, align, n=None):
    n = len(lens) if n is None else n
    ll = C.c_longlong * max(len(lens), 1)
    off = ll(*([-7] * max(len(lens), 1)))
    total = lib.r8b_clip_pack_offsets(n, ll(*lens), channels, align, off)
    return [off[i] for i in range(len(lens))], total


def test_pack_offsets():
    lib = r8b.load()
    assert pack(lib, LENGTHS, 1, 1) == ([0, 0, 1, 2000, 4000, 8500], 14501)
    assert pack(lib, LENGTHS, 2, 1) == ([0, 0, 2, 4000, 8000, 17000], 29002)
    # every base a multiple of 16, the total the end of the last clip (not rounded)
    assert pack(lib, LENGTHS, 1, 16) == ([0, 0, 16, 2016, 4016, 8528], 14529)
    assert pack(lib, [5, 3], 3, 16) == ([0, 16], 25)
    # a zero-length clip in the middle has its neighbour's base
    assert pack(lib, [10, 0, 7], 1, 1) == ([0, 10, 10], 17)
    assert pack(lib, [10, 0, 7], 1, 16) == ([0, 16, 16], 23)
    assert pack(lib, [], 1, 1) == ([], 0)
    # the refusals touch nothing
    for lens, channels, align, n in (([1, 2], 1, 1, -1), ([1, -2], 1, 1, None), ([1, 2], 0, 1, None), ([1, 2], 1, 0, None)):
        assert pack(lib, lens, channels, align, n) == ([-7] * len(lens), -1), (lens, channels, align, n)


# ---------------------------------------------------------------- 9. bases past 2^32 bytes
@pytest.mark.gpu
@pytest.mark.parametrize("out_il", [True, False])
def test_base_past_4gib_gpu(out_il):
    """one stereo S16 clip of 1999 frames written packed just past byte 2^32 of an uninitialised buffer that ends soon
    after it: the region is right, and the 64 bytes on either side of it, pre-set, are untouched"""
    import torch
    tier = Tier(None)
    K, n = 2, 1999
    x = signal(K)
    out_len = tier.out_len([n])
    ref, _ = reference(tier, K, None, x, "noise", S16, [n], S16, out_len)
    size = out_len[0] * K * 2                    # the region's bytes
    base = (1 << 31) + 9                         # elements: byte 2^32 + 18
    big = torch.empty(base * 2 + size + 64, dtype=torch.uint8, device="cuda")
    big[base * 2 - 64:base * 2] = SENTINEL
    big[base * 2 + size:] = SENTINEL
    xb, in_off = pack_in(F.encode_units(x, S16, [n] * K), K, True, [n], [0])
    xin = tier.buf(xb)
    tier.sync()
    a = tier.make(K)
    assert a.resample_clips_packed_ptr(0, K, None, tier.ptr(xin), S16, True, 0, in_off, [n], big.data_ptr(), S16, out_il, 0,
                                       [base], out_len) == out_len[0]
    torch.cuda.synchronize()
    got = big[base * 2 - 64:].cpu().numpy()
    want = np.full(64 + size + 64, SENTINEL, dtype=np.uint8)
    want[64:64 + size] = pack_out(ref, K, 2, out_il, out_len, [0], out_len[0] * K)
    assert_same(got, want, ("past 4 GiB", out_il))


# ---------------------------------------------------------------- 10. the Python entry
@pytest.mark.gpu
def test_resample_clips_packed_tensors_gpu():
    import torch
    tier = Tier(None)
    K = 2
    x = signal(NCLIPS * K)
    in_len = LENGTHS
    out_len = tier.out_len(in_len)
    P = max(out_len)
    rows = np.ascontiguousarray(F.encode_units(x, S16, F.rows_of(in_len, K))).view(np.int16).reshape(NCLIPS * K, T)
    a = tier.make(NCLIPS * K)
    # what resample_clips makes of the padded interleaved clips
    xt = torch.from_numpy(np.ascontiguousarray(rows.reshape(NCLIPS, K, T).transpose(0, 2, 1))).cuda()
    padded, ol = a.resample_clips(xt, in_len, out_format=F32, clip_channels=K, interleaved=True)
    assert ol == out_len
    torch.cuda.synchronize()
    padded = padded.cpu().numpy().view(np.uint32)                                   # [nclips, P, K]
    # the same clips end to end, default offsets on both sides
    packed = torch.from_numpy(np.concatenate([rows[i * K:(i + 1) * K, :n].T.reshape(-1) for i, n in enumerate(in_len)])).cuda()
    out, off, ol = a.resample_clips_packed(packed, in_len, out_format=F32, clip_channels=K, interleaved=True)
    assert ol == out_len and off == [int(v) for v in np.cumsum([0] + [n * K for n in out_len[:-1]])]
    assert out.dtype == torch.float32 and tuple(out.shape) == (sum(out_len) * K,)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    for i, n in enumerate(out_len):
        assert np.array_equal(got[off[i]:off[i] + n * K], padded[i, :n].reshape(-1)), i
    # given offsets and a given buffer, planar regions
    in_off, total = pack_offsets([n * K for n in in_len])
    src = np.full(total, 32767, dtype=np.int16)
    for i, n in enumerate(in_len):
        src[in_off[i]:in_off[i] + n * K] = rows[i * K:(i + 1) * K, :n].reshape(-1)
    out_off, total = pack_offsets([n * K for n in out_len], ORDER[::-1])
    buf = torch.full((total,), -7.0, dtype=torch.float32, device="cuda")
    res, off, _ = a.resample_clips_packed(torch.from_numpy(src).cuda(), in_len, offsets=in_off, out_offsets=out_off,
                                          out_format=F32, out=buf, clip_channels=K)
    assert res.data_ptr() == buf.data_ptr() and off == out_off
    torch.cuda.synchronize()
    got = res.cpu().numpy()
    want = np.full(total, -7.0, dtype=np.float32)
    for i, n in enumerate(out_len):
        want[out_off[i]:out_off[i] + n * K] = padded[i, :n].T.reshape(-1).view(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # out_packed=False: what resample_clips returns
    res, ol = a.resample_clips_packed(packed, in_len, out_format=F32, clip_channels=K, interleaved=True, out_packed=False)
    assert ol == out_len and tuple(res.shape) == (NCLIPS, P, K)
    torch.cuda.synchronize()
    assert np.array_equal(res.cpu().numpy().view(np.uint32), padded)
