"""The true-peak meter of the PCM egress (include/r8bsrc.h "true peak"; csrc/r8b_truepeak.h): oracle and checks shared by the
emulated and the GPU tier of tests/test_true_peak.py.

The oracle needs no resampler: every check takes its call's output as F64, so x is known exactly, and evaluates the
specified chain -- one multiplication, then eleven correctly rounded fused multiply-adds per phase -- in exact rational
arithmetic from tests/golden/true_peak_taps.json.  To stay quick it first computes every y in plain fp64 (error below
1e-14 of the largest sample in reach) and evaluates exactly only the y within 1e-12 of the largest: the exact maximum is
among them.  Equality with the meter is BITWISE everywhere."""
import importlib
import json
import os
import re
from fractions import Fraction

import numpy as np

import pcm8_cases as M

r8b = importlib.import_module("r8brain-free-src_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, S16 = r8b.PCM_F64, r8b.PCM_S16
_GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "true_peak_taps.json")))
G = [[float.fromhex(v) for v in row] for row in _GOLD["g"]]
TAPS, DELAY = _GOLD["taps"], _GOLD["delay"]
HIST = TAPS - 1
assert (len(G), TAPS, DELAY) == (3, 12, 6) and all(len(row) == TAPS for row in G)
# the kernel's tile, frames of a workgroup
TF = int(re.search(r"kTpTile = (\d+);", open(os.path.join(ROOT, "r8brain-free-src_amd", "csrc", "r8b_truepeak.h")).read()).group(1))
CUTS = [1, 5, 11, 12, 13, TF - 1, TF, TF + 1, 2 * TF + 3]
ATT = 136.45


class Tier(M.Tier):
    def f64(self, b):
        return self.host(b).view(np.float64)


# ---------------------------------------------------------------- the oracle
_EXACT = {}


def exact_chain(p, w):
    """y[4 j + p] for the window w[t] = x[j - t] of finite doubles"""
    k = (p, w.tobytes())
    if k not in _EXACT:
        g = G[p - 1]
        acc = g[0] * float(w[0])
        for t in range(1, TAPS):
            acc = float(Fraction(g[t]) * Fraction(float(w[t])) + Fraction(acc))
        _EXACT[k] = acc
    return _EXACT[k]


def oracle(x, hist=None, skip=0, tail=False, where=False):
    """max |y| over frames [skip, len(x) (+ 11 with tail)) of the frames x behind the 11 frames hist (None: zeros), NaN
    skipped; with where: (value, [(frame, phase) of every y that attains it])"""
    x = np.asarray(x, dtype=np.float64)
    z = np.concatenate([np.zeros(HIST) if hist is None else np.asarray(hist, dtype=np.float64), x,
                        np.zeros(HIST if tail else 0)])
    nf = len(z) - HIST
    best, at = 0.0, []

    def note(v, j, p):
        nonlocal best, at
        v = abs(v)
        if v > best:
            best, at = v, [(j, p)]
        elif v == best and v > 0:
            at.append((j, p))

    if nf > skip:
        W = np.lib.stride_tricks.sliding_window_view(z, TAPS)[skip:, ::-1]  # W[j - skip, t] = x[j - t]
        fin = np.isfinite(W).all(axis=1)
        p0 = np.abs(W[:, DELAY])
        ok0 = ~np.isnan(p0)
        top0 = p0[ok0].max() if ok0.any() else 0.0
        for j in np.nonzero(ok0 & (p0 == top0))[0]:
            note(p0[j], skip + int(j), 0)
        rows = np.nonzero(fin)[0]
        if len(rows):
            approx = np.abs(W[rows] @ np.array(G).T)
            floor = max(approx.max(), top0 if np.isfinite(top0) else 0.0) - 1e-12 * np.abs(W[rows]).max()
            if np.isfinite(top0):
                for i, p in zip(*np.nonzero(approx >= floor)):
                    note(exact_chain(int(p) + 1, W[rows[i]]), skip + int(rows[i]), int(p) + 1)
        # a window that holds Inf or NaN: every partial sum behind the first such term is Inf or NaN, whatever the rounding
        for j in np.nonzero(~fin)[0]:
            for p in (1, 2, 3):
                acc = G[p - 1][0] * float(W[j, 0])
                for t in range(1, TAPS):
                    acc = G[p - 1][t] * float(W[j, t]) + acc
                assert not np.isfinite(acc)
                if not np.isnan(acc):
                    note(acc, skip + int(j), p)
    return (best, at) if where else best


class Expect:
    """what a stream's meter reads call after call: feed() the output rows [nch, n] of every call"""

    def __init__(self, nch, skip=0):
        self.val = np.zeros(nch)
        self.hist = [np.zeros(HIST) for _ in range(nch)]
        self.skip = skip

    def feed(self, rows):
        n = rows.shape[1]
        s = min(self.skip, n)
        for c in range(len(self.val)):
            self.val[c] = max(self.val[c], oracle(rows[c], self.hist[c], skip=s))
            self.hist[c] = np.concatenate([self.hist[c], rows[c]])[-HIST:]
        self.skip -= s
        return self.val.copy()


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    assert len(bad) == 0, "%s: channel %d reads %r (%s), the oracle says %r (%s); %d channels differ" % (
        what, bad[0], got[bad[0]], got[bad[0]].hex(), want[bad[0]], want[bad[0]].hex(), len(bad))


# ---------------------------------------------------------------- streams
def noise(nch, n, seed):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, size=(nch, n))


def call(tier, a, x, out_il=False, out_fmt=F64):
    """one r8b_batch_process_pcm call, planar F64 in: the output rows [nch, n] (F64) or the output's bytes"""
    nch, l = x.shape
    cap = max(a.max_out_len, 1)
    xin = tier.buf(np.ascontiguousarray(x))
    B = M.BYTES[out_fmt]
    out = tier.buf(np.zeros(nch * cap * B, dtype=np.uint8))
    tier.sync()
    n = a.process_pcm_ptr(tier.ptr(xin), F64, False, l, l, tier.ptr(out), out_fmt, out_il, nch if out_il else cap)
    raw = tier.host(out)
    if out_fmt != F64:
        return np.array(raw[:nch * n * B] if out_il else raw.reshape(nch, cap * B)[:, :n * B])
    y = raw.view(np.float64)
    return np.array(y.reshape(cap, nch)[:n].T if out_il else y.reshape(nch, cap)[:, :n])


def stream(tier, a, x, cuts, out_il=False):
    """the stream x [nch, N] cut at `cuts` (the rest in one more call): [(output rows, meter read after the call)]"""
    res, pos = [], 0
    for l in list(cuts) + [x.shape[1] - sum(cuts)]:
        if l > 0:
            rows = call(tier, a, x[:, pos:pos + l], out_il)
            res.append((rows, a.read_true_peak()))
            pos += l
    return res


def metered(tier, nch, src, dst, chunk):
    a = tier.make(nch, src, dst, chunk, att=ATT)
    a.enable_true_peak()
    return a


def check_stream(tier, a, x, cuts, what, out_il=False, skip=0):
    want = Expect(x.shape[0], skip)
    for k, (rows, got) in enumerate(stream(tier, a, x, cuts, out_il)):
        same_bits(got, want.feed(rows), "%s, after call %d (%d frames)" % (what, k, rows.shape[1]))
    return want.val


# 1. the specification, and 2. chunk invariance
def check_spec_pass(tier):
    """Src == Dst, 3 channels, noise; calls of every length in CUTS, read after each; then the same stream in one call"""
    N = sum(CUTS)
    x = noise(3, N, 901)
    a = metered(tier, 3, 44100.0, 44100.0, max(CUTS))
    cut = check_stream(tier, a, x, CUTS[:-1], "Src == Dst, cut")
    for il in (False, True):
        b = metered(tier, 3, 44100.0, 44100.0, N)
        whole = check_stream(tier, b, x, [], "Src == Dst, one call", out_il=il)
        same_bits(whole, cut, "one call against the cut stream")
    # the cuts in the opposite order: the long calls first
    a.clear()
    same_bits(check_stream(tier, a, x, CUTS[::-1][:-1], "Src == Dst, cut backwards"), cut, "cut backwards")


def check_spec_chain(tier):
    """44100 -> 88200, 3 channels (a pair and a solo), calls that span more than two tiles; planar and interleaved"""
    L = TF + TF // 16
    x = noise(3, 3 * L, 902)
    vals = []
    for il in (False, True):
        a = metered(tier, 3, 44100.0, 88200.0, L)
        assert a.max_out_len > 2 * TF
        vals.append(check_stream(tier, a, x, [L, L], "44100 -> 88200", out_il=il))
    same_bits(vals[0], vals[1], "interleaved against planar")
    b = metered(tier, 3, 44100.0, 88200.0, L)
    same_bits(check_stream(tier, b, x, [1, 5, 11, 12, 13, 700, L, 300, L - 1], "44100 -> 88200, cut"), vals[0], "cut against whole calls")


def burst(n, j, p, amp=0.75):
    """frames whose 4x interpolation peaks in phase p of frame j: an fs/4 tone centred at j - 6 + p / 4 under a taper"""
    d = np.arange(n) - (j - DELAY + p / 4.0)
    return amp * np.cos(np.pi / 2 * d) * np.where(np.abs(d) < 16, 1.0 - (d / 16.0) ** 2, 0.0)


def check_phases(tier):
    """the maximum in phase 1, 2, 3 in turn, at a tile's first lane, a tile's last lane and among a call's first 11
    frames (its window is the history); and the fs/4 pattern +a +a -a -a, whose peak lies in phase 2"""
    first = 2 * TF + 3
    N = first + 100
    a = metered(tier, 4, 44100.0, 44100.0, first)
    for p in (1, 2, 3):
        where = [TF, 2 * TF - 1, first + 3]
        x = np.stack([burst(N, j, p) for j in where] + [np.tile([0.5, 0.5, -0.5, -0.5], N // 4 + 1)[:N]])
        for c, j in enumerate(where):
            assert oracle(x[c], where=True)[1] == [(j, p)], (p, j, oracle(x[c], where=True))
        v, at = oracle(x[3], where=True)
        assert v > 0.7 and {q for _, q in at} == {2}
        a.clear()
        check_stream(tier, a, x, [first], "phase %d" % p)


# 3. the lone sample
def check_lone_sample(tier):
    """one non-zero sample per channel, at every frame of a tile and across its edge: whichever lane and wave meters it,
    the value is its magnitude (phase 0; every tap is smaller than 1)"""
    pos = list(range(TF + 16))
    n = TF + 32
    x = np.zeros((len(pos), n))
    want = np.array([(1.0 + c / 4096.0) * (-1) ** c for c in range(len(pos))])
    x[np.arange(len(pos)), pos] = want
    a = metered(tier, len(pos), 44100.0, 44100.0, n)
    assert np.array_equal(call(tier, a, x), x)
    same_bits(a.read_true_peak(), np.abs(want), "lone sample")
    # ... and in two calls cut inside the tile: the sample is in the history when phase 0 reaches it
    a.clear()
    call(tier, a, x[:, :TF - 3])
    call(tier, a, x[:, TF - 3:])
    same_bits(a.read_true_peak(), np.abs(want), "lone sample, cut at TF - 3")


# 4. non-finite samples
def check_nonfinite(tier):
    n = 300
    x = noise(5, n, 904)
    x[0, 100] = np.nan
    x[1, 100] = np.inf
    x[2, 100], x[2, 107] = np.inf, -np.inf
    x[3, 100] = -np.inf
    x[4, 280:] = np.nan     # (the finite y in front still count)
    a = metered(tier, 5, 44100.0, 44100.0, n)
    got = check_stream(tier, a, x, [150], "non-finite")
    assert np.isfinite(got[0]) and got[0] > 0 and np.isfinite(got[4]) and got[4] > 0
    assert got[1] == np.inf and got[2] == np.inf and got[3] == np.inf


# ---------------------------------------------------------------- 5. clips
def _lay(rows, lens, K, il, packed, pad):
    """[nclips K, T] -> (the buffer's doubles, stride, offsets or None): strided rows / frame-major clips of T frames,
    or packed regions at the clips' own lengths, 3 doubles of `pad` between them"""
    nclips, T = len(lens), rows.shape[1]
    if not packed:
        if not il:
            return rows.reshape(-1).copy(), T, None
        return rows.reshape(nclips, K, T).transpose(0, 2, 1).reshape(-1).copy(), T * K, None
    parts, off, at = [], [], 0
    for i, n in enumerate(lens):
        r = rows[i * K:(i + 1) * K, :n]
        parts += [(r.T if il else r).reshape(-1), np.full(3, pad)]
        off.append(at)
        at += n * K + 3
    return np.concatenate(parts), 0, off


def _unlay(y, lens, K, il, stride, off):
    """the output buffer's doubles -> one array per object channel, in the caller's order"""
    out = []
    for i, n in enumerate(lens):
        for k in range(K):
            if off is not None:
                reg = y[off[i]:off[i] + n * K]
                out.append(reg.reshape(n, K)[:, k].copy() if il else reg[k * n:(k + 1) * n].copy())
            elif il:
                out.append(y[i * stride:i * stride + n * K].reshape(n, K)[:, k].copy())
            else:
                out.append(y[(i * K + k) * stride:(i * K + k) * stride + n].copy())
    return out


def clip_call(tier, a, entry, K, rows, in_len, out_len, in_il=False, out_il=False, packed=False, flags=0):
    """one call of a clip entry on F64 buffers: the outputs per object channel (out_len frames each)"""
    nclips, P = len(in_len), max(out_len)
    xb, in_stride, in_off = _lay(rows, in_len, K, in_il, packed, 9e9)
    if packed:
        out_off, n_out = [], 0
        for n in out_len:
            out_off.append(n_out)
            n_out += n * K + 3
        out_stride = 0
    else:
        out_off, out_stride = None, (P * K if out_il else P) + 5
        n_out = out_stride * (nclips if out_il else nclips * K)
    xin, out = tier.buf(xb), tier.buf(np.full(max(n_out, 1), 7e7))
    tier.sync()
    pi, po = tier.ptr(xin), tier.ptr(out)
    if entry == "clips":
        assert K == 1 and not packed
        p = a.resample_clips_ptr(pi, F64, in_stride, in_len, po, F64, out_stride, out_len)
    elif entry == "ex":
        p = a.resample_clips_ex_ptr(K, pi, F64, in_il, in_stride, in_len, po, F64, out_il, out_stride, out_len)
    elif entry == "mix":
        p = a.resample_clips_mix_ptr(K, K, np.eye(K), pi, F64, in_il, in_stride, in_len, po, F64, out_il, out_stride, out_len)
    elif entry == "packed":
        p = a.resample_clips_packed_ptr(0, K, None, pi, F64, in_il, in_stride, in_off, in_len, po, F64, out_il, out_stride,
                                        out_off, out_len)
    else:
        p = a.resample_clips_sched_ptr(0, K, None, pi, F64, in_il, in_stride, in_off, in_len, po, F64, out_il, out_stride,
                                       out_off, out_len, flags)
    assert p == P
    return _unlay(tier.f64(out), out_len, K, out_il, out_stride, out_off)


def check_clip_call(tier, a, what, *args, **kw):
    """a call on a zeroed meter: every channel's value is the oracle's over its output and the 11 frames of its tail"""
    a.read_true_peak(reset=True)
    outs = clip_call(tier, a, *args, **kw)
    want = np.array([oracle(y, tail=True) for y in outs])
    got = a.read_true_peak()
    same_bits(got, want, what)
    return outs, got


CLIP_LENS = [0, 1, 10, 11, 12, 100, 101, 137]   # MaxInLen 50: ends at a step's last output, in a step's first frame
CLIP_FORMS = [("clips", 1, False, False, False), ("ex", 1, False, False, False), ("ex", 2, True, True, False),
              ("ex", 2, True, False, False), ("mix", 2, False, True, False), ("mix", 1, False, False, False),
              ("packed", 1, False, False, True), ("packed", 2, True, True, True), ("packed", 2, False, False, True),
              ("sched", 1, False, False, True), ("sched", 2, True, True, False)]


def check_clips_pass(tier):
    """Src == Dst: the five entries, strided and packed, interleaved and planar, on the lengths of CLIP_LENS; a clip cut
    short and one that runs on into zeros; true_peak >= peak; the next call starts from zero history"""
    T = max(CLIP_LENS) + 3
    objs = {}
    for entry, K, in_il, out_il, packed in CLIP_FORMS:
        nch = len(CLIP_LENS)
        if nch not in objs:
            objs[nch] = metered(tier, nch, 44100.0, 44100.0, 50)
            objs[nch].enable_meters()
        a = objs[nch]
        lens = CLIP_LENS if K == 1 else [12, 100, 101, 1]
        out_len = list(lens)
        out_len[-1], out_len[-2] = lens[-1] - 1 if lens[-1] > 1 else 1, lens[-2] + 20    # (cut short; run on into zeros)
        rows = noise(nch, T, 905)
        for c in range(nch):
            rows[c, max(out_len[c // K] - 1, 0)] = 3.0 + c    # the clip's last frame is its largest: only the tail shows it
        what = "%s K=%d in %s out %s %s" % (entry, K, "il" if in_il else "planar", "il" if out_il else "planar",
                                           "packed" if packed else "strided")
        flags = r8b.CLIPS_DROP_FINISHED | r8b.CLIPS_LONGEST_FIRST if entry == "sched" else 0
        a.read_meters(reset=True)
        outs, got = check_clip_call(tier, a, what, entry, K, rows, lens, out_len, in_il, out_il, packed, flags)
        peak = a.read_meters()["peak"]
        assert np.all(got.view(np.uint64) >= peak.view(np.uint64)), (what, got, peak)
        for c, y in enumerate(outs):
            assert len(y) == 0 or got[c] == 3.0 + c or out_len[c // K] > lens[c // K], (what, c, got[c])
        # the same object again, quiet clips behind the loud ends: nothing of the first call is left in the history
        check_clip_call(tier, a, what + ", second call", entry, K, rows * 1e-3, lens, out_len, in_il, out_il, packed, flags)


def check_clips_tile_edge(tier):
    """clips that end at a tile's last frames: the tail runs past the tile, in the workgroup that holds the last frame"""
    lens = [TF, TF + 1, TF - 1, TF - 8, TF + 11, 2 * TF]
    a = metered(tier, len(lens), 44100.0, 44100.0, 2 * TF + 5)
    rows = noise(len(lens), 2 * TF + 5, 906)
    for c, n in enumerate(lens):
        rows[c, n - 1] = 2.0 + c
    outs, got = check_clip_call(tier, a, "tile edge", "clips", 1, rows, lens, lens)
    assert np.array_equal(got, 2.0 + np.arange(len(lens)))
    b = metered(tier, len(lens), 44100.0, 44100.0, TF // 2 + 1)
    check_clip_call(tier, b, "tile edge, short steps", "clips", 1, rows, lens, lens)
    same_bits(b.read_true_peak(), got, "short steps against one step")


def check_clips_chain(tier):
    """44100 -> 88200, six clips of unequal length: plain, and DROP_FINISHED | LONGEST_FIRST -- values in the caller's order"""
    in_len = [300, 0, 700, 128, 701, 5]
    a = metered(tier, 6, 44100.0, 88200.0, 256)
    a.enable_meters()
    out_len = [a.clip_out_len(44100.0, 88200.0, n) for n in in_len]
    rows = noise(6, 704, 907)
    _, plain = check_clip_call(tier, a, "chain, flags 0", "sched", 1, rows, in_len, out_len, packed=True)
    flags = r8b.CLIPS_DROP_FINISHED | r8b.CLIPS_LONGEST_FIRST
    a.read_meters(reset=True)
    _, sched = check_clip_call(tier, a, "chain, drop | longest first", "sched", 1, rows, in_len, out_len, packed=True, flags=flags)
    assert plain[1] == 0.0 and np.all(plain[[0, 2, 3, 4, 5]] > 0)
    assert np.all(sched.view(np.uint64) >= a.read_meters()["peak"].view(np.uint64))
    # (longest first pairs other channels in the pair kernels: the outputs agree to rounding only, and so do the values)
    assert sched[1] == 0.0 and np.allclose(sched, plain, rtol=1e-12, atol=0)
    check_clip_call(tier, a, "chain, K = 2 interleaved, drop | longest first", "sched", 2, rows, in_len[::2], out_len[::2],
                            True, True, False, flags)


# ---------------------------------------------------------------- 6. lifecycle
C = 2000    # frames per call of the 44100 -> 88200 streams below: the first call already has outputs


def check_lifecycle(tier):
    a = tier.make(3, 44100.0, 88200.0, C, att=ATT)
    try:
        a.read_true_peak()
        raise AssertionError("read before enable went through")
    except RuntimeError as e:
        assert "never enabled" in str(e)
    assert a._lib.r8b_batch_true_peak_read(a._h, None, 0, None) == -1
    a.enable_true_peak()
    assert np.array_equal(a.read_true_peak(), np.zeros(3))
    x = noise(3, 4 * C, 908)
    want = Expect(3)
    v1 = want.feed(call(tier, a, x[:, :C]))
    v1 = want.feed(call(tier, a, x[:, C:2 * C]))
    assert np.all(v1 > 0)
    same_bits(a.read_true_peak(reset=True), v1, "before reset")
    assert np.array_equal(a.read_true_peak(), np.zeros(3))
    # reset zeroes the value only: the history goes on
    want.val[:] = 0
    v2 = want.feed(call(tier, a, x[:, 2 * C:3 * C]))
    same_bits(a.read_true_peak(), v2, "after reset")
    # disabled: kept, and not moved; re-enabled in mid-stream: the next 11 frames refill the history
    a.enable_true_peak(False)
    call(tier, a, 4.0 * x[:, 3 * C:])
    same_bits(a.read_true_peak(), v2, "while disabled")
    a.enable_true_peak()
    same_bits(a.read_true_peak(), v2, "re-enabled")
    blob = a.state_dict()
    tail = noise(3, 2 * C, 909)
    rows = [call(tier, a, tail[:, :C]), call(tier, a, tail[:, C:])]
    after = Expect(3, skip=HIST)
    after.val[:] = v2
    after.feed(rows[0])
    same_bits(a.read_true_peak(), after.feed(rows[1]), "re-enabled in mid-stream")
    # state_load: the same frames on another object, unmetered while the history refills
    b = metered(tier, 3, 44100.0, 88200.0, C)
    b.load_state_dict(blob)
    loaded = Expect(3, skip=HIST)
    for k in range(2):
        got = call(tier, b, tail[:, C * k:C * k + C])
        assert np.array_equal(got, rows[k])
        same_bits(b.read_true_peak(), loaded.feed(got), "after state_load, call %d" % k)
    # clear(): value and history
    b.clear()
    assert np.array_equal(b.read_true_peak(), np.zeros(3))
    check_stream(tier, b, x, [C, C, C], "after clear()")


def check_shards(tier):
    x = noise(4, 2 * C, 910)
    whole = metered(tier, 4, 44100.0, 88200.0, C)
    parts = [metered(tier, 2, 44100.0, 88200.0, C) for _ in range(2)]
    for k in range(2):
        call(tier, whole, x[:, C * k:C * k + C])
        for s in range(2):
            call(tier, parts[s], x[2 * s:2 * s + 2, C * k:C * k + C])
    got = whole.read_true_peak()
    assert np.all(got > 0)
    same_bits(np.concatenate([p.read_true_peak() for p in parts]), got, "shards against the whole")


# ---------------------------------------------------------------- 7. nothing else moves
def check_inert(tier):
    """a chain whose last stage is fed through the staging rows anyway (44100 -> 88200) and one whose last stage encodes a
    planar side itself (44100 -> 176400); meters, dither, neither"""
    x = noise(3, 3 * C, 911)
    for dst in (88200.0, 176400.0):
        for meters, dither in ((True, None), (False, None), (True, 5), (False, 5)):
            res = {}
            for mode in ("never", "on", "off again"):
                a = tier.make(3, 44100.0, dst, C, dither=dither, meters=meters, att=ATT)
                a.set_option("timing", 1)
                if mode != "never":
                    a.enable_true_peak()
                if mode == "off again":
                    a.enable_true_peak(False)
                out = [(call(tier, a, x[:, C * k:C * k + C], il, S16).tobytes(), a.boundary_symbols())
                       for k, il in enumerate((False, True, False))]
                res[mode] = (out, a.read_meters() if meters else None, a.stat("pcm_staged_sides"))
                if mode == "on":
                    assert np.all(a.read_true_peak() > 0)
            what = "-> %g, meters %s, dither %s" % (dst, meters, dither)
            never, on, off = res["never"], res["on"], res["off again"]
            assert off[0] == never[0] and off[2] == never[2], what + ": switched off again, something differs"
            assert [b for b, _ in on[0]] == [b for b, _ in never[0]], what + ": the output bytes moved"
            for k in ("peak", "clipped", "nonfinite") if meters else ():
                assert np.array_equal(on[1][k], never[1][k]) and np.array_equal(off[1][k], never[1][k]), (what, k)
            if meters or dither is not None or never[2] != 0:
                # the output side is staged already: same kernels, same count
                assert on[0] == never[0] and on[2] == never[2], what
            else:
                # the two planar calls now go through the staging rows, counted by the existing rule; the egress kernel
                # is the plain one
                assert [s for _, s in never[0]] == [("", ""), ("", "k_pcm_out"), ("", "")], what
                assert [s for _, s in on[0]] == [("", "k_pcm_rows_out"), ("", "k_pcm_out"), ("", "k_pcm_rows_out")], what
                assert on[2] == 2, what
