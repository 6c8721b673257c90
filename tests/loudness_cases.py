"""The loudness meter of the PCM egress (include/r8bsrc.h "loudness"; csrc/r8b_loudness.h): oracle and checks shared by the
emulated and the GPU tier of tests/test_loudness.py.

The oracle is a Python restatement of the definition in exact rational arithmetic: an fma is
float(Fraction(a) * Fraction(b) + Fraction(c)), correctly rounded.  It takes x from the call's own F64 output and the
constants from r8b_loudness_design, and runs the segments as the header states them -- Z_k from zero state, the hand-off
chain, z from S_k, the pieces, the sub-block sums.  Some twenty exact fmas per frame: oracle streams stay at a few
thousand frames, at Dst = 8000 (H = 800).  Equality with the meter is BITWISE wherever the oracle, or another run of the
meter, is the reference."""
import ctypes as C
import importlib
import math
import os
import re
from fractions import Fraction

import numpy as np

import true_peak_cases as TP

r8b = importlib.import_module("r8brain-free-src_amd")
ROOT = TP.ROOT
F64, S16 = TP.F64, TP.S16
ATT = TP.ATT
M = 64
H = 800          # the sub-block at 8000 Hz
_TEXT = open(os.path.join(ROOT, "r8brain-free-src_amd", "csrc", "r8b_loudness.h")).read()
TILE = int(re.search(r"kLdTile = (\d+);", _TEXT).group(1))
assert M == int(re.search(r"kLdSeg = (\d+);", _TEXT).group(1)) and TILE % M == 0
CUTS = [1, 63, 64, 65, H - 1, H, H + 1, TILE - 1, TILE, TILE + 1]
Tier = TP.Tier
noise, call, same_bits = TP.noise, TP.call, TP.same_bits


# ---------------------------------------------------------------- the constants
def design(lib, rate):
    """(coef[10], phi[16], hop) of r8b_loudness_design, or None where it refuses the rate"""
    coef, phi, hop = np.zeros(10), np.zeros(16), C.c_longlong()
    dp = C.POINTER(C.c_double)
    if lib.r8b_loudness_design(float(rate), coef.ctypes.data_as(dp), phi.ctypes.data_as(dp), C.byref(hop)) != 0:
        return None
    return coef, phi, hop.value


def formulas(fs):
    """the header's formulas in Python's fp64"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = math.pow(10.0, G / 20.0)
    Vb = math.pow(Vh, 0.4996667741545416)
    a0 = 1.0 + K / Q + K * K
    c = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0,
         (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    return np.array(c + [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])


# ---------------------------------------------------------------- the oracle
def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def frame(c, x, s):
    """one frame on the state list s = [p1, q1, p2, q2], in place: z"""
    if x == 0.0 and s[0] == 0.0 and s[1] == 0.0 and s[2] == 0.0 and s[3] == 0.0:
        return 0.0      # (every product and sum is an exact zero)
    y = fma(c[0], x, s[0])
    s[0] = fma(-c[3], y, fma(c[1], x, s[1]))
    s[1] = fma(-c[4], y, c[2] * x)
    z = fma(c[5], y, s[2])
    s[2] = fma(-c[8], z, fma(c[6], y, s[3]))
    s[3] = fma(-c[9], z, c[7] * y)
    return z


def oracle_phi(c):
    phi = np.zeros(16)
    for j in range(4):
        s = [0.0] * 4
        s[j] = 1.0
        for _ in range(M):
            frame(c, 0.0, s)
        for i in range(4):
            phi[4 * i + j] = s[i]
    return phi


_ORACLE = {}


def oracle(x, des, clip=False):
    """the sums of the sub-blocks the frames x complete: a stream runs its whole segments; a clip (clip=True) runs its
    last segment filled with zeros and stores len(x) // hop sub-blocks"""
    coef, phi, hop = des
    x = np.asarray(x, dtype=np.float64)
    key = (x.tobytes(), coef.tobytes(), hop, clip)
    if key in _ORACLE:
        return _ORACLE[key]
    x = np.where(np.isfinite(x), x, 0.0)
    limit = len(x) // hop if clip else None
    nseg = -(-len(x) // M) if clip else len(x) // M
    x = np.concatenate([x, np.zeros(nseg * M)])[:nseg * M]
    S, sums, A = [0.0] * 4, [], 0.0
    for k in range(nseg):
        seg = [float(v) for v in x[k * M:(k + 1) * M]]
        s = list(S)
        pieces = {}
        for j, v in enumerate(seg):
            z = frame(coef, v, s)
            b = (k * M + j) // hop
            pieces[b] = fma(z, z, pieces.get(b, 0.0))
        Z = [0.0] * 4
        for v in seg:
            frame(coef, v, Z)
        S = [fma(phi[4 * i + 3], S[3], fma(phi[4 * i + 2], S[2], fma(phi[4 * i + 1], S[1], fma(phi[4 * i], S[0], Z[i]))))
             for i in range(4)]
        for b in sorted(pieces):
            A = A + pieces[b]
            if (b + 1) * hop - 1 < (k + 1) * M:
                sums.append(A)
                A = 0.0
    sums = np.array(sums[:limit] if clip else sums)
    _ORACLE[key] = sums
    return sums


def metered(tier, nch, src, dst, chunk, capacity=600):
    a = tier.make(nch, src, dst, chunk, att=ATT)
    a.enable_loudness(capacity=capacity)
    return a


def feed(tier, a, x, cuts=()):
    """the stream x [nch, N] cut at `cuts` (the rest in one more call): the output rows [nch, n] of the whole stream"""
    rows, pos = [], 0
    for l in list(cuts) + [x.shape[1] - sum(cuts)]:
        if l > 0:
            rows.append(call(tier, a, x[:, pos:pos + l]))
            pos += l
    return np.concatenate(rows, axis=1)


def same_store(got, want, what):
    (gs, gc), (ws, wc) = got, want
    assert np.array_equal(gc, wc), (what, gc, wc)
    assert gs.shape == ws.shape, (what, gs.shape, ws.shape)
    for c in range(len(gc)):
        same_bits(gs[c, :gc[c]], ws[c, :wc[c]], "%s, channel %d" % (what, c))


def against_oracle(a, rows, what, clip=False, lens=None):
    """the object's store against the oracle over the output rows"""
    des = design(a._lib, a._rates[1])
    sums, counts = a.read_loudness()
    for c in range(rows.shape[0] if lens is None else len(lens)):
        want = oracle(rows[c] if lens is None else rows[c][:lens[c]], des, clip)
        assert counts[c] == len(want), (what, c, counts[c], len(want))
        same_bits(sums[c, :counts[c]], want, "%s, channel %d" % (what, c))
    return sums, counts


def ref_store(tier, rows):
    """the store a fresh pass-through 8000 -> 8000 object has after the frames rows [nch, n] in one call"""
    b = metered(tier, rows.shape[0], 8000.0, 8000.0, rows.shape[1])
    assert np.array_equal(call(tier, b, rows), rows)
    return b.read_loudness()


# 1. the constants
def check_design(tier):
    lib = tier.make(1, 8000.0, 8000.0, 16)._lib
    coef, phi, hop = design(lib, 48000.0)
    table = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
             1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]
    assert np.abs(coef - np.array(table)).max() < 1e-12, coef
    assert hop == 4800
    for fs in (8000.0, 44100.0, 96000.0, 48000.0):
        coef, phi, hop = design(lib, fs)
        want = formulas(fs)
        assert np.all(np.abs(coef - want) <= 4 * np.spacing(np.abs(want))), (fs, coef, want)
        assert hop == int(fs / 10 + 0.5)
        same_bits(phi + 0.0, oracle_phi(coef) + 0.0, "the hand-off matrix at %g" % fs)
        # the high-pass's state does not reach the shelf's
        assert np.all(phi.reshape(4, 4)[:2, 2:] == 0.0) and np.all(phi.reshape(4, 4)[2:, :2] != 0.0)
    for fs, want in ((11025.0, 1103), (22050.0, 2205), (8000.0, 800), (44100.0, 4410)):
        assert design(lib, fs)[2] == want
    assert design(lib, 7999.0) is None and design(lib, float("nan")) is None
    a = tier.make(1, 8000.0, 4000.0, 64, att=ATT)
    try:
        a.enable_loudness()
        raise AssertionError("Dst = 4000 was accepted")
    except RuntimeError as e:
        assert "8000" in str(e)
    assert a._lib.r8b_batch_loudness_read(a._h, None, 0, None, 0, None) == -1
    assert tier.make(1, 8000.0, 8000.0, 64).loudness_hop == 800


# 2. the specification
def check_spec(tier):
    """three channels, 2 H + 3 M + 17 frames (two sub-blocks, a call that ends inside a segment), Src == Dst and a chain"""
    N = 2 * H + 3 * M + 17
    x = noise(3, N, 921)
    a = metered(tier, 3, 8000.0, 8000.0, N)
    rows = feed(tier, a, x)
    assert np.array_equal(rows, x)
    _, counts = against_oracle(a, rows, "8000 -> 8000")
    assert list(counts) == [2, 2, 2]
    # the chain: enough input for the same number of output frames
    b = metered(tier, 3, 16000.0, 8000.0, 1024)
    xin = noise(3, 9000, 922)     # (the chain's first outputs make up its latency)
    rows = feed(tier, b, xin, [1024] * 8)
    assert rows.shape[1] >= N, rows.shape
    _, counts = against_oracle(b, rows, "16000 -> 8000")
    assert list(counts) == [rows.shape[1] // M * M // H] * 3 and counts[0] >= 2


# 3. cut invariance
def check_cuts(tier):
    """a stream longer than two tiles, one call against two calls cut at every length of CUTS, and against the stream
    cut at all of them in turn"""
    N = sum(CUTS) + 333
    assert N > 2 * TILE
    x = noise(2, N, 923)
    whole = metered(tier, 2, 8000.0, 8000.0, N)
    feed(tier, whole, x)
    want = whole.read_loudness()
    assert list(want[1]) == [N // M * M // H] * 2
    a = metered(tier, 2, 8000.0, 8000.0, N)
    for cut in CUTS:
        a.clear()
        feed(tier, a, x, [cut])
        same_store(a.read_loudness(), want, "cut at %d" % cut)
    a.clear()
    feed(tier, a, x, CUTS)
    same_store(a.read_loudness(), want, "cut at all of them")
    a.clear()
    feed(tier, a, x, CUTS[::-1])
    same_store(a.read_loudness(), want, "cut backwards")
    # ... and a chain, whose calls yield what they yield
    xin = noise(2, 3 * TILE, 924)
    b = metered(tier, 2, 16000.0, 8000.0, 3 * TILE)
    rows = feed(tier, b, xin)
    c = metered(tier, 2, 16000.0, 8000.0, 3 * TILE)
    assert np.array_equal(feed(tier, c, xin, [1, 63, 64, 65, 2 * H - 1, 2 * H + 1, TILE + 1]), rows)
    same_store(c.read_loudness(), b.read_loudness(), "16000 -> 8000, cut")


# 4. the lone sample
def check_lone_sample(tier):
    where = [0, 63, 64, TILE - 1, TILE, TILE + 1]
    N = -(-(TILE + 2) // H) * H + M      # the sub-block the last impulse lies in completes
    x = np.zeros((len(where), N))
    for c, j in enumerate(where):
        x[c, j] = (0.5 + c / 16.0) * (-1) ** c
    a = metered(tier, len(where), 8000.0, 8000.0, N)
    rows = feed(tier, a, x)
    sums, counts = against_oracle(a, rows, "lone sample")
    for c, j in enumerate(where):
        assert np.all(sums[c, :j // H] == 0.0) and sums[c, j // H] > 0.0, (c, j, sums[c])


# 5. non-finite samples
def check_nonfinite(tier):
    N = 3 * H
    x = noise(4, N, 925)
    bad = x.copy()
    bad[0, 100] = np.nan
    bad[1, 100], bad[1, 863] = np.inf, -np.inf
    bad[2, 0], bad[2, 63], bad[2, 64] = -np.inf, np.nan, np.inf
    zeroed = np.where(np.isfinite(bad), bad, 0.0)
    a, b = metered(tier, 4, 8000.0, 8000.0, N), metered(tier, 4, 8000.0, 8000.0, N)
    feed(tier, a, bad, [900])
    feed(tier, b, zeroed, [900])
    got = a.read_loudness()
    assert np.all(np.isfinite(got[0])) and np.all(got[0] > 0) and list(got[1]) == [2] * 4
    same_store(got, b.read_loudness(), "non-finite samples against zeros")


# ---------------------------------------------------------------- 6. clips
CLIP_LENS = [0, 1, 63, 64, H - 1, H, 2 * H + 100, 3 * H + 37]    # MaxInLen 500: steps that end inside segments


def _clip_reference(tier, outs):
    """the streaming run of "clip followed by zeros" of every channel"""
    n = max(max(len(y) for y in outs), 1)
    n = -(-n // M) * M + M
    rows = np.zeros((len(outs), n))
    for c, y in enumerate(outs):
        rows[c, :len(y)] = y
    return ref_store(tier, rows)


def _check_clip_call(tier, a, what, entry, K, rows, in_len, out_len, *args):
    outs = TP.clip_call(tier, a, entry, K, rows, in_len, out_len, *args)
    sums, counts = a.read_loudness()
    ref, _ = _clip_reference(tier, outs)
    for c, y in enumerate(outs):
        assert counts[c] == len(y) // H == out_len[c // K] // H, (what, c, counts[c], len(y))
        same_bits(sums[c, :counts[c]], ref[c, :counts[c]], "%s, channel %d" % (what, c))
    return outs


def check_clips_pass(tier):
    """Src == Dst: the five entries, strided and packed, interleaved and planar, K = 1 and K = 2; twice on one object"""
    T = max(CLIP_LENS) + 3
    nch = len(CLIP_LENS)
    a = metered(tier, nch, 8000.0, 8000.0, 500)
    for entry, K, in_il, out_il, packed in TP.CLIP_FORMS:
        lens = CLIP_LENS if K == 1 else [H, 3 * H + 37, 2 * H + 100, 65]
        rows = noise(nch, T, 926)
        what = "%s K=%d in %s out %s %s" % (entry, K, "il" if in_il else "planar", "il" if out_il else "planar",
                                           "packed" if packed else "strided")
        flags = r8b.CLIPS_DROP_FINISHED | r8b.CLIPS_LONGEST_FIRST if entry == "sched" else 0
        _check_clip_call(tier, a, what, entry, K, rows, lens, lens, in_il, out_il, packed, flags)
        # the same object again, other samples: state and store start empty
        _check_clip_call(tier, a, what + ", second call", entry, K, rows[::-1] * 0.5, lens, lens, in_il, out_il, packed, flags)
    # against the oracle once: a clip that ends inside a segment
    lens = [H + 100, H, 65, 0]
    b = metered(tier, 4, 8000.0, 8000.0, 500)
    outs = TP.clip_call(tier, b, "clips", 1, noise(4, H + 100, 927), lens, lens)
    against_oracle(b, outs, "clips against the oracle", clip=True, lens=lens)


def check_clips_chain(tier):
    """16000 -> 8000, six clips of unequal length: plain, and DROP_FINISHED | LONGEST_FIRST, values in the caller's order;
    K = 2 interleaved"""
    in_len = [2 * H + 77, 0, 6 * H + 130, 300, 4 * H + 2, 5 * H]
    a = metered(tier, 6, 16000.0, 8000.0, 1000)
    out_len = [a.clip_out_len(16000.0, 8000.0, n) for n in in_len]
    rows = noise(6, max(in_len) + 3, 928)
    _check_clip_call(tier, a, "chain, flags 0", "sched", 1, rows, in_len, out_len, False, False, True, 0)
    plain = a.read_loudness()
    assert list(plain[1]) == [n // H for n in out_len] and plain[1][2] == 3
    flags = r8b.CLIPS_DROP_FINISHED | r8b.CLIPS_LONGEST_FIRST
    _check_clip_call(tier, a, "chain, drop | longest first", "sched", 1, rows, in_len, out_len, False, False, True, flags)
    sched = a.read_loudness()
    # (longest first pairs other channels in the pair kernels: the outputs agree to rounding only, and so do the sums)
    assert np.array_equal(sched[1], plain[1]) and np.allclose(sched[0], plain[0], rtol=1e-9, atol=0)
    _check_clip_call(tier, a, "chain, K = 2 interleaved, drop | longest first", "sched", 2, rows, in_len[::2], out_len[::2],
                     True, True, False, flags)
    # a clip call's store lasts until the next metered call, which starts from an empty one
    a.clear()
    x = noise(6, 8000, 929)
    out = feed(tier, a, x, [1000] * 7)
    assert out.shape[1] > 2 * H
    same_store(a.read_loudness(), ref_store(tier, out), "a stream after the clip calls")


# ---------------------------------------------------------------- 7. lifecycle
def check_lifecycle(tier):
    a = tier.make(2, 16000.0, 8000.0, 4000, att=ATT)
    try:
        a.read_loudness()
        raise AssertionError("read before enable went through")
    except RuntimeError as e:
        assert "never enabled" in str(e)
    x = noise(2, 16000, 930)
    pre = call(tier, a, x[:, :4000])
    # enabled in mid-stream: meter frame 0 is the next call's first frame
    a.enable_loudness(capacity=2)
    assert a.read_loudness()[1].tolist() == [0, 0] and a.read_loudness()[0].shape == (2, 0)
    r1 = call(tier, a, x[:, 4000:7400])
    assert pre.shape[1] > 0 and 2 * H <= r1.shape[1] < 3 * H - M
    want1 = ref_store(tier, r1)
    same_store(a.read_loudness(), want1, "enabled in mid-stream")
    assert want1[1].tolist() == [2, 2]
    # the store is full: a call that would complete a third sub-block is refused, and nothing has changed
    blob = a.state_dict()
    try:
        call(tier, a, x[:, 7400:11400])
        raise AssertionError("a call past the capacity went through")
    except RuntimeError as e:
        assert "drain" in str(e)
    assert np.array_equal(a.state_dict(), blob)
    same_store(a.read_loudness(), want1, "after the refused call")
    same_store(a.read_loudness(drain=True), want1, "the draining read")
    assert a.read_loudness()[1].tolist() == [0, 0]
    r2 = call(tier, a, x[:, 7400:11400])
    ref = ref_store(tier, np.concatenate([r1, r2], axis=1))
    got = a.read_loudness()
    assert got[1].tolist() == [ref[1][0] - 2] * 2 and got[1][0] >= 2
    same_store(got, (ref[0][:, 2:], ref[1] - 2), "behind the drained sub-blocks")
    # disabled: kept and not moved; re-enabled: the meter starts again behind what the store holds
    a.read_loudness(drain=True)
    a.enable_loudness(capacity=600)
    r3 = call(tier, a, x[:, 11400:14000])
    kept = a.read_loudness()
    assert kept[1][0] >= 1
    a.enable_loudness(False)
    call(tier, a, 4.0 * x[:, 14000:])
    same_store(a.read_loudness(), kept, "while disabled")
    a.enable_loudness()
    same_store(a.read_loudness(), kept, "re-enabled")
    blob = a.state_dict()
    tail = noise(2, 4000, 931)
    r4 = call(tier, a, tail)
    fresh = ref_store(tier, r4)
    both = (np.concatenate([kept[0], fresh[0]], axis=1), kept[1] + fresh[1])
    same_store(a.read_loudness(), both, "re-enabled in mid-stream")
    # state_load: the meter restarts and the store stays
    b = metered(tier, 2, 16000.0, 8000.0, 4000)
    r0 = call(tier, b, x[:, :4000])
    first = b.read_loudness()
    b.load_state_dict(blob)
    assert np.array_equal(call(tier, b, tail), r4)
    same_store(b.read_loudness(), (np.concatenate([first[0], fresh[0]], axis=1), first[1] + fresh[1]), "after state_load")
    # clear(): store and state
    b.clear()
    assert b.read_loudness()[1].tolist() == [0, 0]
    rows = feed(tier, b, x[:, :8000], [4000])
    same_store(b.read_loudness(), ref_store(tier, rows), "after clear()")
    # the raw read: counts alone, a stride that is too small
    counts = (C.c_longlong * 2)()
    most = b._lib.r8b_batch_loudness_read(b._h, None, 0, counts, 0, None)
    assert most == counts[0] == counts[1] > 1
    one = np.zeros(2)
    assert b._lib.r8b_batch_loudness_read(b._h, one.ctypes.data_as(C.POINTER(C.c_double)), 1, counts, 0, None) == -1


# ---------------------------------------------------------------- 8. nothing else moves
def check_inert(tier):
    """as the true-peak meter's check: a chain whose output side is staged anyway (44100 -> 88200) and one whose last
    stage encodes a planar side itself (44100 -> 176400); meters, dither, neither; the true peak beside it"""
    Cn = TP.C
    x = noise(3, 5 * Cn, 932)
    for dst in (88200.0, 176400.0):
        for meters, dither, tp in ((True, None, True), (False, None, False), (True, 5, False), (False, 5, True)):
            res = {}
            for mode in ("never", "on", "off again"):
                a = tier.make(3, 44100.0, dst, Cn, dither=dither, meters=meters, att=ATT)
                a.set_option("timing", 1)
                if tp:
                    a.enable_true_peak()
                if mode != "never":
                    a.enable_loudness()
                if mode == "off again":
                    a.enable_loudness(False)
                out = [(call(tier, a, x[:, Cn * k:Cn * k + Cn], il, S16).tobytes(), a.boundary_symbols())
                       for k, il in enumerate((False, True, False, True, False))]
                res[mode] = (out, a.read_meters() if meters else None, a.stat("pcm_staged_sides"),
                             a.read_true_peak().tobytes() if tp else None)
                if mode == "on":
                    sums, counts = a.read_loudness()
                    assert counts[0] >= 1 and np.all(sums > 0)
            what = "-> %g, meters %s, dither %s, true peak %s" % (dst, meters, dither, tp)
            never, on, off = res["never"], res["on"], res["off again"]
            assert off == never if not meters else (off[0] == never[0] and off[2:] == never[2:]), what + ": switched off again"
            assert [b for b, _ in on[0]] == [b for b, _ in never[0]], what + ": the output bytes moved"
            assert on[3] == never[3], what + ": the true peak moved"
            for k in ("peak", "clipped", "nonfinite") if meters else ():
                assert np.array_equal(on[1][k], never[1][k]) and np.array_equal(off[1][k], never[1][k]), (what, k)
            if meters or dither is not None or tp or never[2] != 0:
                assert on[0] == never[0] and on[2] == never[2], what
            else:
                assert [s for _, s in never[0]] == [("", ""), ("", "k_pcm_out")] * 2 + [("", "")], what
                assert [s for _, s in on[0]] == [("", "k_pcm_rows_out"), ("", "k_pcm_out")] * 2 + [("", "k_pcm_rows_out")], what
                assert on[2] == 3, what


# ---------------------------------------------------------------- 8b. the three meters beside each other
SIDE = {"peak": ("peak",), "true_peak": ("true_peak",), "loudness": ("loudness",), "all": ("peak", "true_peak", "loudness")}


def _side_run(tier, src, which):
    """one object, 3 channels src -> 8000 (MaxInLen 4000), through a stream's life with the meters `which` on: one record
    (step, output bytes or None, {meter: reading as bytes}) per step.  A call's length below is in OUTPUT frames and the
    call takes src / 8000 times as many; the chain's first call after creation / clear() is a whole chunk instead, most
    of which makes up the chain's latency.  The loudness store holds 2 sub-blocks: the streams between two draining
    reads and the clips stay below 3 H frames, and the whole chunk behind the first drain completes a third"""
    ratio = int(src // 8000)
    a = tier.make(3, src, 8000.0, 4000, dither=5, att=ATT)
    x = 1.5 * noise(3, 12000, 940)
    log, pos = [], [0]

    def switch(on):
        if "peak" in which:
            a.enable_meters(on)
        if "true_peak" in which:
            a.enable_true_peak(on)
        if "loudness" in which:
            a.enable_loudness(on, capacity=2)

    def readings(reset=False):
        r = {}
        if "peak" in which:
            m = a.read_meters(reset=reset)
            r["peak"] = m["peak"].tobytes() + m["clipped"].tobytes() + m["nonfinite"].tobytes()
        if "true_peak" in which:
            r["true_peak"] = a.read_true_peak(reset=reset).tobytes()
        if "loudness" in which:
            sums, counts = a.read_loudness(drain=reset)
            r["loudness"] = b"".join(sums[c, :counts[c]].tobytes() for c in range(3)) + counts.tobytes()
        return r

    def note(step, out=None, reset=False):
        log.append((step, out, readings(reset)))

    def stream(step, n, il, first=False):
        l = 4000 if first and ratio > 1 else n * ratio
        out = call(tier, a, x[:, pos[0]:pos[0] + l], il, S16).tobytes()
        pos[0] += l
        note(step, out)

    def refused(step, text, others, fn):
        """fn() fails with `text`; the checkpoint and the readings of the meters `others` stay"""
        blob, before = a.state_dict(), readings()
        try:
            fn()
            raise AssertionError("%s went through" % step)
        except RuntimeError as e:
            assert text in str(e), (step, str(e))
        after = readings()
        assert np.array_equal(a.state_dict(), blob), step + ": the checkpoint moved"
        for m in others:
            assert m not in which or after[m] == before[m], "%s: the %s reading moved" % (step, m)
        note(step)

    switch(True)
    for k, (n, il) in enumerate(((500, False), (650, True), (450, False))):
        stream("stream %d" % k, n, il, k == 0)
    note("reset / drain", reset=True)
    note("after reset / drain")
    if "loudness" in which:
        refused("past the capacity", "drain", SIDE["all"], lambda: call(tier, a, x[:, pos[0]:pos[0] + 4000], False, S16))
    a.load_state_dict(a.state_dict())
    note("state_load")
    stream("after state_load", 900, True)
    switch(False)
    stream("disabled", 400, False)
    switch(True)
    note("re-enabled")
    stream("after re-enabling", 1000, True)
    a.clear()
    note("clear()")
    flags = r8b.CLIPS_DROP_FINISHED | r8b.CLIPS_LONGEST_FIRST
    for step, entry, outs, packed, fl in (("clips, sched", "sched", [2350, 0, 900], True, flags),
                                         ("clips, plain", "clips", [900, 2350, 0], False, 0)):
        in_len = [n * ratio + (ratio - 1 if n else 0) for n in outs]
        out_len = [a.clip_out_len(src, 8000.0, n) for n in in_len]
        assert out_len == outs
        ys = TP.clip_call(tier, a, entry, 1, x[:, :max(in_len) + 3], in_len, out_len, False, False, packed, fl)
        note(step, b"".join(y.tobytes() for y in ys))
    # (a clip call empties the loudness store and notes its clips' counts before it tests the pointers: that meter's
    # reading moves, and is compared with its alone-run's like every other)
    xin = tier.buf(np.zeros(3 * 1600 * ratio))
    tier.sync()
    refused("clips, null output", "null device pointer", ("peak", "true_peak"), lambda: a.resample_clips_ptr(
        tier.ptr(xin), F64, 1600 * ratio, [1600 * ratio, 0, 800 * ratio], 0, F64, 1600, [1600, 0, 800]))
    pos[0] = 0
    stream("stream after the clips 0", 600, True, True)
    stream("stream after the clips 1", 500 * ratio, False)
    return log


def check_side_by_side(tier):
    """the peak/clip meters, the true-peak meter and the loudness meter on one object through a stream's life -- streaming
    calls to dithered S16, a resetting / draining read, a call refused by the loudness capacity, a checkpoint loaded,
    switched off and on again in mid-stream, clear(), a scheduled and a plain clip call, a clip call refused for its null
    output pointer, a stream again: every meter reads at every step, bit for bit, what it reads when it is the only one
    switched on, the output bytes are those of the three alone-runs, and a refused call leaves the checkpoint and the other
    meters' readings alone (_side_run).  A chain whose sub-block is 800 frames, a lone channel behind the pair; and a
    pass-through object, which has no stage"""
    for src in (16000.0, 8000.0):
        runs = {name: _side_run(tier, src, which) for name, which in SIDE.items()}
        both = runs["all"]
        assert any(step == "past the capacity" for step, _, _ in both) and len(both) == 17
        for name in ("peak", "true_peak", "loudness"):
            alone = {step: (out, r) for step, out, r in runs[name]}
            assert len(alone) == len(both) - (name != "loudness")
            for step, out, r in both:
                if step == "past the capacity" and name != "loudness":
                    continue
                what = "%g -> 8000, %s, %s" % (src, name, step)
                assert alone[step][0] == out, what + ": the output bytes differ"
                assert alone[step][1][name] == r[name], what + ": the reading differs from the meter's alone-run"
        # the clip call refused for its pointer had emptied the loudness store and noted its own clips' counts
        null = [r for step, _, r in both if step == "clips, null output"][0]["loudness"]
        assert null[-24:] == np.array([2, 0, 1], dtype=np.int64).tobytes(), np.frombuffer(null[-24:], dtype=np.int64)
        # (the script meters something: the last readings are no zeros)
        last = both[-1][2]
        assert all(any(last[m]) for m in SIDE["all"]), last


# ---------------------------------------------------------------- 9. gating and conformance
def integrated_numpy(sums, counts, Kp, w, hop):
    """the header's gating in numpy"""
    out = []
    for p in range(sums.shape[0] // Kp):
        nb = int(min(counts[p * Kp:(p + 1) * Kp]))
        s = sums[p * Kp:(p + 1) * Kp, :nb]
        if nb < 4:
            out.append(-np.inf)
            continue
        blocks = s[:, :-3] + s[:, 1:-2] + s[:, 2:-1] + s[:, 3:]
        G = (np.asarray(w)[:, None] * blocks).sum(axis=0) / (4.0 * hop)
        with np.errstate(divide="ignore"):
            l = -0.691 + 10 * np.log10(G)
        keep = l > -70
        if not keep.any():
            out.append(-np.inf)
            continue
        gate = -0.691 + 10 * np.log10(G[keep].mean()) - 10
        keep &= l > gate
        out.append(-0.691 + 10 * np.log10(G[keep].mean()) if keep.any() else -np.inf)
    return np.array(out)


def check_gating(tier):
    a = tier.make(12, 48000.0, 48000.0, 16)
    rng = np.random.RandomState(933)
    nb = 200
    level = 10 ** (rng.uniform(-9, 0, size=(12, nb)))     # sub-block means from -90 dB up: both gates bite
    level[4:6, 50:] = 0.0                                   # silence
    level[6:8] = 1e-12                                      # nothing passes the absolute gate
    sums = level * 4800
    counts = np.full(12, nb, dtype=np.int64)
    counts[8], counts[10:] = 57, 3                         # a programme is as long as its shortest channel; too short
    for Kp, w in ((1, None), (2, None), (2, [1.0, 1.41]), (6, [1.0, 1.0, 1.0, 0.0, 1.41, 1.41])):
        got = a.integrated_loudness(sums, counts, Kp, w)
        want = integrated_numpy(sums, counts, Kp, [1.0] * Kp if w is None else w, 4800)
        assert np.array_equal(np.isfinite(got), np.isfinite(want)), (Kp, got, want)
        assert np.all(got[~np.isfinite(want)] == -np.inf)
        fin = np.isfinite(want)
        assert fin.any() and np.abs(got[fin] - want[fin]).max() < 1e-9, (Kp, got, want)
    assert a.integrated_loudness(sums, counts, 2)[3] == -np.inf and a.integrated_loudness(sums, counts, 2)[5] == -np.inf


def _tone(freq, parts, fs=48000.0):
    """a sine whose level follows parts = [(dBFS, seconds), ...]"""
    amp = np.concatenate([np.full(int(round(sec * fs)), 10 ** (db / 20.0)) for db, sec in parts])
    return amp * np.sin(2 * np.pi * freq / fs * np.arange(len(amp)))


EBU = {
    "1": (1000.0, [(-23, 20)], 2, -23.0),
    "2": (1000.0, [(-33, 20)], 2, -33.0),
    "3": (1000.0, [(-36, 10), (-23, 60), (-36, 10)], 2, -23.0),
    "4": (1000.0, [(-72, 10), (-36, 10), (-23, 60), (-36, 10), (-72, 10)], 2, -23.0),
    "5": (1000.0, [(-26, 20), (-20, 20.1), (-26, 20)], 2, -23.0),
    "mono997": (997.0, [(0, 5)], 1, -3.01),
}


def ebu_check(name):
    freq, parts, active, want = EBU[name]

    def check(tier):
        """EBU Tech 3341's synthetic signals through a 48000 -> 48000 stereo object: within the standard's own 0.1 LU"""
        sig = _tone(freq, parts)
        chunk = 480000
        a = metered(tier, 2, 48000.0, 48000.0, chunk, capacity=len(sig) // 4800 + 1)
        x = np.stack([sig, sig if active == 2 else np.zeros(len(sig))])
        for pos in range(0, len(sig), chunk):
            call(tier, a, x[:, pos:pos + chunk], False, S16)
        sums, counts = a.read_loudness()
        assert list(counts) == [len(sig) // M * M // 4800] * 2
        got = a.integrated_loudness(sums, counts, 2)[0]
        print("EBU %s reads %.4f LUFS" % (name, got))
        assert abs(got - want) <= 0.1, (name, got, want)
    check.__name__ = "check_ebu_" + name
    return check


EBU_CHECKS = [ebu_check(n) for n in EBU]
