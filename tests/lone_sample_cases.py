"""A lone sample swept across the pair kernels' cross-lane reductions (r8b_kernels.hip GpuExecP / GpuExecQ / GpuExec:
post_bits / collect_bits, post_levels / collect_levels, post_shift / collect_shift): shared by the emulation tier (CPU)
and the GPU tier (tests/test_lone_sample.py).

Per transform block the pair kernels decide three things from words reduced over the block's threads: whether a channel is
silent (exact zeros out), by which power of two the quieter partner is brought to the louder one's level, and whether a
channel is faulty (Inf / NaN in its window: +0.0 in, NaN out).  With dense noise every thread holds a non-zero sample at
the channel's top exponent, so a reduction that lost a lane would still decide right.  Here ONE thread holds the sample
that decides: pair p (channels 2p, 2p + 1) carries a lone sample at source position k0 + p, k0 the start of the third
convolver block's new samples, p over `in_len` consecutive positions -- every slot of a block's new samples and, one
block later, of its history; `in_len` counts the convolver's zero-stuffed samples, so where it up-samples the sweep
spans `up` consecutive blocks, among them both blocks of a two-block workgroup -- of a stream six blocks long.

  variant A  even channel: zeros and a lone 1.0; odd channel: 1e-12 x full-scale noise (one row shared by all pairs)
  variant B  odd channel: zeros and a lone 1e-9; even channel: full-scale noise
  variant F  even pairs: the even channel is zeros and a lone NaN; odd pairs: the odd channel is zeros and a lone -Inf;
             the partner is full-scale noise
The last pass of a geometry has an unpaired last channel that carries a lone sample too.

check_lone_sample() asserts, with the project's tolerances (cases.RMS_TOL / PEAK_TOL) times the channel's own level:
  1. A, B: every channel against the compiled reference (refwrap.batch_check: per-call counts and samples), where
     oracle/_ref was built;
  2. A, B: both channels of 16 pairs spread evenly over the pass against the numpy oracle;
  3. A, B: every lone-sample channel's output has a non-zero sample (a missed lane would call it silent);
  4. F: every partner is finite and bitwise what it is beside all-zero channels;
  5. F: every faulty channel holds NaN, none farther from its sample than nonfinite_cases' property 4 allows;
  6. all: another cut of the stream into calls (nonfinite_cases._lens and a one-sample call in the middle of the sweep)
     gives the same bits, every NaN taken as the canonical one -- a level, a fault or a silence bit that leaked between
     the blocks of one wave or one workgroup would depend on which blocks a call puts side by side."""
import math
import re

import numpy as np

import r8b_oracle as O
from cases import PEAK_TOL, RMS_TOL
from nonfinite_cases import _bits, _lens, chain_geometry

# every form pinned by its options whatever the channel count (large objects take the half-array forms by default)
_PIN = {"half": 0, "half_fused": 0, "walk": 0}


def _geom(name, src, dst, maxin, tb, att, in_len, up, fft, symbol, opts=None, solo=False):
    o = dict(_PIN)
    o.update(opts or {})
    return dict(name=name, src=src, dst=dst, maxin=maxin, tb=tb, att=att, in_len=in_len, up=up, fft=fft, symbol=symbol,
                opts=o, solo=solo)


# name, (src, dst, maxin, tb, atten), the first convolver's in_len and up-sampling factor, its describe() fragment, the
# device symbol of the first stage's kernel, options
GEOMETRIES = [
    _geom("fft32", 44100.0, 96000.0, 2048, 45.0, 49.0, 48, 2, "fft=32/64", "k_convp<5, 1, 0, 24>"),          # 4 threads per block
    _geom("fft64", 44100.0, 96000.0, 2048, 30.0, 109.56, 70, 2, "fft=64/128", "k_convp<6, 1, 1, 24>"),
    _geom("fft256", 44100.0, 96000.0, 4096, 10.0, 109.56, 338, 2, "fft=256/512", "k_convp<8, 1, 1, 24>"),
    _geom("fft512", 44100.0, 88200.0, 2048, 5.0, 109.56, 678, 2, "fft=512/1024", "k_convp<9, 1, 0, 24>"),    # NT = 64
    _geom("fft1024", 44100.0, 96000.0, 4096, 2.0, 109.56, 1180, 2, "fft=1024/2048", "k_convp<10, 1, 4, 24>"),  # 2 blocks / workgroup
    _geom("cfg2", 44100.0, 96000.0, 4096, 2.0, 180.15, 2680, 2, "fft=2048/4096", "k_convp<11, 1, 4, 24>"),   # NWB = 4
    _geom("cfg3", 96000.0, 44100.0, 4096, 2.0, 180.15, 2554, 1, "fft=4096/4096", "k_convp<12, 0, 5, 24>"),
    _geom("decim", 88200.0, 44100.0, 4096, 2.0, 180.15, 2680, 1, "fft=4096/2048", "k_convp<12, -1, 0, 24>"),
    _geom("up3", 44100.0, 132300.0, 2048, 10.0, 109.56, 764, 3, "io=3/1", "k_convp<10, 0, 3, 24>"),           # 3x zero stuffing
    _geom("fft4096", 44100.0, 96000.0, 8192, 1.0, 180.15, 5358, 2, "fft=4096/8192", "k_convp<12, 1, 4, 24>"),  # 512 threads
    _geom("split", 44100.0, 88200.0, 4096, 0.5, 180.15, 10714, 2, "fft=8192/16384", "k_convp<13, 0, 8, 24>"),
    _geom("half21", 44100.0, 88200.0, 4096, 2.0, 180.15, 2680, 2, "fft=2048/4096", "k_convp<11, 1, 21, 24>", {"half": 2}),
    _geom("half23", 44100.0, 96000.0, 16384, 2.0, 180.15, 2680, 2, "fft=2048/4096", "k_convp<11, 1, 23, 24>",
          {"half_fused": 2}),
    _geom("half25", 44100.0, 48000.0, 16384, 2.0, 180.15, 2680, 2, "fft=2048/4096", "k_convp<11, 1, 25, 24>",
          {"half_fused": 2}),
    _geom("walk", 44100.0, 96000.0, 16384, 2.0, 180.15, 2680, 2, "fft=2048/4096", "k_convp_walk<11, 1, 4, 24>",
          {"walk": 2, "walk_len": 3, "half_fused": 0}),
    _geom("quad", 44100.0, 88200.0, 2048, 2.0, 180.15, 2680, 2, "fft=2048/4096", "k_convq", {"quad": 1}),
    _geom("convx", 44100.0, 96000.0, 4096, 2.0, 180.15, 2680, 2, "fft=2048/4096", "k_convx<10, 1, 1, 24>", {"pair_conv": 0}),
    # the one-channel form (16384-point blocks, no partner): r8b_convp.h applies the silence decision to it (convp_body:
    # cp_silence on the workgroup's collect_bits), so variant A's lone-sample channels are checked there
    _geom("solo", 96000.0, 44100.0, 8192, 0.5, 180.15, 10212, 1, "fft=16384/16384", "k_convp<13, 0, 18, 24>", solo=True),
]
GEOMETRY = {g["name"]: g for g in GEOMETRIES}

MAX_CHANNELS = 4096      # per object
HOST_BYTES = 1.2e9       # input and output of one pass on the host


def stream_len(g):
    """six convolver blocks, in whole calls of maxin"""
    return -(-int(math.ceil(6.0 * g["in_len"] / g["up"])) // g["maxin"]) * g["maxin"]


def passes(g, max_pairs=None):
    """[(first position, pairs, unpaired channel?)]: the geometry's in_len positions in passes of nearly equal size, at most
    max_pairs pairs each (default: MAX_CHANNELS channels and HOST_BYTES of host arrays); the last has the unpaired channel"""
    if max_pairs is None:
        n = stream_len(g)
        per_channel = 8.0 * n * (1.0 + g["dst"] / g["src"])
        max_pairs = (min(MAX_CHANNELS, int(HOST_BYTES / per_channel)) - 1) // 2
    npass = -(-g["in_len"] // max_pairs)
    res, p0 = [], 0
    for i in range(npass):
        k = g["in_len"] // npass + (1 if i < g["in_len"] % npass else 0)
        res.append((p0, k, i == npass - 1))
        p0 += k
    assert p0 == g["in_len"] and all(k <= max_pairs for _, k, _ in res)
    return res


def lone_sample_input(variant, n, k0, p0, npairs, unpaired, noise):
    """returns x, the channels' levels, the lone-sample channels and their positions"""
    nch = 2 * npairs + (1 if unpaired else 0)
    x = np.zeros((nch, n))
    level = np.ones(nch)
    p = np.arange(npairs)
    pos = k0 + p0 + p
    if variant == "A":
        ch, val = 2 * p, np.full(npairs, 1.0)
        x[1:2 * npairs:2] = 1e-12 * noise
        level[1:2 * npairs:2] = 1e-12
    elif variant == "B":
        ch, val = 2 * p + 1, np.full(npairs, 1e-9)
        x[0:2 * npairs:2] = noise
        level[ch] = 1e-9
    else:
        ch, val = 2 * p + (p & 1), np.where(p & 1, -np.inf, np.nan)
        x[2 * p + 1 - (p & 1)] = noise
    x[ch, pos] = val
    if unpaired:
        ch = np.append(ch, nch - 1)
        pos = np.append(pos, k0 + p0 + npairs // 2)
        x[nch - 1, pos[-1]] = {"A": 1.0, "B": 1e-9, "F": np.nan}[variant]
        level[nch - 1] = {"A": 1.0, "B": 1e-9, "F": 1.0}[variant]
    return x, level, ch, pos


class HostRunner:
    """streams through process_host; arrays are numpy"""

    def put(self, x):
        return x

    def host(self, y):
        return y

    def stream(self, b, x, lens):
        ys, pos = [], 0
        for l in lens:
            ys.append(b.process_host(x[:, pos:pos + l]))
            pos += l
        assert pos == x.shape[1]
        return np.concatenate(ys, axis=1), [y.shape[1] for y in ys]

    def zeroed(self, x, rows):
        x = x.copy()
        x[rows] = 0.0
        return x

    def same_bits(self, a, b, rows=None):
        if rows is not None:
            a, b = a[rows], b[rows]
        return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


class DeviceRunner:
    """streams through process() on device tensors; outputs stay on the device for the bitwise comparisons"""

    def __init__(self, torch):
        self.t = torch

    def put(self, x):
        return self.t.from_numpy(x).cuda()

    def host(self, y):
        return y.cpu().numpy()

    def stream(self, b, x, lens):
        ys, pos = [], 0
        for l in lens:
            ys.append(b.process(x[:, pos:pos + l]).clone())
            pos += l
        assert pos == x.shape[1]
        return self.t.cat(ys, dim=1), [y.shape[1] for y in ys]

    def zeroed(self, x, rows):
        x = x.clone()
        x[self.t.as_tensor(np.asarray(rows), device=x.device)] = 0.0
        return x

    def same_bits(self, a, b, rows=None):
        t = self.t
        if rows is not None:
            idx = t.as_tensor(np.asarray(rows), device=a.device)
            a, b = a[idx], b[idx]
        if a.shape != b.shape:
            return False
        nan = t.full((), float("nan"), dtype=a.dtype, device=a.device)
        a, b = t.where(t.isnan(a), nan, a).contiguous(), t.where(t.isnan(b), nan, b).contiguous()
        return t.equal(a.view(t.int64), b.view(t.int64))


def _first_difference(runner, a, b, rows=None):
    a, b = runner.host(a), runner.host(b)
    if rows is not None:
        a, b = a[rows], b[rows]
    if a.shape != b.shape:
        return (a.shape, b.shape)
    c, j = np.nonzero(_bits(a) != _bits(b))
    return (int(c[0] if rows is None else np.asarray(rows)[c[0]]), int(j[0]), len(c)) if len(c) else None


_NOISE = {}
_ORACLE_CACHE = {}


def _noise(n):
    if n not in _NOISE:
        _NOISE[n] = O.splitmix_uniform(77, n)
    return _NOISE[n]


def _oracle(g, v, lens, shared):
    """the numpy oracle over the calls of `lens`; the shared noise rows are computed once per geometry"""
    key = (g["name"], shared, len(v)) if shared else None
    if key is not None and key in _ORACLE_CACHE:
        return _ORACLE_CACHE[key]
    o = O.OracleResampler(g["src"], g["dst"], g["maxin"], g["tb"], g["att"])
    ys, pos = [], 0
    for l in lens:
        ys.append(o.process(v[pos:pos + l]))
        pos += l
    y = np.concatenate(ys)
    if key is not None:
        _ORACLE_CACHE[key] = y
    return y


def check_lone_sample(make, runner, g, variant, p0, npairs, unpaired, refwrap=None):
    """`make(nch)` builds a fresh object of the geometry with its options set.  Returns the record of the pass: pairs,
    worst own-level (rms, peak) against the compiled reference (None without it) and against the numpy oracle."""
    src, dst, maxin = g["src"], g["dst"], g["maxin"]
    nch = 2 * npairs + (1 if unpaired else 0)
    assert nch <= MAX_CHANNELS
    b = make(nch)
    desc = b.describe()
    conv = [l for l in desc.splitlines() if l.startswith("BlockConvolver")][0]
    assert g["fft"] in conv and int(re.search(r"in_len=(\d+)", conv).group(1)) == g["in_len"] and \
        int(re.search(r"io=(\d+)/", conv).group(1)) == g["up"], conv
    block_src, window, later = chain_geometry(desc, src)
    assert block_src * g["up"] == g["in_len"]
    n = stream_len(g)
    k0 = int(math.ceil(2.0 * block_src))
    assert 0 <= p0 and p0 + npairs <= g["in_len"] and k0 + g["in_len"] + block_src <= n
    x, level, lone, lone_pos = lone_sample_input(variant, n, k0, p0, npairs, unpaired, _noise(n))
    where = lambda c: "channel %d (pair %d of the sweep, source position %d)" % (c, p0 + c // 2, k0 + p0 + c // 2)

    lens = [maxin] * (n // maxin)
    xd = runner.put(x)
    b.set_option("timing", 1)
    yd, counts = runner.stream(b, xd, lens)
    assert b.stage_symbols()[0] == g["symbol"], b.stage_symbols()
    y = runner.host(yd)
    assert y.shape[0] == nch and y.shape[1] > 0
    rec = {"pairs": npairs, "ref": None, "oracle": None}

    if variant in "AB":
        # (the one-channel form has no partner: its lone-sample channels only)
        rows = lone if g["solo"] else np.arange(nch)
        # 3. the silence decision: a lone sample is not silence
        nz = np.array([y[c].any() for c in lone])
        assert nz.all(), "exact zeros out of " + where(int(lone[np.argmin(nz)]))
        # 1. every channel against the compiled reference, each at its own level
        if refwrap is not None:
            r, p = refwrap.batch_check(src, dst, maxin, lens, x, y, counts, g["tb"], g["att"])
            r, p = r / level, p / level
            rec["ref"] = (float(r[rows].max()), float(p[rows].max()))
            bad = rows[(r[rows] > RMS_TOL) | (p[rows] > PEAK_TOL)]
            assert len(bad) == 0, "%d channels miss the own-level bound against the reference, first: %s rms %.3g peak %.3g" % (
                len(bad), where(int(bad[0])), r[bad[0]], p[bad[0]])
        # 2. both channels of 16 pairs spread over the pass against the numpy oracle
        worst_r = worst_p = 0.0
        for q in np.unique(np.linspace(0, npairs - 1, 16).round().astype(int)):
            for c in (2 * q, 2 * q + 1):
                if g["solo"] and c not in lone:
                    continue
                yo = _oracle(g, x[c], lens, None if c in lone else variant)
                assert len(yo) == y.shape[1], (len(yo), y.shape)
                d = (y[c] - yo) / level[c]
                rr, pp = math.sqrt(float(np.mean(d * d))), float(np.abs(d).max())
                worst_r, worst_p = max(worst_r, rr), max(worst_p, pp)
                assert rr <= RMS_TOL and pp <= PEAK_TOL, "%s misses the own-level bound against the oracle: rms %.3g peak %.3g" % (
                    where(int(c)), rr, pp)
        rec["oracle"] = (worst_r, worst_p)
    else:
        faulty = lone
        partners = np.setdiff1d(np.arange(nch), faulty)
        # 4. partners: finite, and bitwise what they are beside all-zero channels
        fin = np.isfinite(y[partners]).all(axis=1)
        assert fin.all(), "Inf / NaN reached " + where(int(partners[np.argmin(fin)]))
        yz, _ = runner.stream(make(nch), runner.zeroed(xd, faulty), lens)
        assert runner.same_bits(yd, yz, partners), \
            "partners differ from their run beside zeros, first (channel, output, count): %s" % (
                _first_difference(runner, yd, yz, partners),)
        del yz
        # 5. every faulty channel holds NaN, inside the span its sample can reach
        nan = np.isnan(y[faulty])
        has = nan.any(axis=1)
        assert has.all(), "no NaN in " + where(int(faulty[np.argmin(has)]))
        first, last = nan.argmax(axis=1), y.shape[1] - 1 - nan[:, ::-1].argmax(axis=1)
        margin = int(math.ceil(block_src * dst / src + later * dst)) + 2
        span = margin + int(math.ceil(window * dst))
        lat = b.getInLenBeforeOutPos(0)
        lo = np.floor((lone_pos - lat) * dst / src).astype(np.int64) - span
        hi = np.ceil((lone_pos - lat) * dst / src).astype(np.int64) + span
        out = (first < lo) | (last > hi)
        assert not out.any(), "NaN outside its span in %s: outputs %d ... %d, allowed %d ... %d" % (
            where(int(faulty[np.argmax(out)])), first[np.argmax(out)], last[np.argmax(out)], lo[np.argmax(out)], hi[np.argmax(out)])

    # 6. another cut into calls: a call ends in the middle of the sweep, a one-sample call follows it
    lens2, at = _lens(n, maxin, k0 + p0 + npairs // 2)
    assert at is not None and at + 1 < len(lens2)
    if lens2[at + 1] > 1:
        lens2[at + 1:at + 2] = [1, lens2[at + 1] - 1]
    assert sum(lens2) == n and 1 in lens2
    y2, _ = runner.stream(make(nch), xd, lens2)
    assert runner.same_bits(yd, y2), "the output depends on the cut into calls, first (channel, output, count): %s" % (
        _first_difference(runner, yd, y2),)
    return rec
