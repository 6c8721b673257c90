"""Inf / NaN samples stay in their own channel (include/r8bsrc.h, r8b_convp.h cp_level_shift): shared by the emulation
tier (CPU) and the GPU tier (tests/test_nonfinite.py).

The pair kernels convolve channels 2c and 2c+1 as the real and imaginary part of one complex transform.  A channel whose
block window holds an Inf or a NaN is FAULTY in that block: it goes into the transform as +0.0 and every output of the
block comes out as NaN, so that its partner is computed exactly as beside a silent channel.  check_nonfinite() feeds a
batch of nine channels -- four pairs and an unpaired last channel -- in which some channels carry non-finite samples, and
checks, per call sequence:
  1. partners: finite everywhere, the usual tolerance of their own level against their own oracle, and -- beside a faulty
     channel that is zero apart from its non-finite samples -- bitwise what they are beside an all-zero channel;
  2. a faulty channel is non-finite wherever its non-finite inputs reach (the oracle's response to them, as 1.0 over an
     all-zero background, is non-zero there);
  3. wherever a faulty channel is finite, it meets the usual tolerance against the oracle on the same input with the
     non-finite samples replaced by 0;
  4. no NaN lies farther than one convolver block (at the output rate, with the later stages' filter lengths) from
     that reach, and the output is finite again behind it;
  5. another cut of the stream into calls, with a checkpoint saved and loaded into a fresh object in the middle of a NaN
     run, gives the same outputs bit for bit, NaN positions included (a NaN's sign and payload aside: _bits)."""
import math
import re

import numpy as np

import r8b_oracle as O
from cases import PAIR_SCALE_CASES, PEAK_TOL, RMS_TOL

# (src, dst, maxin, chunk, n_in, tb, atten[, engine options]): the pair-kernel forms of cases.PAIR_SCALE_CASES (fused 2x up,
# fused 1:1 with In > Out, convolver alone, decimating, 3x zero stuffing, several blocks per workgroup, half-band cascade
# behind, the one-channel and split forms of the long blocks), a half-band decimator in front, cfg5's chain, the polyphase
# 3x form (kernel mode 19) on each of its geometries -- 4096 points with four blocks per workgroup, 8192 with two, 16384
# with one --, and the option-selected forms: eight elements per thread ("quad"), the half-band decimator fused into the
# convolver's load ("fuse_hbconv") and the walk form ("walk")
NONFINITE_CASES = list(PAIR_SCALE_CASES) + [
    (44100.0, 132300.0, 2048, 1500, 2048 * 8, 4.0, 180.15),
    (44100.0, 132300.0, 2048, 2048, 2048 * 8, 2.0, 180.15),
    (44100.0, 132300.0, 8192, 8192, 8192 * 4, 1.0, 180.15),
    (176400.0, 44100.0, 4096, 3000, 4096 * 8, 2.0, 180.15),
    (44100.0, 2822400.0, 1024, 1024, 1024 * 8, 2.0, 180.15),
    (44100.0, 88200.0, 2048, 2048, 2048 * 6, 2.0, 180.15, {"quad": 1}),
    (176400.0, 44100.0, 4096, 4096, 4096 * 8, 2.0, 180.15, {"fuse_hbconv": 1}),
    (44100.0, 96000.0, 16384, 16384, 16384 * 4, 2.0, 180.15, {"walk": 2, "walk_len": 3, "half_fused": 0}),
]
# minimum-phase chains (r8b_batch_create_ex ReqPhase = 1: complex kernel spectra -- modes 6 / 7, 16 / 17, 12 ... 15): the
# numpy oracle has no minimum-phase designer, so properties 1 (bitwise), 4 and 5 are checked on them
NONFINITE_MINPHASE_CASES = [
    (44100.0, 88200.0, 4096, 4096, 4096 * 4, 2.0, 180.15),
    (44100.0, 96000.0, 4096, 3000, 4096 * 4, 2.0, 180.15),
    (44100.0, 88200.0, 2048, 2048, 2048 * 24, 0.5, 180.15),
]

NCH = 9
ZERO_FAULTY = (0, 3, 6)       # faulty channels that are zero apart from their non-finite samples
PARTNERS = (1, 2, 5, 7)       # ... the faulty channels' partners, finite
FAULTY = (0, 3, 4, 6, 8)      # 4: full-scale noise with a few non-finite samples; 8: the unpaired last channel
LEVELS = [0.0, 1.0, 1.0, 0.0, 1.0, 1e-6, 0.0, 1.0, 1.0]


def chain_geometry(desc, src):
    """from r8b_batch_describe: the first convolver's new input samples per block, in source samples; its window and the
    filter lengths of the stages behind it, in seconds (times dst: output samples)"""
    rate = float(src)
    block_src = None
    window = 0.0
    later = 0.0
    for line in desc.splitlines():
        if line.startswith("HBDownsampler"):
            taps = int(re.search(r"taps=(\d+)", line).group(1))
            if block_src is not None:
                later += 4.0 * taps / rate
            rate /= 2.0
        elif line.startswith("HBUpsampler"):
            taps = int(re.search(r"taps=(\d+)", line).group(1))
            later += 4.0 * taps / rate
            rate *= 2.0
        elif line.startswith("BlockConvolver"):
            up, down = map(int, re.search(r"io=(\d+)/(\d+)", line).groups())
            fft_in = int(re.search(r"fft=(\d+)/", line).group(1))
            in_len = int(re.search(r"in_len=(\d+)", line).group(1))
            if block_src is None:
                block_src = in_len / up * (src / rate)
                window = fft_in / rate             # (a window in input samples: fft_in at most)
            else:
                later += fft_in / rate
            rate = rate * up / down
        elif line.startswith("FracInterpolator"):
            a, b = map(float, re.search(r"([\d.]+)->([\d.]+)", line).groups())
            taps = int(re.search(r"taps=(\d+)", line).group(1))
            later += 2.0 * taps / a
            rate = b
    assert block_src is not None, desc
    return block_src, window, later


def nonfinite_input(n, chunk, block_src, seed0=21):
    """nine channels (ZERO_FAULTY / PARTNERS / FAULTY above); returns the samples and the NaN run of channel 3"""
    x = np.zeros((NCH, n))
    for c in (1, 2, 4, 7, 8):
        x[c] = O.splitmix_uniform(seed0 + c, n)
    x[5] = 1e-6 * O.splitmix_uniform(seed0 + 5, n)
    # channel 0: a single NaN, later a -Inf
    x[0, n // 5 + 7] = np.nan
    x[0, n // 3] = -np.inf
    # channel 3: a run of NaNs longer than one block
    r0 = n // 4
    r1 = r0 + int(1.25 * block_src) + 1
    assert r1 < 2 * n // 3, (n, block_src)
    x[3, r0:r1] = np.nan
    # channel 4: full-scale noise with a few NaNs and a +Inf
    x[4, n // 6] = np.nan
    x[4, n // 6 + 100] = np.inf
    x[4, n // 3 + 5] = np.nan
    # channel 6: the first sample of a call, the last sample of a call (its block parks outputs for the next call)
    k = max(1, (n // chunk) // 3)
    x[6, k * chunk] = np.nan
    x[6, (k + 1) * chunk - 1] = np.nan
    # channel 8, unpaired
    x[8, n // 2] = np.nan
    return x, (r0, r1)


def _stream(b, x, lens, save_at=None, make=None):
    ys, pos = [], 0
    for i, l in enumerate(lens):
        ys.append(b.process_host(x[:, pos:pos + l]))
        pos += l
        if save_at is not None and i == save_at:
            blob = b.state_dict()
            b = make()
            b.load_state_dict(blob)
    assert pos == x.shape[1]
    return np.concatenate(ys, axis=1)


def _lens(n, maxin, cut):
    """ragged calls of at most maxin samples; one of them ends at `cut` (returned: its index)"""
    lens, pos, i, at = [], 0, 0, None
    pattern = [maxin // 2 + 3, maxin, 777 % maxin + 1, 1, maxin // 3 + 1, maxin]
    while pos < n:
        l = min(pattern[i % len(pattern)], n - pos)
        if pos < cut < pos + l:
            l = cut - pos
        lens.append(l)
        pos += l
        if pos == cut:
            at = len(lens) - 1
        i += 1
    return lens, at


_ORACLE_CACHE = {}


def _oracle(src, dst, maxin, tb, att, v):
    key = (src, dst, maxin, tb, att, v.tobytes())
    if key not in _ORACLE_CACHE:
        _ORACLE_CACHE[key] = O.OracleResampler(src, dst, maxin, tb, att).process(v)
    return _ORACLE_CACHE[key]


def _bits(y):
    """the outputs' bit patterns with every NaN as the canonical quiet NaN: a NaN's sign and payload carry no data and
    are not part of the contract (where the half-band stages combine two NaNs, the device's tiling picks either)"""
    return np.where(np.isnan(y), np.nan, y).view(np.uint64)


def check_nonfinite(make, case, phase=0):
    """`make()` builds a fresh, equally configured batch object of NCH channels (engine options set).  Checks
    properties 1-5 of the module's docstring; phase 1 (minimum phase): 1 (bitwise), 4 and 5 only."""
    src, dst, maxin, chunk, n, tb, att = case[:7]
    b = make()
    block_src, window, later = chain_geometry(b.describe(), src)
    # (long blocks: a stream of eight of them at least, whole calls)
    n = max(n, -(-int(8 * block_src) // chunk) * chunk)
    x, (r0, r1) = nonfinite_input(n, chunk, block_src)
    lens = [min(chunk, n - i) for i in range(0, n, chunk)]
    y = _stream(b, x, lens)
    bad = ~np.isfinite(x)

    # 1. partners: finite; beside a channel that is zero apart from its non-finite samples, bitwise as beside zeros
    xz = x.copy()
    xz[list(ZERO_FAULTY)] = 0.0
    yz = _stream(make(), xz, lens)
    assert y.shape == yz.shape and y.shape[1] > 0
    for c in PARTNERS:
        assert np.isfinite(y[c]).all(), (c, np.flatnonzero(~np.isfinite(y[c]))[:5])
    for c in (1, 2, 7):
        assert np.array_equal(y[c].view(np.uint64), yz[c].view(np.uint64)), (c, float(np.abs(y[c] - yz[c]).max()))

    # 4. the reach of the non-finite samples, one convolver block around it at most; finite again behind it
    # (one convolver block at the output rate, with the later stages' filter lengths)
    margin = int(math.ceil(block_src * dst / src + later * dst)) + 2
    span = margin + int(math.ceil(window * dst))
    out_n = y.shape[1]
    for c in FAULTY:
        nf = np.flatnonzero(~np.isfinite(y[c]))
        assert len(nf) > 0, c
        # (the outputs a non-finite input can touch at all: from its position to one window + the later stages behind it)
        pos = np.flatnonzero(bad[c])
        lat = b.getInLenBeforeOutPos(0)
        lo = int(math.floor((pos.min() - lat) * dst / src)) - span
        hi = int(math.ceil((pos.max() - lat) * dst / src)) + span
        assert nf.min() >= lo and nf.max() <= hi, (c, nf.min(), nf.max(), lo, hi)
        if c in (0, 4):
            assert nf.max() + 1 < out_n and np.isfinite(y[c, nf.max() + 1:]).all(), c   # (finite again behind it)

    # 2., 3., 4.: against the oracle (linear phase)
    if phase == 0:
        for c in PARTNERS:
            yo = _oracle(src, dst, maxin, tb, att, x[c])
            d = y[c] - yo
            sc = LEVELS[c]
            assert math.sqrt(float(np.mean(d * d))) <= RMS_TOL * sc and float(np.abs(d).max()) <= PEAK_TOL * sc, c
        for c in FAULTY:
            reach_c = _oracle(src, dst, maxin, tb, att, bad[c].astype(np.float64)) != 0.0
            fin = np.isfinite(y[c])
            assert reach_c.any() and not fin[reach_c].any(), (c, np.flatnonzero(reach_c & fin)[:5])
            yo = _oracle(src, dst, maxin, tb, att, np.where(bad[c], 0.0, x[c]))
            d = (y[c] - yo)[fin]
            sc = max(LEVELS[c], 1.0)
            assert math.sqrt(float(np.mean(d * d))) <= RMS_TOL * sc and float(np.abs(d).max()) <= PEAK_TOL * sc, \
                (c, math.sqrt(float(np.mean(d * d))), float(np.abs(d).max()), np.flatnonzero(np.abs(d) > PEAK_TOL)[:5])
            # (every NaN within one block of that reach)
            ra = np.flatnonzero(reach_c)
            nf = np.flatnonzero(~fin)
            dist = np.abs(nf[:, None] - ra[None, :]).min(axis=1) if len(nf) * len(ra) < 5e7 else \
                np.minimum(np.abs(nf - ra[np.clip(np.searchsorted(ra, nf), 0, len(ra) - 1)]),
                           np.abs(nf - ra[np.clip(np.searchsorted(ra, nf) - 1, 0, len(ra) - 1)]))
            assert dist.max() <= margin, (c, int(dist.max()), margin)

    # 5. another cut into calls, a checkpoint in the middle of channel 3's NaN run
    lens2, save_at = _lens(n, maxin, (r0 + r1) // 2)
    y2 = _stream(make(), x, lens2, save_at=save_at, make=make)
    assert y2.shape == y.shape and np.array_equal(_bits(y2), _bits(y))
    return y
