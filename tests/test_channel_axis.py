"""GPU tier: the channel count as a tested variable.

The parity tests elsewhere run objects of at most 1024 channels.  Here: shards of one batch against the unsharded object
(the size-driven kernel choices follow option form_channels, not the shard's own count); each size-driven choice run
on both sides of its threshold with the same channels; objects whose rows start past 2^31 and 2^32 bytes; rows of a
few channels 4 GiB apart through every kernel family; and the grid's y limit of 65535 channels.

Large outputs are compared on the device; only sampled rows travel to the host for the compiled reference.  Channel
counts are derived from the engine's threshold formulas (Engine::half_worth, launch_cascade, Engine::process), so a
retuned threshold fails the symbol assertions instead of leaving a test that straddles nothing."""
import importlib
import math
import re

import numpy as np
import pytest

from cases import RMS_TOL, PEAK_TOL, make_input

pytestmark = pytest.mark.gpu

r8b = importlib.import_module("r8brain-free-src_amd")
sharding = importlib.import_module("r8brain-free-src_amd.sharding")

CFG2 = (44100.0, 96000.0)
CFG3 = (96000.0, 44100.0)
HALF_WORKGROUPS = 512        # Engine::half_worth: channel pairs x blocks of the largest call
WALK_CHANNELS = 256          # launch_fused: the walk form from this many channels
HBC_TILES = 256 * 6          # launch_cascade: channels x 8192-output tiles for the 8192 tile
POLY_CAP = 96.0 * 1048576.0  # Engine::process, poly_groups = 1: bytes between the two stages per group
POLY_MIN_PER = 512           # ... and channels per group at least


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


class _Mem:
    """peak device memory in use while a test runs (the engine allocates with hipMalloc, so torch's own counters do
    not see it: sampled from the free memory the device reports)"""

    def __init__(self, torch):
        self.t = torch
        self.free0, self.total = torch.cuda.mem_get_info()
        self.low = self.free0

    def sample(self):
        self.low = min(self.low, self.t.cuda.mem_get_info()[0])

    def report(self, what):
        print("[channel_axis] %s: peak device memory %.2f GB above the start, %.2f GB in use"
              % (what, (self.free0 - self.low) / 1e9, (self.total - self.low) / 1e9))


@pytest.fixture
def mem(torch, request):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    m = _Mem(torch)
    yield m
    m.sample()
    m.report(request.node.name)
    torch.cuda.empty_cache()


def conv_blocks(b, maxin):
    """overlap-save blocks of the object's largest call at its first convolver (Engine::half_worth's `blocks`)"""
    m = re.search(r"BlockConvolver: .*?in_len=(\d+) io=(\d+)/(\d+)", b.describe())
    in_len, up = int(m.group(1)), int(m.group(2))
    per = max(1, in_len // max(1, up))
    return -(-maxin // per)


def half_channels(src, dst, maxin):
    """smallest channel count whose objects take the half-array forms by default"""
    b = r8b.BatchResampler(src, dst, maxin, 2.0, 180.15, nch=2, device=0)
    pairs = -(-HALF_WORKGROUPS // conv_blocks(b, maxin))
    return 2 * pairs - 1


def make(src, dst, maxin, nch, opts=(), tb=2.0, att=180.15):
    b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=nch, device=0)
    for k, v in dict(opts).items():
        b.set_option(k, v)
    b.set_option("timing", 1)
    return b


def dev_input(torch, nch, l, seed, stride=None):
    """[nch, l] uniform +-1 on the device (rows of `stride` doubles when given), made in slices of rows"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.empty((nch, stride if stride else l), dtype=torch.float64, device="cuda")[:, :l]
    for c0 in range(0, nch, 2048):
        c1 = min(nch, c0 + 2048)
        x[c0:c1].copy_(torch.rand((c1 - c0, l), generator=g, dtype=torch.float64, device="cuda") * 2.0 - 1.0)
    return x


def sampled_rows(nch, cap, in_stride, extra=()):
    """>= 64 channels: the first and last pairs, pair boundaries spread over the object, the rows on both sides of the
    2^31- and 2^32-byte output and input offsets"""
    rows = {0, 1, 2, 3, nch - 2, nch - 1}
    for lim in (1 << 31, 1 << 32):
        for stride in (cap, in_stride):
            c = -(-lim // (8 * stride))
            if c < nch:
                rows |= {c - 1, c, c + 1}
    for k in range(1, 30):
        c = (k * nch // 30) & ~1
        rows |= {c - 1, c}
    rows |= set(extra)
    return sorted(r for r in rows if 0 <= r < nch)


def check_reference(refwrap, src, dst, maxin, lens, xs, ys, counts):
    x = np.concatenate(xs, axis=1)
    y = np.concatenate(ys, axis=1)
    r, p = refwrap.batch_check(src, dst, maxin, lens, x, y, counts)
    assert r.max() <= RMS_TOL and p.max() <= PEAK_TOL, (r.max(), p.max(), int(r.argmax()))


def run_big_against_parts(torch, mem, refwrap, src, dst, L, nch, parts, lens, in_stride=None, opts=(), seed=1,
                          extra_rows=()):
    """ONE object over nch channels against objects over [lo, hi) of the same rows (whole pairs, option form_channels =
    nch: the same size-driven choices), in lockstep, call by call: every channel bit for bit, the same stage symbols;
    sampled channels of the big object against the compiled reference"""
    big = make(src, dst, L, nch, opts)
    cap = big.max_out_len
    out = torch.empty((nch, cap), dtype=torch.float64, device="cuda")
    subs = []
    sub_out = torch.empty((max(hi - lo for lo, hi in parts), cap), dtype=torch.float64, device="cuda")
    for lo, hi in parts:
        s = make(src, dst, L, hi - lo, opts)
        s.set_option("form_channels", nch)
        subs.append((lo, hi, s, sub_out[:hi - lo]))
    rows = sampled_rows(nch, cap, in_stride or L, extra_rows)
    assert len(rows) >= 64 or nch < 64
    xs, ys, counts = [], [], []
    for i, l in enumerate(lens):
        x = dev_input(torch, nch, l, seed * 1000 + i, in_stride)
        y = big.process(x, out=out)
        mem.sample()
        counts.append(y.shape[1])
        xs.append(x[rows].cpu().numpy())
        ys.append(y[rows].cpu().numpy())
        for lo, hi, s, o in subs:
            ys_ = s.process(x[lo:hi], out=o)
            assert ys_.shape[1] == y.shape[1]
            if not torch.equal(ys_, y[lo:hi]):
                d = (ys_ != y[lo:hi]).any(dim=1).nonzero()
                raise AssertionError("call %d: channels %s of [%d, %d) differ" % (i, (d[:8, 0] + lo).tolist(), lo, hi))
        del x
    syms = big.stage_symbols()
    for lo, hi, s, _ in subs:
        assert s.stage_symbols() == syms, (lo, hi, s.stage_symbols(), syms)
    assert sum(counts) > 0
    check_reference(refwrap, src, dst, L, lens, xs, ys, counts)
    return syms, [t[0] for t in big.stage_timings()]


# ------------------------------------------------------------------------------------------------------------------
# A. shards of one batch == the unsharded object, on either side of the half-array threshold

def shard_objects(total, world, make_one):
    """the per-rank objects exactly as ShardedBatchResampler builds them on ranks 0 .. world-1"""
    objs = []
    saved = sharding._rank_world
    try:
        for r in range(world):
            sharding._rank_world = lambda r=r: (r, world)
            sh = sharding.ShardedBatchResampler(make_one, total)
            objs.append((sh.lo, sh.hi, sh.local))
    finally:
        sharding._rank_world = saved
    return objs


@pytest.mark.parametrize("world", [2, 3, 4])
def test_shards_equal_the_unsharded_object(torch, mem, world):
    """cfg2 at 16384 per call: the whole batch is above the half-array threshold (mode 23), every shard alone would be
    below it; every shard's rows must be the unsharded rows bit for bit, with the unsharded stage symbols"""
    src, dst, L = CFG2[0], CFG2[1], 16384
    nmin = half_channels(src, dst, L)
    total = nmin + 50 + (nmin + 50) % 2           # above the threshold (an even count)
    shards = [sharding.channel_shard(total, r, world) for r in range(world)]
    assert all(hi - lo < nmin for lo, hi in shards), (total, shards)   # ... each shard alone below it
    lens = [L, 7777, L]

    def one(nch):
        b = r8b.BatchResampler(src, dst, L, 2.0, 180.15, nch=nch, device=0)
        b.set_option("timing", 1)
        return b

    whole = one(total)
    parts = shard_objects(total, world, one)
    assert [(lo, hi) for lo, hi, _ in parts] == shards
    for i, l in enumerate(lens):
        x = dev_input(torch, total, l, 77 + i)
        y = whole.process(x).clone()
        for lo, hi, b in parts:
            ys = b.process(x[lo:hi])
            assert ys.shape == y[lo:hi].shape
            if not torch.equal(ys, y[lo:hi]):
                d = (ys - y[lo:hi]).abs()
                ch = int(d.max(dim=1).values.argmax()) + lo
                raise AssertionError("world %d, call %d: channels [%d, %d) differ from the unsharded object; worst "
                                     "channel %d, max |diff| %.3g, rms %.3g; symbols %s vs %s"
                                     % (world, i, lo, hi, ch, float(d.max()), float((d * d).mean().sqrt()),
                                        b.stage_symbols(), whole.stage_symbols()))
        mem.sample()
    assert whole.stage_symbols()[0] == "k_convp<11, 1, 23, 24>", whole.stage_symbols()
    for lo, hi, b in parts:
        assert b.stage_symbols() == whole.stage_symbols(), (lo, hi, b.stage_symbols())


# ------------------------------------------------------------------------------------------------------------------
# B. each size-driven choice on both sides of its threshold, the other choices pinned

def straddle(torch, src, dst, maxin, counts, lens, opts, seed=3):
    """the first min(counts) channels through an object of counts[0] and of counts[1] channels: outputs of the shared
    channels (device), stage symbols and timings of both"""
    n0 = min(counts)
    res = []
    for nch in counts:
        b = make(src, dst, maxin, nch, opts)
        ys = []
        for i, l in enumerate(lens):
            x = dev_input(torch, max(counts), l, seed * 100 + i)[:nch]   # (the same rows whatever nch)
            ys.append(b.process(x)[:n0].clone())
        res.append((torch.cat(ys, dim=1), b.stage_symbols(), b.stage_timings(), b))
    return res


def test_walk_form_threshold(torch, mem):
    """WALK_CHANNELS - 2 and WALK_CHANNELS channels (cfg2, 2048 -> 4096-point pair, half-array forms pinned off): a
    workgroup per block below, the walk form from the threshold on; bitwise equal"""
    src, dst, L = CFG2[0], CFG2[1], 16384
    opts = {"half": 0, "half_fused": 0}
    (ya, sa, _, _), (yb, sb, _, b) = straddle(torch, src, dst, L, (WALK_CHANNELS - 2, WALK_CHANNELS),
                                              [L, 9000, L], opts)
    mem.sample()
    assert sa[0] == "k_convp<11, 1, 4, 24>", sa
    assert sb[0] == "k_convp_walk<11, 1, 4, 24>", sb
    assert b.stat("walk_blocks") > 0
    assert torch.equal(ya, yb)


def test_half_band_cascade_tile_threshold(torch, mem):
    """44100 -> 2822400 at 1000 samples per call (the cascade's 64 000 outputs: 8 tiles of 8192): channels x tiles one
    pair below and at HBC_TILES -- 4096-output tiles below, 8192 from the threshold on; half-array forms pinned; bitwise equal"""
    src, dst, L, l = 44100.0, 2822400.0, 1024, 1000
    # (outputs per call of the cascade's last stage: the stage timings of a small object past its start-up)
    p = make(src, dst, L, 2, {"half": 0, "half_fused": 0})
    for _ in range(4):
        p.process(dev_input(torch, 2, l, 1))
    p.stage_timings()
    p.process(dev_input(torch, 2, l, 1))
    casc = [t for t in p.stage_timings() if t[0] == "k_hbcascade" and t[2] > 0]   # (the run's row: its outputs)
    assert len(casc) == 1 and casc[0][2] == 1, p.stage_timings()
    tiles = -(-casc[0][4] // 8192)
    hi = -(-HBC_TILES // tiles)
    hi += hi % 2
    opts = {"half": 0, "half_fused": 0}
    (ya, sa, ta, a), (yb, sb, tb, b) = straddle(torch, src, dst, L, (hi - 2, hi), [l, l, l, l], opts)
    mem.sample()
    assert sa == sb and "k_hbcascade" in sa, (sa, sb)
    assert a.stat("hbc_tile_8192") == 0 and b.stat("hbc_tile_8192") > 0, (a.stat("hbc_tile_8192"), b.stat("hbc_tile_8192"))
    assert torch.equal(ya, yb)


def poly_groups_of(nch, stream_per_channel):
    """Engine::process with poly_groups = 1: the groups of a call whose convolver writes `stream_per_channel` samples
    per channel"""
    groups = math.ceil(8.0 * nch * stream_per_channel / POLY_CAP)
    while groups > 1 and nch // groups < POLY_MIN_PER:
        groups -= 1
    return groups


def poly_windows(nch, stream_per_channel):
    """launches per stage of such a call: windows of whole pairs, the last one ragged"""
    groups = poly_groups_of(nch, stream_per_channel)
    if groups <= 1:
        return 1
    per = (-(-nch // groups) + 1) & ~1
    return -(-nch // per)


def run_poly_grouped(torch, mem, nch, lens, seed, rows=None):
    """44100 -> 44101 through poly_groups = 1 and 0, call by call: the outputs (compared on the device), per call the
    launches the group formula predicts from the convolver's output count; sampled rows for the reference"""
    src, dst, L = 44100.0, 44101.0, max(lens)
    a = make(src, dst, L, nch, {"poly_groups": 1})
    b = make(src, dst, L, nch, {"poly_groups": 0})
    oa = torch.empty((nch, a.max_out_len), dtype=torch.float64, device="cuda")
    ob = torch.empty_like(oa)
    xs, ys, counts, grouped = [], [], [], 0
    for i, l in enumerate(lens):
        x = dev_input(torch, nch, l, seed + i)
        ya, yb = a.process(x, out=oa), b.process(x, out=ob)
        mem.sample()
        assert ya.shape == yb.shape and torch.equal(ya, yb), i
        ta, tb = a.stage_timings(), b.stage_timings()
        assert [t[0] for t in ta] == [t[0] for t in tb] == ["k_convp", "k_poly"], (ta, tb)
        assert a.stage_symbols() == b.stage_symbols()
        w = poly_windows(nch, tb[0][4]) if tb[0][4] > 0 and tb[1][4] > 0 else 1
        assert [t[2] for t in ta] == [w * t[2] for t in tb], (i, ta, tb, w)
        grouped += w > 1
        if rows is not None:
            xs.append(x[rows].cpu().numpy())
            ys.append(ya[rows].cpu().numpy())
        counts.append(ya.shape[1])
    return grouped, xs, ys, counts


def test_poly_channel_groups_threshold(torch, mem):
    """44100 -> 44101 at 16384 per call with the automatic cap (poly_groups = 1) against poly_groups = 0: an odd channel
    count just large enough for two groups, so the last group ends on the unpaired channel; bitwise equal, the launches
    the groups make"""
    L = 16384
    nch = 2 * POLY_MIN_PER + 1
    # (the convolver doubles the rate: ~2 L samples per channel between the stages in a whole call)
    assert poly_windows(nch, 2 * L) == 2 and poly_windows(nch - 2, 2 * L) == 1
    grouped, _, _, _ = run_poly_grouped(torch, mem, nch, [L, L, L, 5000], 500)
    assert grouped >= 2


@pytest.mark.parametrize("option,dst,sym", [("half", 88200.0, "k_convp<11, 1, 21, 24>"),
                                            ("half_fused", 96000.0, "k_convp<11, 1, 23, 24>")])
def test_half_array_threshold(torch, refwrap, mem, option, dst, sym):
    """pairs x blocks = 511 and 512: one channel pair whose largest call spans 511 and 512 blocks (MaxInLen), the calls
    themselves the same; the full-array kernel below, the half-array one at the threshold.  The two agree to rounding
    (run_half_case's bound) and each is within the tolerance of the compiled reference"""
    src = 44100.0
    b1 = r8b.BatchResampler(src, dst, 1024, 2.0, 180.15, nch=2, device=0)
    m = re.search(r"in_len=(\d+) io=(\d+)/", b1.describe())
    per = int(m.group(1)) // int(m.group(2))
    other = "half_fused" if option == "half" else "half"
    lens = [20000, 7001, 20000]
    x = make_input(2, sum(lens), 9)
    outs = []
    for blocks, want in ((HALF_WORKGROUPS - 1, None), (HALF_WORKGROUPS, sym)):
        maxin = blocks * per
        b = make(src, dst, maxin, 2, {other: 0})
        assert conv_blocks(b, maxin) == blocks
        ys, counts, pos = [], [], 0
        for l in lens:
            y = b.process(torch.from_numpy(x[:, pos:pos + l]).cuda()).cpu().numpy()
            pos += l
            ys.append(y)
            counts.append(y.shape[1])
        s = b.stage_symbols()
        if want:
            assert s[0] == want, s
        else:
            assert s[0] != sym and re.match(r"k_convp<11, 1, [0-9]+, 24>", s[0]), s
        y = np.concatenate(ys, axis=1)
        check_reference(refwrap, src, dst, maxin, lens, [x], [y], counts)
        outs.append(y)
    d = outs[0] - outs[1]
    assert outs[0].shape == outs[1].shape and outs[0].shape[1] > 1000
    assert np.sqrt((d * d).mean()) <= 2e-16 and np.abs(d).max() <= 4e-15
    mem.sample()


# ------------------------------------------------------------------------------------------------------------------
# C. large objects on one GPU

@pytest.mark.parametrize("rates", [CFG2, CFG3])
def test_8192_channels_against_1024_channel_objects(torch, refwrap, mem, rates):
    """BASELINE's cfg4 batch on one GPU (cfg2's output rows cross 2^31 bytes at ~7 500 channels): every channel bit for
    bit the channels of eight 1024-channel objects over the same rows, sampled channels against the reference"""
    nch, L = 8192, 16384
    parts = [(k * 1024, (k + 1) * 1024) for k in range(8)]
    run_big_against_parts(torch, mem, refwrap, rates[0], rates[1], L, nch, parts, [L, L, 9001], extra_rows=(8190, 8191))
    mem.report("8192 channels %s" % (rates,))


def test_16384_channels_with_padded_input_rows(torch, refwrap, mem):
    """16384 channels of cfg2 with input rows of 32768 + 8 doubles: input offsets past 2^32 bytes (and output offsets
    past 2^32); against sixteen 1024-channel objects"""
    nch, L = 16384, 16384
    parts = [(k * 1024, (k + 1) * 1024) for k in range(16)]
    run_big_against_parts(torch, mem, refwrap, CFG2[0], CFG2[1], L, nch, parts, [L, 9001], in_stride=32768 + 8)


def test_8191_channels_poly_groups_against_one_launch(torch, refwrap, mem):
    """44100 -> 44101 at 8191 channels: automatic channel groups (ragged last group ending on the unpaired channel)
    against poly_groups = 0, bit for bit; sampled channels against the reference"""
    src, dst, L, nch = 44100.0, 44101.0, 16384, 8191
    per = (-(-nch // poly_groups_of(nch, 2 * L)) + 1) & ~1
    assert poly_windows(nch, 2 * L) > 2 and nch % per != 0, per
    lens = [L, L, 6000]
    rows = sampled_rows(nch, r8b.BatchResampler(src, dst, L, 2.0, 180.15, nch=2, device=0).max_out_len, L)
    grouped, xs, ys, counts = run_poly_grouped(torch, mem, nch, lens, 900, rows)
    assert grouped >= 2
    check_reference(refwrap, src, dst, L, lens, xs, ys, counts)


def test_pcm_8192_channels_int24_in_planar_f32_out(torch, mem):
    """one PCM call at 8192 channels: interleaved packed int24 in, planar f32 out == the fp64 path on the decoded
    samples followed by the numpy codec of tests/test_pcm.py"""
    from test_pcm import make_pcm, np_decode, np_encode
    nch, L = 8192, 4096
    store, vals = make_pcm(r8b.PCM_S24, L, nch, 21)
    a = make(CFG2[0], CFG2[1], L, nch)
    b = make(CFG2[0], CFG2[1], L, nch)
    xin = torch.from_numpy(store).cuda()
    cap = a.max_out_len
    out = torch.empty((nch, cap), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    n = a.process_pcm_ptr(xin.data_ptr(), r8b.PCM_S24, True, nch, L, out.data_ptr(), r8b.PCM_F32, False, cap, stream)
    x64 = torch.from_numpy(np.ascontiguousarray(np_decode(vals, r8b.PCM_S24).T)).cuda()
    y64 = b.process(x64)
    mem.sample()
    assert n == y64.shape[1] and n > 0
    assert torch.equal(out[:, :n], y64.to(torch.float32))
    rows = [0, 1, 4095, 4096, 8190, 8191]
    assert np.array_equal(out[rows, :n].cpu().numpy(), np_encode(y64[rows].cpu().numpy(), r8b.PCM_F32))


# ------------------------------------------------------------------------------------------------------------------
# D. rows of a few channels 4 GiB apart, every kernel family

# (name, src, dst, maxin, tb, atten, options, the stage label (stage_timings) that must have run)
FAR_TOPOLOGIES = [
    ("pair", 44100.0, 96000.0, 4096, 2.0, 180.15, {}, "k_convp_whole"),
    ("one-channel", 96000.0, 44100.0, 8192, 0.5, 180.15, {}, "k_convp_whole"),
    ("convx", 44100.0, 96000.0, 4096, 2.0, 180.15, {"pair_conv": 0}, "k_convx_whole"),
    ("conv", 44100.0, 96000.0, 4096, 2.0, 180.15, {"fuse": 0, "fast_conv": 0}, "k_conv"),
    ("conv_big", 32000.0, 48000.0, 2048, 0.5, 180.15, {}, "k_conv"),
    ("whole", 44100.0, 96000.0, 4096, 2.0, 180.15, {"fuse": 0}, "k_whole"),
    ("poly_tiled", 44100.0, 44101.0, 1024, 2.0, 180.15, {}, "k_poly"),
    ("hbup", 44100.0, 2822400.0, 1024, 2.0, 180.15, {"fuse_hb": 0}, "k_hbup"),
    ("hbcascade", 44100.0, 2822400.0, 1024, 2.0, 180.15, {}, "k_hbcascade"),
    ("hbdown", 2822400.0, 176400.0, 4096, 2.0, 180.15, {"fuse_hbd": 0}, "k_hbdown"),
    ("hbdcascade", 2822400.0, 176400.0, 4096, 2.0, 180.15, {"fuse_hbd": 1}, "k_hbdcascade"),
    ("tail", 96000.0, 44100.0, 4096, 2.0, 180.15, {"fold_tail": 0}, "k_convp_whole"),
]
FAR_NCH = 5
GUARD = 64
GUARD_VALUE = -7.25


@pytest.fixture(scope="module")
def far_rows(torch):
    """two buffers of FAR_NCH rows of 2^27 + 1 doubles (5 GiB each), allocated once; nothing but the guards and the
    rows' used parts is ever written"""
    S = (1 << 27) + 1
    a = torch.empty(FAR_NCH * S + GUARD, dtype=torch.float64, device="cuda")
    b = torch.empty(FAR_NCH * S + GUARD, dtype=torch.float64, device="cuda")
    yield a, b
    del a, b
    torch.cuda.empty_cache()


def _guards(buf, stride, nch, n):
    """views of the GUARD elements before and after the first n elements of every row"""
    g = []
    for c in range(nch):
        s = c * stride
        if s >= GUARD:
            g.append(buf[s - GUARD:s])
        g.append(buf[s + n:s + n + GUARD])
    return g


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("topo", FAR_TOPOLOGIES, ids=[t[0] for t in FAR_TOPOLOGIES])
def test_far_rows_every_kernel_family(torch, far_rows, topo, odd):
    """rows 2^27 (+ 1) doubles apart -- the last starts past 4 GiB -- against compact rows bit for bit; the doubles just
    before and after every written output row untouched, parked and tail paths included"""
    name, src, dst, maxin, tb, att, opts, label = topo
    stride = (1 << 27) + (1 if odd else 0)
    big_in, big_out = far_rows
    nch = FAR_NCH
    a = make(src, dst, maxin, nch, opts, tb, att)
    b = make(src, dst, maxin, nch, opts, tb, att)
    lens = [maxin, maxin // 3 + 1, maxin, 1, maxin - 5, maxin]
    cap = a.max_out_len
    xin = big_in[:nch * stride].view(nch, stride)
    yout = big_out[:nch * stride].view(nch, stride)
    tails0 = b.stat("tail_launches")
    for i, l in enumerate(lens):
        x = dev_input(torch, nch, l, 4000 + i)
        want = a.process(x).clone()
        xin[:, :l].copy_(x)
        for g in _guards(big_out, stride, nch, cap):
            g.fill_(GUARD_VALUE)
        stream = torch.cuda.current_stream().cuda_stream
        n = b.process_ptr(xin.data_ptr(), stride, l, yout.data_ptr(), stride, stream)
        assert n == want.shape[1]
        assert torch.equal(yout[:, :n], want), (name, i)
        for g in _guards(big_out, stride, nch, cap):
            assert bool((g == GUARD_VALUE).all()), (name, i)
        # (between n and cap: nothing of this call's output; the engine may park what it computed ahead elsewhere)
    assert label in [t[0] for t in b.stage_timings()], b.stage_timings()
    if name == "tail":
        assert b.stat("tail_launches") > tails0


@pytest.mark.parametrize("odd", [False, True])
def test_far_rows_planar_pcm(torch, far_rows, odd):
    """planar int16 in and out with rows 2^29 (+ 1) samples apart (the last starts past 4 GiB): equal to compact rows
    bit for bit, guards untouched"""
    nch, L = FAR_NCH, 4096
    stride = (1 << 29) + (1 if odd else 0)
    big_in, big_out = far_rows
    xin = big_in.view(torch.int16)[:nch * stride].view(nch, stride)
    yout = big_out.view(torch.int16)
    a = make(CFG2[0], CFG2[1], L, nch)
    b = make(CFG2[0], CFG2[1], L, nch)
    g = torch.Generator(device="cuda")
    g.manual_seed(8)
    for i, l in enumerate([L, 1000, L, 17]):
        x = torch.randint(-32768, 32768, (nch, l), generator=g, dtype=torch.int16, device="cuda")
        want = a.process_pcm(x.contiguous(), planar=True).clone()
        xin[:, :l].copy_(x)
        for gv in _guards(yout, stride, nch, a.max_out_len):
            gv.fill_(-12345)
        stream = torch.cuda.current_stream().cuda_stream
        n = b.process_pcm_ptr(xin.data_ptr(), r8b.PCM_S16, False, stride, l, yout.data_ptr(), r8b.PCM_S16, False,
                              stride, stream)
        assert n == want.shape[1]
        assert torch.equal(yout[:nch * stride].view(nch, stride)[:, :n], want), i
        for gv in _guards(yout, stride, nch, a.max_out_len):
            assert bool((gv == -12345).all()), i


# ------------------------------------------------------------------------------------------------------------------
# E. the grid's y limit

@pytest.mark.parametrize("rates,label", [(CFG2, "k_convp_whole"), ((44100.0, 2822400.0), "k_hbcascade")])
def test_65535_channels(torch, refwrap, mem, rates, label):
    """the largest object there is, 128 samples per call: the last channel (65534) has no partner at the highest grid
    y index; bitwise against smaller objects with the same size-driven choices (form_channels), sampled channels
    against the reference"""
    nch, L = 65535, 128
    per = 8192
    parts = [(lo, min(nch, lo + per)) for lo in range(0, nch, per)]
    lens = [L] * 23 + [77] + [L] * 8
    src, dst = rates
    syms, labels = run_big_against_parts(torch, mem, refwrap, src, dst, L, nch, parts, lens,
                                         extra_rows=(32766, 32767, 65533, 65534))
    assert label in labels, (labels, syms)
    mem.report("65535 channels %s" % (rates,))


def test_65536_channels_refused(torch):
    lib = r8b.load()
    assert not lib.r8b_batch_create(44100.0, 96000.0, 128, 2.0, 180.15, 65536, 0)
    assert "65535" in lib.r8b_last_error().decode()
