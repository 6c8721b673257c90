"""The one-byte formats of the PCM boundary: R8B_PCM_U8, R8B_PCM_ULAW, R8B_PCM_ALAW (include/r8bsrc.h; codec:
r8b_pcm_codec.h "boundary codec"; the one-byte row form: r8b_pcm.h; Python: in_format=).

Every check runs on two tiers, as tests/test_clip_packed.py's do: the host emulation (numpy buffers as "device"
pointers) and the product on the GPU (torch tensors).  Every comparison is bitwise; nothing here has a tolerance.  The
G.711 tables are those of tests/golden/g711.npz (tests/golden/make_g711.py), the rest of the specification is restated
in numpy in tests/pcm8_cases.py.

  1  the codec, exhaustively, through a pass-through object (48000 -> 48000: a call is ingest and egress alone)
  2  the alignment sweep of the one-byte row form: packed clips a guard byte apart, the first base at 0 .. 15
  3  equivalence with the S16 path through a real chain (8000 -> 16000), one case per entry and form
  4  dither (U8 alone) and chunk invariance
  5  the Python entries"""
import importlib
import os

import numpy as np
import pytest

import cases
import pcm8_cases as E
from pcm8_cases import ALAW, F32, F64, PCM8, S16, SENTINEL, U8, ULAW, Tier

r8b = importlib.import_module("r8brain-free-src_amd")


@pytest.fixture(scope="module")
def emul():
    return cases.emul_lib()


def fmt_id(f):
    return E.NAME[f]


# ---------------------------------------------------------------- 1. the codec, exhaustively
FORMS = [(1, False), (3, True)]       # (channels, interleaved): planar rows and interleaved tiles


def convert(tier, x, in_fmt, out_fmt, nch, il):
    """the samples x (1-D, the input format's dtype) through ONE process_pcm call of a pass-through object with nch
    channels, in the buffer's element order; -> the output buffer's elements, as many"""
    n = len(x)
    frames = -(-n // nch)
    xp = np.concatenate([x, np.repeat(x[:1], frames * nch - n)])
    a = tier.make(nch, 48000.0, 48000.0, frames)
    xin, out = tier.buf(xp), tier.sentinels(frames * nch * E.BYTES[out_fmt])
    stride = nch if il else frames
    assert a.process_pcm_ptr(tier.ptr(xin), in_fmt, il, stride, frames, tier.ptr(out), out_fmt, il, stride) == frames
    return tier.host(out).copy().view(E.NP_DTYPE[out_fmt])[:n]


U8_EDGES = np.array([0.5 / 128, -0.5 / 128, 1.5 / 128, 2.5 / 128, 1.0, -1.0, 2.0, -3.0, np.nan, np.inf, -np.inf,
                     127.5 / 128, 126.5 / 128, -127.5 / 128, -128.5 / 128, 0.0, -0.0])


def check_codec(tier):
    all_codes = np.arange(256, dtype=np.uint8)
    grid = np.arange(-32768, 32768, dtype=np.float64) / 32768.0
    for nch, il in FORMS:
        for fmt in PCM8:
            got = convert(tier, all_codes, fmt, F64, nch, il)
            want = (all_codes.astype(np.float64) - 128.0) / 128.0 if fmt == U8 else E.DECODE[fmt] / 32768.0
            assert np.array_equal(got, want), ("decode", fmt, nch, il)
            # ... and back: the identity, but for mu-law's negative zero
            assert np.array_equal(convert(tier, all_codes, fmt, fmt, nch, il), E.round_trip(all_codes, fmt)), (fmt, nch, il)
        for fmt in (ULAW, ALAW):
            got = convert(tier, grid, F64, fmt, nch, il)
            assert np.array_equal(got, E.ENCODE[fmt]), ("encode", fmt, nch, il, int(np.flatnonzero(got != E.ENCODE[fmt])[0]))
        got = convert(tier, U8_EDGES, F64, U8, nch, il)
        want = np.array([128, 128, 130, 130, 255, 0, 255, 0, 128, 255, 0, 255, 254, 0, 0, 128, 128], dtype=np.uint8)
        assert np.array_equal(E.encode(U8_EDGES, U8)[0], want)       # (the restatement says what the header says)
        assert np.array_equal(got, want), ("U8 edges", nch, il, got)
    lib = tier.abi()
    assert [lib.r8b_pcm_sample_bytes(f) for f in PCM8] == [1, 1, 1]
    assert [lib.r8b_pcm_sample_bytes(f) for f in (5, 9, 15, 19, -1, 255)] == [0] * 6
    assert [lib.r8b_pcm_sample_bytes(f) for f in range(5)] == [8, 4, 2, 3, 4]


def test_codec_emulated(emul):
    check_codec(Tier(emul))


@pytest.mark.gpu
def test_codec_gpu():
    check_codec(Tier(None))


def check_refusals(tier):
    """5, 9 and 19 name no format: every entry refuses them on either side with the message of old, and writes nothing"""
    a = tier.make(2, 48000.0, 48000.0, 64)
    xin, out = tier.buf(np.zeros(1024, dtype=np.uint8)), tier.sentinels(1024)
    pi, po, n1, n2 = tier.ptr(xin), tier.ptr(out), [16], [16, 16]
    for bad in (5, 9, 19):
        for fi, fo in ((bad, U8), (ULAW, bad)):
            calls = [
                lambda: a.process_pcm_ptr(pi, fi, True, 2, 16, po, fo, True, 2),
                lambda: a.process_pcm_ptr(pi, fi, False, 16, 16, po, fo, False, 16),
                lambda: a.resample_clips_ptr(pi, fi, 16, n2, po, fo, 16, n2),
                lambda: a.resample_clips_ex_ptr(2, pi, fi, True, 32, n1, po, fo, False, 16, n1),
                lambda: a.resample_clips_mix_ptr(1, 2, [[1.0], [1.0]], pi, fi, False, 16, n1, po, fo, True, 32, n1),
                lambda: a.resample_clips_packed_ptr(0, 1, None, pi, fi, False, 0, [0, 16], n2, po, fo, False, 0, [0, 16], n2),
                lambda: a.resample_clips_sched_ptr(0, 1, None, pi, fi, False, 16, None, n2, po, fo, False, 16, None, n2, 3),
            ]
            for j, call in enumerate(calls):
                with pytest.raises(RuntimeError, match="unknown PCM sample format"):
                    call()
                assert np.all(tier.host(out) == SENTINEL), (bad, j)
    # ... none of which used the object up
    assert a.resample_clips_ptr(pi, U8, 16, n2, po, ALAW, 16, n2) == 16


def test_refusals_emulated(emul):
    check_refusals(Tier(emul))


@pytest.mark.gpu
def test_refusals_gpu():
    check_refusals(Tier(None))


# ---------------------------------------------------------------- 2. the alignment sweep of the row form
# Fourteen one-channel clips packed a guard byte apart, the first at byte 0 .. 15 of its buffer, through a pass-through
# object with MaxInLen 1001: a clip's base + the step's first frame is at every residue mod 8, the clip's end (the
# valid / padding split of its last chunk) falls anywhere in a lane's group, and clips shorter than a group are head
# and tail alone.  The input's gaps hold the format's largest code and its last clip ends with the allocation; the
# output's guard bytes and surroundings must keep their sentinel.
SWEEP_LEN = [0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 2047, 2048, 2049, 2057]
SWEEP_CHUNK = 1001
SWEEP_VARIANTS = ["packed", "strided", "packed_sched", "strided_sched"]


def check_alignment(tier, fmt, variant):
    n, lens, Pmax = len(SWEEP_LEN), SWEEP_LEN, max(SWEEP_LEN)
    b = E.codes(n, Pmax, lens, fmt, 8 + fmt)
    assert all(np.any(b == c) for c in (0x7F, 0xFF, 0x00, 0x80))
    a = tier.make(n, 48000.0, 48000.0, SWEEP_CHUNK)
    flags = 3 if variant.endswith("sched") else 0
    stride = Pmax + 5
    for first in range(16):
        off, pos = [], first
        for m in lens:
            off.append(pos)
            pos += m + 1                 # (the guard byte)
        end = pos - 1                    # the last clip's end: the input ends here
        xb = np.full(end, E.LARGEST[fmt], dtype=np.uint8)
        for i, m in enumerate(lens):
            xb[off[i]:off[i] + m] = b[i, :m]
        if variant.startswith("packed"):
            want = np.full(end + 16, SENTINEL, dtype=np.uint8)
            for i, m in enumerate(lens):
                want[off[i]:off[i] + m] = E.round_trip(b[i, :m], fmt)
            out_off, out_stride, shift = off, 0, 0
        else:
            # rows of P + 5 bytes from byte `first` on: the clip, encoded zeros up to P, nothing at or past P
            rows = np.full((n, stride), SENTINEL, dtype=np.uint8)
            rows[:, :Pmax] = E.ZERO[fmt]
            for i, m in enumerate(lens):
                rows[i, :m] = E.round_trip(b[i, :m], fmt)
            want = np.concatenate([np.full(first, SENTINEL, dtype=np.uint8), rows.reshape(-1), np.full(16, SENTINEL, dtype=np.uint8)])
            out_off, out_stride, shift = None, stride, first
        xin, out = tier.buf(xb), tier.sentinels(want.size)
        p = a.resample_clips_sched_ptr(0, 1, None, tier.ptr(xin), fmt, False, 0, off, lens, tier.ptr(out[shift:]), fmt, False,
                                       out_stride, out_off, lens, flags)
        assert p == Pmax
        E.assert_same(tier.host(out), want, (variant, "first base", first))


@pytest.mark.parametrize("variant", SWEEP_VARIANTS)
@pytest.mark.parametrize("fmt", PCM8, ids=fmt_id)
def test_row_alignment_emulated(emul, fmt, variant):
    check_alignment(Tier(emul), fmt, variant)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", SWEEP_VARIANTS)
@pytest.mark.parametrize("fmt", PCM8, ids=fmt_id)
def test_row_alignment_gpu(fmt, variant):
    check_alignment(Tier(None), fmt, variant)


# ---------------------------------------------------------------- 3. equivalence with the S16 path, through a chain
# 8000 -> 16000 (ReqTransBand 2.0, 136.45 dB, MaxInLen 1000), six clips chosen as tests/test_clips.py chooses its own:
# empty, one sample, one short of a step, a step, mid-step, one past a step's edge.
#   ingest   a call fed the codes gives byte for byte the output of the same call fed the S16 samples T[b] (U8:
#            (b - 128) << 8)
#   egress   a G.711 output is the fixture's compression of the same call's (undithered) S16 output, padding included,
#            and the meters are that call's; a U8 output and its meters are the numpy restatement on the call's F64 output
SRC3, DST3, CHUNK3 = 8000.0, 16000.0, 1000
IN_LEN3 = [0, 1, 999, 1000, 2500, 2001]
NCLIPS3, T3 = 6, 2512
CLIP_CASES = {
    "clips_rows": dict(K=1, Kin=1, M=None, il=(False, False), packed=(False, False), flags=0, out=F64),
    "ex_tiles_to_rows": dict(K=2, Kin=2, M=None, il=(True, False), packed=(False, False), flags=0, out=F64),
    "mix_stereo_to_f32": dict(K=1, Kin=2, M=[[.5, .5]], il=(True, False), packed=(False, False), flags=0, out=F32),
    "packed_both": dict(K=2, Kin=2, M=None, il=(True, True), packed=(True, True), flags=0, out=F64),
    "sched_both_flags": dict(K=1, Kin=1, M=None, il=(False, False), packed=(False, False), flags=3, out=F64),
}


def out_len3(tier):
    nat = tier.out_len(IN_LEN3, SRC3, DST3)
    nat[IN_LEN3.index(2500)] -= 100      # cut short
    nat[IN_LEN3.index(1000)] += 1500     # the filter's tail, then zeros
    return nat


def run_clip_case(tier, name, units, in_fmt, out_fmt, out_len, meters=False):
    """-> (the output buffer's elements, the mask of those the call writes, the meters or None, the output's Layout)"""
    c = CLIP_CASES[name]
    K, Kin, M = c["K"], c["Kin"], c["M"]
    a = tier.make(NCLIPS3 * K, SRC3, DST3, CHUNK3, meters=meters)
    lin, lout = E.Layout(Kin, c["il"][0], c["packed"][0]), E.Layout(K, c["il"][1], c["packed"][1])
    xb, in_stride, in_off = lin.lay_in(units, IN_LEN3)
    total, out_stride, out_off, mask = lout.out_shape(out_len)
    xin, out = tier.buf(xb), tier.sentinels(total * E.BYTES[out_fmt])
    pi, po = tier.ptr(xin), tier.ptr(out)
    if name == "clips_rows":
        p = a.resample_clips_ptr(pi, in_fmt, in_stride, IN_LEN3, po, out_fmt, out_stride, out_len)
    elif name == "ex_tiles_to_rows":
        p = a.resample_clips_ex_ptr(K, pi, in_fmt, lin.il, in_stride, IN_LEN3, po, out_fmt, lout.il, out_stride, out_len)
    elif name == "mix_stereo_to_f32":
        p = a.resample_clips_mix_ptr(Kin, K, M, pi, in_fmt, lin.il, in_stride, IN_LEN3, po, out_fmt, lout.il, out_stride, out_len)
    elif name == "packed_both":
        p = a.resample_clips_packed_ptr(0, K, None, pi, in_fmt, lin.il, in_stride, in_off, IN_LEN3, po, out_fmt, lout.il,
                                        out_stride, out_off, out_len)
    else:
        p = a.resample_clips_sched_ptr(0, K, None, pi, in_fmt, lin.il, in_stride, in_off, IN_LEN3, po, out_fmt, lout.il,
                                       out_stride, out_off, out_len, c["flags"])
    assert p == max(out_len)
    elems = tier.host(out).copy().view(E.NP_DTYPE[out_fmt])
    return elems, mask, (a.read_meters() if meters else None), lout


def check_clip_case(tier, name, fmt):
    c = CLIP_CASES[name]
    out_len = out_len3(tier)
    b = E.codes(NCLIPS3 * c["Kin"], T3, E.F.rows_of(IN_LEN3, c["Kin"]), fmt, 30 + fmt)
    codes_in, s16_in = E.units_of(b, fmt, False), E.units_of(b, fmt, True)
    # ingest
    got, mask, _, lout = run_clip_case(tier, name, codes_in, fmt, c["out"], out_len)
    ref, _, _, _ = run_clip_case(tier, name, s16_in, S16, c["out"], out_len)
    E.assert_same(got.view(np.uint8), ref.view(np.uint8), (name, "ingest"))
    assert np.count_nonzero(got[mask]) > 1000 and np.all(np.isfinite(got[mask]))
    # egress
    enc, mask, m, _ = run_clip_case(tier, name, codes_in, fmt, fmt, out_len, meters=True)
    if fmt == U8:
        v = got if c["out"] == F64 else run_clip_case(tier, name, codes_in, fmt, F64, out_len)[0]
        want = np.where(mask, E.encode(v, U8)[0], np.uint8(SENTINEL))
        want_m = E.meters_of(lout.rows(v, out_len, 0.0), E.F.rows_of(out_len, c["K"]))
    else:
        lin16, _, want_m, _ = run_clip_case(tier, name, s16_in, S16, S16, out_len, meters=True)
        want = np.where(mask, E.compress(lin16, fmt), np.uint8(SENTINEL))
    E.assert_same(enc, want, (name, "egress"))
    E.assert_meters(m, want_m, name)
    assert want_m["peak"].max() > 0.5
    # (the padding behind a short clip is the format's encoded zero)
    rows = lout.rows(enc, out_len, E.ZERO[fmt])
    assert np.all(rows[0] == E.ZERO[fmt]) and np.all(rows[c["K"], out_len[1]:] == E.ZERO[fmt])


@pytest.mark.parametrize("fmt", PCM8, ids=fmt_id)
@pytest.mark.parametrize("name", sorted(CLIP_CASES))
def test_clip_entries_emulated(emul, name, fmt):
    check_clip_case(Tier(emul), name, fmt)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", PCM8, ids=fmt_id)
@pytest.mark.parametrize("name", sorted(CLIP_CASES))
def test_clip_entries_gpu(name, fmt):
    check_clip_case(Tier(None), name, fmt)


NCH3, FRAMES3 = 6, 3000


def run_stream(tier, rows, in_fmt, out_fmt, il, meters=False, dither=None, chunk=CHUNK3, rates=(SRC3, DST3)):
    """rows [nch, frames] of the input format's dtype through process_pcm in calls of `chunk` frames -> (output rows
    [nch, n], meters or None, the object's pcm_staged_sides)"""
    nch, frames = rows.shape
    a = tier.make(nch, rates[0], rates[1], CHUNK3, dither=dither, meters=meters)
    cap, B = max(a.max_out_len, 1), E.BYTES[out_fmt]
    parts = []
    for f in range(0, frames, chunk):
        blk = rows[:, f:f + chunk]
        l = blk.shape[1]
        xin = tier.buf(np.ascontiguousarray(blk.T if il else blk))
        out = tier.sentinels(nch * cap * B)
        n = a.process_pcm_ptr(tier.ptr(xin), in_fmt, il, nch if il else l, l, tier.ptr(out), out_fmt, il, nch if il else cap)
        raw = tier.host(out).copy()
        assert np.all((raw[n * nch * B:] if il else raw.reshape(nch, cap * B)[:, n * B:]) == SENTINEL)
        e = raw.view(E.NP_DTYPE[out_fmt])
        parts.append(e[:n * nch].reshape(n, nch).T if il else e.reshape(nch, cap)[:, :n])
    return np.ascontiguousarray(np.concatenate(parts, axis=1)), (a.read_meters() if meters else None), a.stat("pcm_staged_sides")


def check_stream(tier, fmt, il):
    b = E.codes(NCH3, FRAMES3, [FRAMES3] * NCH3, fmt, 50 + fmt)
    s16 = E.linear(b, fmt).astype(np.int16)
    got, _, _ = run_stream(tier, b, fmt, F64, il)
    ref, _, _ = run_stream(tier, s16, S16, F64, il)
    E.assert_same(got.view(np.uint8), ref.view(np.uint8), "ingest")
    # (the stream is no silence; 8000 -> 16000 doubles the frames, less the chain's latency)
    assert got.shape[1] > FRAMES3 // 2 and np.count_nonzero(got) > NCH3 * FRAMES3 // 2
    enc, m, staged = run_stream(tier, b, fmt, fmt, il, meters=True)
    if fmt == U8:
        want, want_m = E.encode(got, U8)[0], E.meters_of(got, [got.shape[1]] * NCH3)
    else:
        lin16, want_m, _ = run_stream(tier, s16, S16, S16, il, meters=True)
        want = E.compress(lin16, fmt)
    E.assert_same(enc, want, "egress")
    E.assert_meters(m, want_m, "stream")
    # a one-byte side always takes the staging rows: both planar sides of every call are counted
    assert staged == (0 if il else 2 * (FRAMES3 // CHUNK3))
    if not il:
        assert run_stream(tier, b, fmt, fmt, il)[2] == 2 * (FRAMES3 // CHUNK3)      # (... without meters too)


@pytest.mark.parametrize("il", [True, False], ids=["interleaved", "planar"])
@pytest.mark.parametrize("fmt", PCM8, ids=fmt_id)
def test_process_pcm_emulated(emul, fmt, il):
    check_stream(Tier(emul), fmt, il)


@pytest.mark.gpu
@pytest.mark.parametrize("il", [True, False], ids=["interleaved", "planar"])
@pytest.mark.parametrize("fmt", PCM8, ids=fmt_id)
def test_process_pcm_gpu(fmt, il):
    check_stream(Tier(None), fmt, il)


# ---------------------------------------------------------------- 4. dither and chunk invariance
def check_dither(tier, il):
    """a pass-through object: the fp64 values at the egress are the input's, so the header's formula is restated on them"""
    nch, frames, first = 3, 3000, 5
    rng = np.random.RandomState(77)
    v = rng.uniform(-1.02, 1.02, size=(nch, frames))
    v[1, 100], v[2, 2999] = np.nan, np.inf
    same = (48000.0, 48000.0)
    d = E.np_dither(E.SEED, first, nch, 0, frames)
    want, clipped = E.encode(v, U8, d)
    assert np.count_nonzero(want != E.encode(v, U8)[0]) > frames // 2 and clipped.sum() > 10
    got, m, _ = run_stream(tier, v, F64, U8, il, meters=True, dither=first, rates=same)
    E.assert_same(got, want, "dithered U8")
    assert np.array_equal(m["clipped"], clipped.sum(axis=1)) and m["nonfinite"].tolist() == [0, 1, 1]
    # the same stream cut another way
    E.assert_same(run_stream(tier, v, F64, U8, il, dither=first, chunk=333, rates=same)[0], want, "calls of 333")
    # G.711 ignores it
    for fmt in (ULAW, ALAW):
        plain = E.encode(v, fmt)[0]
        E.assert_same(run_stream(tier, v, F64, fmt, il, dither=first, rates=same)[0], plain, ("dither on", fmt))
        E.assert_same(run_stream(tier, v, F64, fmt, il, rates=same)[0], plain, ("dither off", fmt))
    # silence
    got = run_stream(tier, np.zeros((nch, frames)), F64, U8, il, dither=first, rates=same)[0]
    E.assert_same(got, (np.rint(d) + 128).astype(np.uint8), "silence")
    assert set(np.unique(got)) == {127, 128, 129}


@pytest.mark.parametrize("il", [True, False], ids=["interleaved", "planar"])
def test_dither_emulated(emul, il):
    check_dither(Tier(emul), il)


@pytest.mark.gpu
@pytest.mark.parametrize("il", [True, False], ids=["interleaved", "planar"])
def test_dither_gpu(il):
    check_dither(Tier(None), il)


# ---------------------------------------------------------------- 5. the Python entries
@pytest.mark.gpu
def test_python_entries_gpu():
    import torch
    tier = Tier(None)
    nch, frames = 4, 3 * CHUNK3          # (one call long enough to outlast the chain's latency)
    b = E.codes(nch, frames, [frames] * nch, ULAW, 91)
    a = tier.make(nch, SRC3, DST3, frames)
    # mu-law interleaved in, F32 out: bit for bit the call fed the S16 samples of the same values
    x = torch.from_numpy(np.ascontiguousarray(b.T)).cuda()                       # [frames, nch] uint8
    y = a.process_pcm(x, in_format=r8b.PCM_ULAW, out_format=r8b.PCM_F32)
    assert y.dtype == torch.float32 and y.dim() == 2 and y.shape[1] == nch and y.shape[0] > 1000
    ref = tier.make(nch, SRC3, DST3, frames).process_pcm(torch.from_numpy(np.ascontiguousarray(E.linear(b, ULAW).astype(np.int16).T)).cuda(),
                                                        out_format=r8b.PCM_F32)
    assert torch.equal(y, ref)
    # an 8-bit output has no trailing axis; planar
    a.clear()
    z = a.process_pcm(torch.from_numpy(b).cuda(), in_format=r8b.PCM_ULAW, out_format=r8b.PCM_ALAW, planar=True)
    assert z.dtype == torch.uint8 and z.dim() == 2 and z.shape[0] == nch and z.shape[1] == y.shape[0]
    # a bare 2-D uint8 tensor names no format
    for planar in (False, True):
        with pytest.raises(ValueError, match="in_format"):
            a.process_pcm(x if not planar else torch.from_numpy(b).cuda(), planar=planar)
    with pytest.raises(ValueError, match="in_format"):
        a.process_pcm(x.to(torch.int16), in_format=r8b.PCM_U8)
    # clips
    a.clear()
    lengths = [0, 1, 999, 1000]
    u = E.codes(nch, frames, lengths, U8, 92)
    out, ol = a.resample_clips(torch.from_numpy(u).cuda(), lengths, in_format=r8b.PCM_U8)
    assert ol == tier.out_len(lengths, SRC3, DST3) and out.dtype == torch.uint8 and tuple(out.shape) == (nch, max(ol))
    want, _ = a.resample_clips(torch.from_numpy(((u.astype(np.int16) - 128) * 256).astype(np.int16)).cuda(), lengths,
                               out_format=r8b.PCM_U8)
    assert want.dtype == torch.uint8 and torch.equal(out, want)
    assert bool((out[0] == 0x80).all())
    with pytest.raises(ValueError, match="in_format"):
        a.resample_clips(torch.from_numpy(u).cuda(), lengths)
    # packed
    flat = torch.from_numpy(np.concatenate([u[i, :n] for i, n in enumerate(lengths)])).cuda()
    res, off, ol2 = a.resample_clips_packed(flat, lengths, in_format=r8b.PCM_U8, out_format=r8b.PCM_F32)
    assert ol2 == ol and res.dtype == torch.float32 and tuple(res.shape) == (sum(ol),)
    res8, off8, _ = a.resample_clips_packed(flat, lengths, in_format=r8b.PCM_U8)
    assert res8.dtype == torch.uint8 and tuple(res8.shape) == (sum(ol),) and off8 == off
    torch.cuda.synchronize()
    for i, n in enumerate(ol):
        assert torch.equal(res8[off[i]:off[i] + n], out[i, :n]), i
    with pytest.raises(ValueError, match="in_format"):
        a.resample_clips_packed(flat, lengths)


def test_python_format_constants():
    assert (r8b.PCM_U8, r8b.PCM_ULAW, r8b.PCM_ALAW) == (16, 17, 18)
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "r8bsrc.h")).read()
    for name, value in (("U8", 16), ("ULAW", 17), ("ALAW", 18)):
        assert "R8B_PCM_%s = %d" % (name, value) in header
