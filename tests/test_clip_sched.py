"""Finished clips leave the later steps, and clips ride longest first (include/r8bsrc.h r8b_batch_resample_clips_sched,
r8b_clip_schedule, enum r8b_clip_flags; kernels: r8b_clip_sched.h; Python: BatchResampler.resample_clips_sched_ptr,
clip_schedule, and the keywords drop_finished / longest_first of resample_clips / resample_clips_packed).

Every check runs on two tiers, as in tests/test_clip_packed.py whose helpers and setup these are: the host emulation
(tests/emul/Makefile; numpy buffers as "device" pointers) and the product on the GPU (torch tensors).  44100 ->
48000 at 136.45 dB, MaxInLen 2000 (a step makes about 2177 outputs), six clips of K channels with lengths from {0, 1,
1999, 2000, 4500, 6001}, one clip cut short and one running 3000 frames past its natural end (out_lens), garbage past
each clip's end, a sentinel in every output byte.

The expectation of every byte check is the EXISTING call on a second object and has no tolerance:
  DROP_FINISHED alone   the plain strided call (which tests/test_clip_packed.py shows to be the flags == 0 call byte for
                        byte) -- the whole output buffer in each layout and addressing, and the meters;
  LONGEST_FIRST         the plain strided call GIVEN the clips in r8b_clip_schedule's order, its rows and meters taken
                        back to the caller's order -- again the whole buffer, padding and sentinels included.
Dither under LONGEST_FIRST is checked on a Src == Dst object against its own flags == 0 call: there the samples do not
depend on the pair partner and the keys go by the caller's channel, so every byte and meter must match."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import test_clip_frames as F
import test_clip_packed as P
import cases
from conftest import ROOT

r8b = importlib.import_module("r8brain-free-src_amd")

T, SLACK, SENTINEL, BYTES, CHUNK = F.T, F.SLACK, F.SENTINEL, F.BYTES, F.CHUNK
F64, F32, S16, S24, S32 = r8b.PCM_F64, r8b.PCM_F32, r8b.PCM_S16, r8b.PCM_S24, r8b.PCM_S32
DROP, ORDER = 1, 2
NCLIPS = P.NCLIPS
# the longest clips first (everything can drop), scattered, and ascending (the longest last: nothing can drop)
LENGTH_ORDERS = {"descending": [6001, 4500, 2000, 1999, 1, 0], "scattered": [6001, 0, 4500, 1, 1999, 2000],
                 "ascending": [0, 1, 1999, 2000, 4500, 6001]}
ALL_LAYOUTS = P.ALL_LAYOUTS
BOTH_ADDRESSINGS = [(True, True), (False, False)]      # (input packed, output packed)


def test_header_and_python_agree():
    """the enum's values as the Python layer has them, and the two entries in the product library"""
    assert (r8b.CLIPS_DROP_FINISHED, r8b.CLIPS_LONGEST_FIRST) == (DROP, ORDER)
    text = open(os.path.join(ROOT, "include", "r8bsrc.h")).read()
    assert "R8B_CLIPS_DROP_FINISHED = 1, R8B_CLIPS_LONGEST_FIRST = 2" in text
    lib = r8b.load()
    assert lib.r8b_batch_resample_clips_sched and lib.r8b_clip_schedule


@pytest.fixture(scope="module")
def emul():
    return cases.emul_lib()


class Tier(P.Tier):
    """tests/test_clip_packed.py's tiers with the scheduled entry"""

    def make(self, nch, src=F.SRC, dst=F.DST, dither=None, meters=False, opts=()):
        a = super().make(nch, src, dst, dither, meters)
        for name, value in opts:
            a.set_option(name, value)
        return a

    def raw_sched(self, a, Kin, K, mix, xin, in_fmt, in_il, in_stride, in_off, in_len, out, out_fmt, out_il, out_stride,
                  out_off, out_len, flags, stream=0):
        """the C entry as it is: its return value.  mix / in_off / out_off: sequences, or None for a NULL pointer"""
        def ll(v):
            return None if v is None else (C.c_longlong * len(v))(*v)
        m = None if mix is None else (C.c_double * len(mix))(*mix)
        return a._lib.r8b_batch_resample_clips_sched(
            a._h, Kin, K, m, C.c_void_p(self.ptr(xin)), in_fmt, int(in_il), in_stride, ll(in_off), ll(in_len),
            C.c_void_p(self.ptr(out)), out_fmt, int(out_il), out_stride, ll(out_off), ll(out_len), flags, C.c_void_p(stream))


def schedule(lib, out_len, flags):
    n = len(out_len)
    order = (C.c_int * max(n, 1))(*([-7] * max(n, 1)))
    rc = lib.r8b_clip_schedule(n, (C.c_longlong * max(n, 1))(*out_len), flags, order)
    return rc, [order[i] for i in range(n)]


def stable_order(out_len, flags):
    """the header's rule in Python: by output length descending, ties by ascending index"""
    if not flags & ORDER:
        return list(range(len(out_len)))
    return sorted(range(len(out_len)), key=lambda i: -out_len[i])     # (sorted() is stable)


def rows_in_order(order, K):
    return [i * K + k for i in order for k in range(K)]


# ---------------------------------------------------------------- the existing call, once per case
_REF = {}


def reference(tier, K, M, x, key, in_fmt, in_len, out_fmt, out_len, order, src=F.SRC, dst=F.DST, dither=None, meters=False,
              opts=()):
    """(bytes [nclips * K, (P + SLACK) * B] in the CALLER's order, meters in the caller's order or None, the object's
    tail_launches) of the existing strided call -- _ex, or _mix with the matrix M -- on a second object GIVEN the clips in
    `order` (planar rows of T frames, garbage past each clip's end).  Computed once per tier and case, never modified"""
    k = (tier.gpu, K, None if M is None else np.asarray(M).tobytes(), key, in_fmt, tuple(in_len), out_fmt, tuple(out_len),
         tuple(order), src, dst, dither, meters, tuple(opts))
    if k not in _REF:
        Kin = K if M is None else np.shape(M)[1]
        nclips = len(in_len)
        gin, gout = [in_len[i] for i in order], [out_len[i] for i in order]
        units = F.encode_units(x[rows_in_order(order, Kin)], in_fmt, F.rows_of(gin, Kin))
        Pmax, B = max(out_len), BYTES[out_fmt]
        b = tier.make(nclips * K, src, dst, dither, meters, opts)
        xin = tier.buf(units)
        out = tier.sentinels(nclips * K * (Pmax + SLACK) * B)
        if M is None:
            p = b.resample_clips_ex_ptr(K, tier.ptr(xin), in_fmt, False, T, gin, tier.ptr(out), out_fmt, False, Pmax + SLACK, gout)
        else:
            p = b.resample_clips_mix_ptr(Kin, K, M, tier.ptr(xin), in_fmt, False, T, gin, tier.ptr(out), out_fmt, False,
                                         Pmax + SLACK, gout)
        assert p == Pmax
        given = tier.host(out).reshape(nclips * K, (Pmax + SLACK) * B)
        back = np.argsort(rows_in_order(order, K))                 # caller's row -> the row it was given as
        got = given[back].copy()
        got.setflags(write=False)
        m = None
        if meters:
            m = {name: v[back] for name, v in b.read_meters().items()}
        _REF[k] = (got, m, b.stat("tail_launches"))
    return _REF[k]


def plan_counts(lib, src, dst, P_):
    """the per-step output counts of a call that ends with output P_ (r8b_plan_step; Src == Dst: a step hands MaxInLen on)"""
    counts, done = [], 0
    p = None if src == dst else lib.r8b_plan_create(src, dst, CHUNK, 2.0, F.ATT)
    while done < P_:
        n = CHUNK if p is None else lib.r8b_plan_step(p, CHUNK)
        counts.append(n)
        done += n
    if p is not None:
        lib.r8b_plan_delete(p)
    return counts


def expected_counters(lib, src, dst, K, out_len, flags):
    """(clip_steps, clip_channel_steps) by the header's rule"""
    order = stable_order(out_len, flags)
    nclips, steps, chans, done = len(out_len), 0, 0, 0
    for n in plan_counts(lib, src, dst, max(out_len)):
        hi = max([g + 1 for g in range(nclips) if out_len[order[g]] > done] + [0])
        A = hi * K
        if A % 2 and hi < nclips:
            A += K
        steps, chans, done = steps + 1, chans + (A if flags & DROP else nclips * K), done + n
    return steps, chans


def check_sched(tier, K, M, x, key, in_fmt, in_len, out_fmt, out_len, flags, layouts=ALL_LAYOUTS, addressings=BOTH_ADDRESSINGS,
                src=F.SRC, dst=F.DST, dither=None, meters=False, opts=(), ref_order=None):
    """the flagged call in each layout pair and addressing against the existing call: every byte of the output buffer (a
    packed side: each clip's region and sentinels everywhere else; a strided one: padding zeros and slack included), the
    meters if on, and the two counters.  ref_order: the order the reference is given the clips in (default: the
    schedule's)"""
    lib = tier.abi()
    rc, order = schedule(lib, out_len, flags)
    assert rc == 0 and order == stable_order(out_len, flags)
    ref, ref_m, ref_tails = reference(tier, K, M, x, key, in_fmt, in_len, out_fmt, out_len, order if ref_order is None else ref_order,
                                      src, dst, dither, meters, opts)
    Kin = K if M is None else np.shape(M)[1]
    nclips = len(in_len)
    units = F.encode_units(x, in_fmt, F.rows_of(in_len, Kin))
    Pmax, B = max(out_len), BYTES[out_fmt]
    want_counters = expected_counters(lib, src, dst, K, out_len, flags)
    # (where the clips lie in a packed buffer: tests/test_clip_packed.py's order for its six, a stride of 5 for twelve)
    perm = P.ORDER if nclips == NCLIPS else [(i * 5 + 3) % nclips for i in range(nclips)]
    for in_packed, out_packed in addressings:
        for in_il, out_il in layouts:
            if in_packed:
                xb, in_off = P.pack_in(units, Kin, in_il, in_len, perm)
                in_stride = 0
            else:
                (xb, in_stride), in_off = F.lay_in(units, Kin, in_il), None
            if out_packed:
                out_off, total = P.pack_offsets([n * K for n in out_len], perm[::-1], P.GAPS[::-1])
                want, out_stride = P.pack_out(ref, K, B, out_il, out_len, out_off, total), 0
            else:
                out_off, out_stride = None, (Pmax * K + SLACK if out_il else Pmax + SLACK)
                want = F.lay_out(ref, K, Pmax, B, out_il)
            xin, out = tier.buf(xb), tier.sentinels(want.size)
            a = tier.make(nclips * K, src, dst, dither, meters, opts)
            p = a.resample_clips_sched_ptr(0 if M is None else Kin, K, M, tier.ptr(xin), in_fmt, in_il, in_stride, in_off,
                                           in_len, tier.ptr(out), out_fmt, out_il, out_stride, out_off, out_len, flags)
            assert p == Pmax
            what = ("flags", flags, "packed", in_packed, out_packed, "interleaved", in_il, out_il)
            P.assert_same(tier.host(out), want, what)
            if meters:
                m = a.read_meters()
                for name in ("peak", "clipped", "nonfinite"):
                    assert np.array_equal(m[name], ref_m[name]), (name, what, m[name], ref_m[name])
            assert (a.stat("clip_steps"), a.stat("clip_channel_steps")) == want_counters, what
            # (the history copy still rides on the launch that carried it: a dropping step starts no k_tail of its own)
            assert a.stat("tail_launches") == ref_tails, what
    return ref, ref_m, want_counters


_HOT = {}


def hot(K, lens):
    """the noise with something for the meters: the longest clip's first channel times 1.5, an Inf inside the last
    channel of the 4500-frame clip (fp64 input carries both)"""
    k = (K, tuple(lens))
    if k not in _HOT:
        x = P.signal(NCLIPS * K).copy()
        x[lens.index(6001) * K] *= 1.5
        x[lens.index(4500) * K + K - 1, 700] = np.inf
        x.setflags(write=False)
        _HOT[k] = x
    return _HOT[k]


# ---------------------------------------------------------------- 1. drop alone, 2. the counters
def check_drop(tier, K, name):
    lens = LENGTH_ORDERS[name]
    out_len = P.out_lens(tier, lens)
    _, _, (steps, chans) = check_sched(tier, K, None, P.signal(NCLIPS * K), "noise", S16, lens, F32, out_len, DROP)
    ref, m, _ = check_sched(tier, K, None, hot(K, lens), "hot", F64, lens, P.DITHERED[K], out_len, DROP, dither=5, meters=True)
    # (no silence, and the meters have seen something)
    c6, c45 = lens.index(6001) * K, lens.index(4500) * K + K - 1
    assert np.count_nonzero(ref[c6, :5000 * BYTES[P.DITHERED[K]]]) > 1000
    assert m["clipped"][c6] > 100 and m["nonfinite"][c45] > 0 and m["peak"][c6] > 1.0
    # the schedule did what the order allows (the clip that runs 3000 frames on keeps its slot live to the end)
    assert steps == len(plan_counts(tier.abi(), F.SRC, F.DST, max(out_len)))
    if name == "descending":
        assert chans < steps * NCLIPS * K
    if name == "ascending":
        assert chans == steps * NCLIPS * K


@pytest.mark.parametrize("name", sorted(LENGTH_ORDERS))
@pytest.mark.parametrize("K", [1, 2, 3, 33])
def test_drop_alone_emulated(emul, K, name):
    check_drop(Tier(emul), K, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LENGTH_ORDERS))
@pytest.mark.parametrize("K", [1, 2, 3, 33])
def test_drop_alone_gpu(K, name):
    check_drop(Tier(None), K, name)


# ---------------------------------------------------------------- 3. the order
def test_clip_schedule():
    lib = r8b.load()
    cases = [[5, 5, 5], [0, 7, 7, 3, 7, 0, 9], [1], [], [3, 2, 1], [1, 2, 3], [4, 0, 4, 0, 4, 0, 2, 2]]
    for lens in cases:
        for flags in (0, DROP, ORDER, DROP | ORDER):
            assert schedule(lib, lens, flags) == (0, stable_order(lens, flags)), (lens, flags)
    assert schedule(lib, [0, 7, 7, 3, 7, 0, 9], ORDER)[1] == [6, 1, 2, 4, 3, 0, 5]
    # refusals touch nothing
    assert schedule(lib, [1, -2, 3], ORDER) == (-1, [-7] * 3)
    assert schedule(lib, [1, 2, 3], 4) == (-1, [-7] * 3)
    assert schedule(lib, [1, 2, 3], ORDER | 8) == (-1, [-7] * 3)
    assert lib.r8b_clip_schedule(-1, None, 0, None) == -1
    assert lib.r8b_clip_schedule(2, None, 0, None) == -1


def check_order(tier, K):
    """scattered lengths: with K odd the slot count `hi` is odd in some step and the next clip rides along"""
    lens = LENGTH_ORDERS["scattered"]
    out_len = P.out_lens(tier, lens)
    x = P.signal(NCLIPS * K)
    # (the Python entry is the same call)
    assert tier.make(2).clip_schedule(out_len, ORDER) == stable_order(out_len, ORDER)
    for flags in (ORDER, ORDER | DROP):
        _, _, (steps, chans) = check_sched(tier, K, None, x, "noise", S16, lens, F32, out_len, flags)
        check_sched(tier, K, None, x, "noise", F64, lens, S24, out_len, flags, layouts=[(True, False), (False, True)], meters=True)
    assert chans < steps * NCLIPS * K
    # (odd K: some step's A is a whole clip above hi K)
    if K % 2:
        order, done, seen = stable_order(out_len, ORDER), 0, False
        for n in plan_counts(tier.abi(), F.SRC, F.DST, max(out_len)):
            hi = max([g + 1 for g in range(NCLIPS) if out_len[order[g]] > done] + [0])
            seen, done = seen or (hi * K % 2 == 1 and hi < NCLIPS), done + n
        assert seen


@pytest.mark.parametrize("K", [1, 3])
def test_order_emulated(emul, K):
    check_order(Tier(emul), K)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3])
def test_order_gpu(K):
    check_order(Tier(None), K)


def check_dither_under_order(tier, K):
    """Src == Dst: against the object's own kind with flags 0 -- the reference is GIVEN the clips in the caller's order"""
    lens = LENGTH_ORDERS["scattered"]
    out_len = [n + 40 if n == 1999 else n for n in lens]        # (one clip's output runs past its input: dithered silence)
    for flags in (ORDER, ORDER | DROP):
        _, m, _ = check_sched(tier, K, None, hot(K, lens), "hot", F64, lens, P.DITHERED[K], out_len, flags, src=48000.0, dst=48000.0,
                              dither=5, meters=True, ref_order=list(range(NCLIPS)))
    assert m["clipped"][lens.index(6001) * K] > 100


@pytest.mark.parametrize("K", [1, 3])
def test_dither_under_order_emulated(emul, K):
    check_dither_under_order(Tier(emul), K)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3])
def test_dither_under_order_gpu(K):
    check_dither_under_order(Tier(None), K)


# ---------------------------------------------------------------- 4. other chains
TWELVE = [0, 6001, 1, 4500, 1999, 2000, 3000, 6001, 1000, 2500, 4500, 4000]       # (ties: the sort must be stable)
# 44100 -> 44101: a cap of 16 KB on the stream between convolver and polynomial interpolator walks the twelve channels
# in several groups (Engine::process; the last group of a dropping step is cut at the active count)
CHAINS = {"down": (96000.0, 44100.0, ()), "poly": (44100.0, 44101.0, (("poly_groups", 16),)),
          "cascade": (44100.0, 176400.0, ()), "pass": (48000.0, 48000.0, ())}


def check_chain(tier, name):
    src, dst, opts = CHAINS[name]
    out_len = tier.out_len(TWELVE, src, dst)
    out_len[3] -= 100
    out_len[8] += 500
    x = P.signal(12)
    _, _, (steps, chans) = check_sched(tier, 1, None, x, "noise", S16, TWELVE, F32, out_len, DROP | ORDER,
                                       layouts=[(False, False)], src=src, dst=dst, opts=opts)
    assert steps >= 3 and chans < steps * 12


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_other_chains_emulated(emul, name):
    check_chain(Tier(emul), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CHAINS))
def test_other_chains_gpu(name):
    check_chain(Tier(None), name)


# ---------------------------------------------------------------- 5. the mixing ingest
def check_mix(tier, name):
    M, in_fmt, out_fmt, layouts = P.MIXES[name]
    M = np.asarray(M, dtype=np.float64)
    lens = LENGTH_ORDERS["scattered"]
    check_sched(tier, M.shape[0], M, P.signal(NCLIPS * M.shape[1]), "noise", in_fmt, lens, out_fmt, P.out_lens(tier, lens),
                DROP | ORDER, layouts=layouts)


@pytest.mark.parametrize("name", sorted(P.MIXES))
def test_mix_emulated(emul, name):
    check_mix(Tier(emul), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(P.MIXES))
def test_mix_gpu(name):
    check_mix(Tier(None), name)


# ---------------------------------------------------------------- 6. back to back
def check_back_to_back(tier, stream=0, wait=lambda: None):
    """five flagged calls and a plain one on ONE object and one stream, nothing waits in between: more calls than the
    object has slots, each with its own lengths, offsets and flags -- every call's kernels read ITS lengths, bases and
    channels, and the plain call after the dropping ones finds no stale state in the channels they left behind"""
    rot = lambda v, r: v[r:] + v[:r]
    x = P.signal(NCLIPS)
    calls = []
    for j, flags in enumerate([DROP, DROP | ORDER, ORDER, DROP, DROP | ORDER, 0]):
        in_len = rot(LENGTH_ORDERS["descending"], j)
        out_len = [n + 7 * j for n in tier.out_len(in_len)]
        ref, _, _ = reference(tier, 1, None, x, "noise", S16, in_len, F64, out_len, stable_order(out_len, flags))
        xb, in_off = P.pack_in(F.encode_units(x, S16, in_len), 1, True, in_len, rot(P.ORDER, j), rot(P.GAPS, j % 3))
        out_off, total = P.pack_offsets(out_len, rot(P.ORDER, j)[::-1], rot(P.GAPS, (j + 1) % 3))
        want = P.pack_out(ref, 1, 8, False, out_len, out_off, total)
        calls.append((flags, tier.buf(xb), in_off, in_len, tier.sentinels(want.size), out_off, out_len, want))
    tier.sync()
    a = tier.make(NCLIPS)
    for flags, xin, in_off, in_len, out, out_off, out_len, _ in calls:
        assert a.resample_clips_sched_ptr(0, 1, None, tier.ptr(xin), S16, True, 0, in_off, in_len, tier.ptr(out), F64, False, 0,
                                          out_off, out_len, flags, stream) == max(out_len)
    wait()
    for j, call in enumerate(calls):
        P.assert_same(tier.host(call[4]), call[7], ("call", j, "flags", call[0]))


def test_back_to_back_emulated(emul):
    check_back_to_back(Tier(emul))


@pytest.mark.gpu
def test_back_to_back_on_one_stream_gpu():
    import torch
    s = torch.cuda.Stream()
    check_back_to_back(Tier(None), s.cuda_stream, s.synchronize)


# ---------------------------------------------------------------- 7. refusals
def check_refusals(tier):
    K = 2
    x, in_len = P.signal(NCLIPS * K), LENGTH_ORDERS["scattered"]
    out_len = tier.out_len(in_len)
    Pmax, max_in = max(out_len), max(in_len)
    flags = DROP | ORDER
    ref, _, _ = reference(tier, K, None, x, "noise", F64, in_len, F64, out_len, stable_order(out_len, flags))
    units = F.encode_units(x, F64, F.rows_of(in_len, K))
    xb, in_off = P.pack_in(units, K, True, in_len)
    out_off, total = P.pack_offsets([n * K for n in out_len])
    want = P.pack_out(ref, K, 8, True, out_len, out_off, total)
    xs, _ = F.lay_in(units, K, True)
    xin, xstr, out = tier.buf(xb), tier.buf(xs), tier.sentinels(want.size)
    a = tier.make(NCLIPS * K)
    err = a._lib.r8b_last_error

    def call(kin=0, mix=None, i_off=in_off, o_off=out_off, src=xin, i_stride=0, o_stride=0, obj=a, fl=flags):
        return tier.raw_sched(obj, kin, K, mix, src, F64, True, i_stride, i_off, in_len, out, F64, True, o_stride, o_off,
                              out_len, fl)

    def refused(word, **kw):
        assert call(**kw) == -1, kw
        assert word in err(), (kw, err())
        assert np.all(tier.host(out) == SENTINEL), kw
        assert a.stat("clip_steps") == 0

    for bad in (4, 8 | DROP, 0x40000000 | ORDER, -1):
        refused(b"flags", fl=bad)
    # ... and everything the packed call refuses, with the flags set
    refused(b"in_offset", i_off=in_off[:2] + [-1] + in_off[3:])
    refused(b"out_offset", o_off=out_off[:4] + [-8] + out_off[5:])
    i5, i3 = in_len.index(6001), in_len.index(1999)
    refused(b"out_offset", o_off=[out_off[i5] + out_len[i5] * K - 1 if i == i3 else o for i, o in enumerate(out_off)])
    for bad in (1, 3, -1, 65):
        refused(b"in_channels", kin=bad)
    refused(b"in_channels", kin=65, mix=[0.5] * (65 * K))
    refused(b"in_stride", i_off=None, src=xstr, i_stride=max_in * K - 1)
    refused(b"out_stride", o_off=None, o_stride=Pmax * K - 1)
    b = tier.make(NCLIPS * K)
    blk, res = tier.buf(np.zeros((NCLIPS * K, CHUNK))), tier.buf(np.zeros((NCLIPS * K, max(b.max_out_len, 1))))
    tier.sync()
    b.process_ptr(tier.ptr(blk), CHUNK, CHUNK, tier.ptr(res), max(b.max_out_len, 1))
    refused(b"processed samples", obj=b)
    # ... none of which used the object up or changed it
    assert call() == Pmax
    P.assert_same(tier.host(out), want, "after the refusals")


def test_refusals_emulated(emul):
    check_refusals(Tier(emul))


@pytest.mark.gpu
def test_refusals_gpu():
    check_refusals(Tier(None))


# ---------------------------------------------------------------- the Python keywords
@pytest.mark.gpu
def test_keywords_gpu():
    import torch
    tier = Tier(None)
    K = 2
    x, in_len = P.signal(NCLIPS * K), LENGTH_ORDERS["scattered"]
    rows = np.ascontiguousarray(F.encode_units(x, S16, F.rows_of(in_len, K))).view(np.int16).reshape(NCLIPS * K, T)
    xt = torch.from_numpy(np.ascontiguousarray(rows.reshape(NCLIPS, K, T).transpose(0, 2, 1))).cuda()
    a = tier.make(NCLIPS * K)
    plain, ol = a.resample_clips(xt, in_len, out_format=F32, clip_channels=K, interleaved=True)
    dropped, ol2 = a.resample_clips(xt, in_len, out_format=F32, clip_channels=K, interleaved=True, drop_finished=True)
    # (two calls so far, the second of which dropped)
    assert ol2 == ol and a.stat("clip_channel_steps") < a.stat("clip_steps") * NCLIPS * K
    assert torch.equal(plain.view(torch.int32), dropped.view(torch.int32))
    # sorted: the samples of the plain call GIVEN the order, in the caller's order
    order = a.clip_schedule(ol, ORDER)
    given, _ = a.resample_clips(xt[order].contiguous(), [in_len[i] for i in order], out_format=F32, clip_channels=K, interleaved=True)
    both, _ = a.resample_clips(xt, in_len, out_format=F32, clip_channels=K, interleaved=True, drop_finished=True, longest_first=True)
    for g, i in enumerate(order):
        assert torch.equal(both[i].view(torch.int32), given[g].view(torch.int32)), i
    packed = torch.from_numpy(np.concatenate([rows[i * K:(i + 1) * K, :n].T.reshape(-1) for i, n in enumerate(in_len)])).cuda()
    out, off, _ = a.resample_clips_packed(packed, in_len, out_format=F32, clip_channels=K, interleaved=True, drop_finished=True,
                                          longest_first=True)
    torch.cuda.synchronize()
    for i, n in enumerate(ol):
        assert torch.equal(out[off[i]:off[i] + n * K].view(torch.int32), both[i, :n].reshape(-1).view(torch.int32)), i
