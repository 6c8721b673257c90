"""The time axis: stream positions past 2^31, 2^32 and 2^40 samples.

Every kernel is addressed by absolute stream position (r8b_launch.h, r8b_plan.h), and a 2.8224 MHz stream passes 2^31
samples after 12.7 minutes.  Feeding that many samples is out of reach for a test, but with all-zero input every ring
stays zero and only the plan's integer counters move: the test builds' r8b_batch_test_skip_silence (include/r8bsrc.h)
puts an object at position T without a launch, and the oracle's skip_silence() does the same on its own closed forms.

  a. the hook is honest where feeding can check it: skip(T) against T real zeros, bit for bit
  b. every stream of every chain -- the chain's input and each stage's output -- crosses 2^31 and 2^32 while noise flows,
     and runs at 2^40 + 12345, against one offset oracle per channel
  c. checkpoint and clear() past 2^32
  d. the egress dither's frame number past 2^32 output frames

Both tiers run every check: the host emulation (cases.emul_lib(test_hooks=True)) and the GPU through the test-hooks
build of the library (conftest hip_hooks).  Three channels: a pair and a lone channel."""
import importlib

import numpy as np
import pytest

import cases
import r8b_oracle as O
import test_pcm_finish as F   # (the dither's restatement in numpy: np_dither, np_encode, unpack24)

r8b = importlib.import_module("r8brain-free-src_amd")

NCH = 3
B31, B32 = 1 << 31, 1 << 32
FAR = (1 << 40) + 12345


# ---------------------------------------------------------------- the two tiers
@pytest.fixture(scope="module")
def emul():
    return cases.emul_lib(test_hooks=True)


class Tier:
    """lib: a TEST build of the library; gpu: it is the HIP one (torch tensors through the device entry), else the
    host emulation (numpy buffers through process_host)"""

    def __init__(self, lib, gpu):
        self.lib, self.gpu = lib, gpu

    def make(self, chain, options=None, nch=NCH):
        src, dst, maxin, tb, att = chain
        a = r8b.BatchResampler(src, dst, maxin, tb, att, nch=nch, lib=self.lib, device=0 if self.gpu else -1)
        for k, v in (options or {}).items():
            a.set_option(k, v)
        return a

    def feed(self, a, x):
        if not self.gpu:
            return a.process_host(x)
        import torch
        y = a.process(torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0"))
        return y.cpu().numpy()


@pytest.fixture(scope="module")
def tier_emul(emul):
    return Tier(emul, False)


@pytest.fixture(scope="module")
def tier_gpu(hip_hooks):
    return Tier(hip_hooks, True)


# ---------------------------------------------------------------- chains
# (src, dst, MaxInLen, tb, atten), {engine options}, what must have run: every entry a substring of some stage's
# "label|symbol" (the engine's label of the stage's form and, for the compile-time-sized convolvers, the kernel symbol
# with its mode -- as tests/test_emul.py FORM_PINS records them), a counter that must have moved ("stat:<name>"), a
# piece of the chain's describe() text ("fft=..."), or the device symbol of a kernel that is not compile-time sized, which
# only the GPU tier can name ("gpu:<symbol>")
CFG2 = (44100.0, 96000.0, 4096, 2.0, 180.15)
CFG3 = (96000.0, 44100.0, 4096, 2.0, 180.15)
UP2 = (44100.0, 88200.0, 4096, 2.0, 180.15)
DOWN2 = (88200.0, 44100.0, 4096, 2.0, 180.15)
CFG5 = (44100.0, 2822400.0, 1024, 2.0, 180.15)
SACD2 = (2822400.0, 176400.0, 4096, 2.0, 180.15)
UP3 = (44100.0, 132300.0, 1024, 2.0, 180.15)
VARIANTS = [
    # fused two-phase pair kernel with parked outputs, and what each structural choice leaves of it
    (CFG2, {}, ["k_convp_whole|k_convp<11, 1, 4, 24>", "stat:park_calls"]),
    (CFG2, {"half_fused": 2}, ["k_convp_whole|k_convp<11, 1, 23, 24>", "stat:park_calls"]),
    (CFG2, {"park": 0}, ["k_convp_whole|k_convp<11, 1, 4, 24>"]),
    (CFG2, {"pair_two": 0}, ["k_convp_whole|k_convp<11, 1, 1, 24>"]),
    (CFG2, {"fuse": 0}, ["k_convp|k_convp<11, 1, 0, 24>", "k_whole|"]),
    (CFG2, {"pair_conv": 0}, ["k_convx_whole|k_convx<10, 1, 1, 24>"]),
    (CFG2, {"fast_conv": 0}, ["k_conv|", "k_whole|"]),
    # ... in its walk form (a call of 16384 samples has interior blocks to walk: tests/test_emul.py WALK_CASES)
    ((44100.0, 96000.0, 16384, 2.0, 180.15), {"walk": 2}, ["k_convp_whole|k_convp_walk<", "stat:walk_blocks"]),
    # 1:1 fused pair kernel
    (CFG3, {}, ["k_convp_whole|k_convp<12, 0, 5, 24>", "stat:park_calls"]),
    (CFG3, {"half_fused": 2}, ["k_convp_whole|k_convp<12, 0, 33, 24>", "stat:park_calls"]),
    # convolver only
    (UP2, {}, ["k_convp|k_convp<11, 1, 0, 24>", "stat:park_calls"]),
    (UP2, {"half": 2}, ["k_convp|k_convp<11, 1, 21, 24>"]),
    (UP2, {"quad": 1}, ["k_convp|k_convq"]),
    # decimating pair kernel
    (DOWN2, {}, ["k_convp|k_convp<12, -1, 0, 24>", "stat:park_calls"]),
    (DOWN2, {"half": 2}, ["k_convp|k_convp<12, -1, 27, 24>"]),
    # half-band cascade with the carried history copy
    (CFG5, {}, ["k_convp|k_convp<11, 1, 0, 24>", "k_hbcascade|"]),
    (CFG5, {"fuse_hb": 0}, ["k_convp|k_convp<11, 1, 0, 24>", "k_hbup|"]),
    # decimating half-band cascade
    (SACD2, {}, ["k_hbdcascade|", "k_convp|k_convp<12, -1, 0, 24>"]),
    (SACD2, {"fuse_hbd": 0}, ["k_hbdown|", "k_convp|k_convp<12, -1, 0, 24>"]),
    (SACD2, {"fuse_hbconv": 1}, ["k_convp_hb|k_convp<12, -1, 20, 24>"]),
    # half-band decimator + 2x-decimating convolver
    ((176400.0, 44100.0, 4096, 2.0, 180.15), {}, ["k_hbdown|", "k_convp|k_convp<12, -1, 0, 24>"]),
    # polyphase 3x, and the zero-stuffing block behind it
    (UP3, {}, ["k_convp|k_convp<11, 0, 19, 24>", "stat:park_calls"]),
    (UP3, {"up3_poly": 0}, ["k_convp|k_convp<13, 0, 3, 24>"]),
    # strided store, 3/2, 3/4
    ((48000.0, 32000.0, 1024, 2.0, 180.15), {}, ["k_convp|k_convp<12, 1, 3, 24>"]),
    ((32000.0, 48000.0, 1024, 2.0, 180.15), {}, ["k_convp|k_convp<13, -1, 3, 24>"]),
    ((64000.0, 48000.0, 1024, 2.0, 180.15), {}, ["k_convp|k_convp<13, -2, 3, 24>"]),
    # interpolator first
    ((11025.0, 96000.0, 512, 2.0, 136.45), {}, ["k_convp_whole|", "k_whole|", "k_convp|k_convp<9, 1, 0, 24>", "k_hbcascade|"]),
    ((44100.0, 192000.0, 512, 2.0, 180.15), {}, ["k_convp_whole|", "k_whole|", "k_convp|k_convp<10, 1, 0, 24>", "k_hbup|"]),
    # last-stage half-band pair stores: position parity
    ((8000.0, 44100.0, 1024, 2.0, 180.15), {}, ["k_convp_whole|", "k_whole|", "k_convp|k_convp<8, 1, 0, 24>", "k_hbup|"]),
    # more phases than threads / fewer phases than threads
    ((32000.0, 44100.0, 4096, 2.0, 180.15), {}, ["k_convp_whole|k_convp<11, 1, 5, 24>"]),
    ((88200.0, 48000.0, 4096, 2.0, 180.15), {}, ["k_convp_whole|k_convp<12, 1, 1, 24>"]),
    # several blocks per workgroup
    ((44100.0, 96000.0, 4096, 10.0, 109.56), {}, ["k_convp_whole|k_convp<8, 1, 1, 24>"]),
    ((88200.0, 44100.0, 2048, 45.0, 49.0), {}, ["k_convp|k_convp<6, -1, 0, 24>"]),
    # split form
    ((44100.0, 88200.0, 2048, 0.5, 180.15), {}, ["k_convp|k_convp<13, 0, 8, 24>"]),
    # one-channel 16384-point form
    ((96000.0, 44100.0, 8192, 0.5, 180.15), {}, ["k_convp_whole|k_convp<13, 0, 18, 24>"]),
    # the reference's own 32768-point block on the generic kernel
    ((32000.0, 48000.0, 2048, 0.5, 180.15), {}, ["k_conv|", "fft=32768/16384", "gpu:k_conv_big"]),
]


def vid(v):
    chain, options, _ = v
    return "%g-%g-%d-%g-%g%s" % (chain + ("".join("-%s%d" % kv for kv in sorted(options.items())),))


def nstreams(chain):
    return len(O.build_topology(chain[0], chain[1], chain[3], chain[4])) + 1


# ---------------------------------------------------------------- the oracle side, computed once per (chain, T, calls)
_PROBE = {}


def probe(chain):
    """an oracle of the chain that is never fed: its closed forms"""
    if chain not in _PROBE:
        _PROBE[chain] = O.OracleResampler(*chain)
    return _PROBE[chain]


def stream_counts(chain, m):
    """samples of every stream -- the chain's input, each stage's output -- after m input samples"""
    c = [m]
    for s in probe(chain).stages:
        m = s.total(m)
        c.append(m)
    return c


def first_input_reaching(chain, k, B):
    """the smallest m at which stream k holds B samples"""
    hi = 1
    while stream_counts(chain, hi)[k] < B:
        hi *= 2
    lo = hi // 2
    while lo + 1 < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if stream_counts(chain, mid)[k] >= B else (mid, hi)
    return hi


def crossing_plan(chain, k, B):
    """(T, call lengths, index of the crossing call): noise from position T in ragged calls -- past the chain's latency
    plus a call, so that outputs flow --, then a 1-sample call that takes stream k from below B to B or past it (the
    chain's input: from B - 1 to B), then a call whose first sample is the next one (the chain's input: sample B
    exactly), then two more"""
    c = chain[2]
    lat = probe(chain).in_len_before_out_pos(0)
    pre, pattern = [], [c, c // 3 + 1, max(c - 7, 1), 17]
    while sum(pre) < lat + c // 2:
        pre.append(pattern[len(pre) % 4])
    pre.append(c)
    m = first_input_reaching(chain, k, B)
    return m - 1 - sum(pre), pre + [1, c, c // 2 + 3], len(pre)


_ORACLE = {}


def oracle_run(chain, T, lens):
    """One oracle per channel, skipped by T and fed the calls of noise: (input [NCH, sum(lens)], per call the outputs
    [NCH, n], per call the counts of every stream before and after it).  Computed once for the option variants of a
    chain, which follow each other (the latest run alone is kept), and never modified."""
    key = (chain, T, tuple(lens))
    if key not in _ORACLE:
        _ORACLE.clear()
        x = cases.make_input(NCH, sum(lens), 41)
        os_ = [O.OracleResampler(*chain) for _ in range(NCH)]
        nz = [o.skip_silence(T) for o in os_]
        assert len(set(nz)) == 1

        def counts(o):
            return [o.stages[0].m()] + [s.done for s in o.stages]
        outs, pos, p = [], [], 0
        for l in lens:
            before = counts(os_[0])
            y = np.stack([o.process(x[ch, p:p + l]) for ch, o in enumerate(os_)])
            p += l
            y.setflags(write=False)
            outs.append(y)
            pos.append((before, counts(os_[0])))
        x.setflags(write=False)
        _ORACLE[key] = (x, nz[0], outs, pos)
    return _ORACLE[key]


def forms_of(a, labels):
    """"label|symbol" of every stage's latest launch (symbols of the compile-time-sized convolver kernels only: the
    launchers whose symbol the emulator notes too; a call that a stage served from its park buffer names none)"""
    return ["%s|%s" % (n, s if n.startswith(("k_convp", "k_convx")) else "") for n, s in zip(labels, a.stage_symbols())]


def check_forms(tier, a, expect, forms):
    for e in expect:
        if e.startswith("stat:"):
            assert a.stat(e[5:]) > 0, (e, forms)
        elif e.startswith("fft="):
            assert e in a.describe(), (e, a.describe())
        elif e.startswith("gpu:"):
            assert not tier.gpu or e[4:] in a.stage_symbols(), (e, a.stage_symbols())
        else:
            assert any(e in f for f in forms), (e, forms)


def check_against_oracle(tier, variant, T, lens):
    """counts call by call; the error over the whole signal, per channel, within the project's bounds"""
    chain, options, expect = variant
    x, nz, outs, _ = oracle_run(chain, T, lens)
    a = tier.make(chain, options)
    a.set_option("timing", 1)
    assert cases.skip_silence(a, T) == nz
    err = np.zeros(NCH)
    ref = np.zeros(NCH)
    pk = np.zeros(NCH)
    n, p = 0, 0
    labels, seen = [t[0] for t in a.stage_timings()], set()
    for l, yo in zip(lens, outs):
        y = tier.feed(a, x[:, p:p + l])
        seen.update(forms_of(a, labels))
        p += l
        assert y.shape == yo.shape, (p, y.shape, yo.shape)
        if yo.shape[1]:
            d = y - yo
            err += np.sum(d * d, axis=1)
            ref += np.sum(yo * yo, axis=1)
            pk = np.maximum(pk, np.abs(d).max(axis=1))
            n += yo.shape[1]
    assert n > 0
    rms = np.sqrt(err / n)
    print("T=%d rms %s peak %s" % (T, rms, pk))
    for ch in range(NCH):
        sc = cases.tol_scale(ref[ch], n)
        assert rms[ch] <= cases.RMS_TOL * sc and pk[ch] <= cases.PEAK_TOL * sc, (ch, rms[ch], pk[ch], sc)
    check_forms(tier, a, expect, sorted(seen))


# ---------------------------------------------------------------- a. the hook against real zeros
def ragged(total, c, pattern):
    lens = []
    while sum(lens) < total:
        lens.append(min(pattern[len(lens) % len(pattern)], total - sum(lens)))
    return lens


def check_hook_is_honest(tier, variant):
    chain, options, expect = variant
    c = chain[2]
    lat = probe(chain).in_len_before_out_pos(0)
    a, b = tier.make(chain, options), tier.make(chain, options)
    sig = ragged(2 * lat + 2 * c, c, [c, c // 3 + 1, 1, max(c - 7, 1), 17])
    x = cases.make_input(NCH, sum(sig), 43)
    # (the last one: past the latency, a call and a half into the flowing outputs -- where a parking chain's call ends
    # inside a block whose rest waits in the park buffer)
    for T in (0, 1, c - 1, 3 * c + 17, lat + c + c // 2 + 3):
        a.clear()
        b.clear()
        na = cases.skip_silence(a, T)
        nb = 0
        for l in ragged(T, c, [c // 3 + 1, 1, c, 17]):
            y = tier.feed(b, np.zeros((NCH, l)))
            assert not y.any()
            nb += y.shape[1]
        assert na == nb, (T, na, nb)
        p = 0
        for i, l in enumerate(sig):
            parked = b.stat("park_calls")
            ya, yb = tier.feed(a, x[:, p:p + l]), tier.feed(b, x[:, p:p + l])
            p += l
            assert ya.shape == yb.shape and np.array_equal(ya, yb), (T, i, l, ya.shape, yb.shape)
            if i == 0 and T > lat and "stat:park_calls" in expect:
                # the silence ended inside a parked block: the object fed real zeros serves the first outputs of the
                # signal's first call from its park buffer, the skipped one computes them
                assert b.stat("park_calls") == parked + 1
        assert ya.any()
    with pytest.raises(RuntimeError, match="processed samples"):
        cases.skip_silence(a, 5)          # fed since clear()
    a.clear()
    with pytest.raises(RuntimeError, match="negative"):
        cases.skip_silence(a, -1)


@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
def test_skip_equals_real_zeros_emulated(tier_emul, variant):
    check_hook_is_honest(tier_emul, variant)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
def test_skip_equals_real_zeros_gpu(tier_gpu, variant):
    check_hook_is_honest(tier_gpu, variant)


def check_hook_refuses_polynomial(tier):
    a = tier.make((44100.0, 44101.0, 1024, 2.0, 180.15))
    with pytest.raises(RuntimeError, match="polynomial"):
        cases.skip_silence(a, 100)
    y = tier.feed(a, cases.make_input(NCH, 1024, 3))     # (and nothing moved)
    b = tier.make((44100.0, 44101.0, 1024, 2.0, 180.15))
    assert np.array_equal(y, tier.feed(b, cases.make_input(NCH, 1024, 3)))


def test_skip_refuses_a_polynomial_interpolator_emulated(tier_emul):
    check_hook_refuses_polynomial(tier_emul)


@pytest.mark.gpu
def test_skip_refuses_a_polynomial_interpolator_gpu(tier_gpu):
    check_hook_refuses_polynomial(tier_gpu)


# ---------------------------------------------------------------- b. crossings against the oracle
# (the option variants of a chain side by side: they share the oracle's run)
CHAINS = list(dict.fromkeys(v[0] for v in VARIANTS))
CROSSINGS = [(v, k, B) for c in CHAINS for k in range(nstreams(c)) for B in (B31, B32) for v in VARIANTS if v[0] == c]


def cid(c):
    return "%s-stream%d-2^%d" % (vid(c[0]), c[1], c[2].bit_length() - 1)


def check_crossing(tier, crossing):
    variant, k, B = crossing
    chain = variant[0]
    T, lens, at = crossing_plan(chain, k, B)
    _, _, outs, pos = oracle_run(chain, T, lens)
    # from the oracle's own counters: the stream crosses B in call `at`, with outputs flowing on both sides of it
    assert pos[at][0][k] < B <= pos[at][1][k], (k, B, pos[at])
    assert outs[at - 1].any() and outs[at + 1].any()
    if k == 0:
        assert pos[at + 1][0][0] == B     # the next call's first sample is sample B of the chain's input
    check_against_oracle(tier, variant, T, lens)


@pytest.mark.parametrize("crossing", CROSSINGS, ids=cid)
def test_crossing_emulated(tier_emul, crossing):
    check_crossing(tier_emul, crossing)


@pytest.mark.gpu
@pytest.mark.parametrize("crossing", CROSSINGS, ids=cid)
def test_crossing_gpu(tier_gpu, crossing):
    check_crossing(tier_gpu, crossing)


def check_far(tier, variant):
    chain = variant[0]
    _, lens, _ = crossing_plan(chain, 0, B31)
    _, _, outs, pos = oracle_run(chain, FAR, lens)
    assert pos[0][0][0] == FAR and outs[-1].any() and outs[-2].any()
    check_against_oracle(tier, variant, FAR, lens)


@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
def test_far_position_emulated(tier_emul, variant):
    check_far(tier_emul, variant)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
def test_far_position_gpu(tier_gpu, variant):
    check_far(tier_gpu, variant)


# ---------------------------------------------------------------- c. state at a high position
def check_state_past_2_32(tier, chain):
    c = chain[2]
    lat = probe(chain).in_len_before_out_pos(0)
    T = B32 + 12345
    lens = ragged(lat + 2 * c, c, [c, c // 3 + 1, 17])
    more = [c, 1, c // 2 + 3, c]
    x = cases.make_input(NCH, sum(lens) + sum(more), 47)
    a, b = tier.make(chain), tier.make(chain)
    cases.skip_silence(a, T)
    p = 0
    for l in lens:
        ya = tier.feed(a, x[:, p:p + l])
        p += l
    assert ya.any()
    # checkpoint into a fresh object: it continues the uninterrupted stream bit for bit
    b.load_state_dict(a.state_dict())
    b._produced = a._produced if hasattr(a, "_produced") else 0
    for l in more:
        ya, yb = tier.feed(a, x[:, p:p + l]), tier.feed(b, x[:, p:p + l])
        p += l
        assert ya.shape == yb.shape and np.array_equal(ya, yb), l
    assert ya.any()
    # clear(): the stream of a fresh object from position 0, same counts
    a.clear()
    f = tier.make(chain)
    p, n = 0, 0
    for l in lens + more:
        ya, yf = tier.feed(a, x[:, p:p + l]), tier.feed(f, x[:, p:p + l])
        p += l
        assert ya.shape == yf.shape and np.array_equal(ya, yf), l
        n += ya.shape[1]
    assert n > 0 and ya.any()


@pytest.mark.parametrize("chain", [CFG2, CFG3], ids=["44100-96000", "96000-44100"])
def test_state_past_2_32_emulated(tier_emul, chain):
    check_state_past_2_32(tier_emul, chain)


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [CFG2, CFG3], ids=["44100-96000", "96000-44100"])
def test_state_past_2_32_gpu(tier_gpu, chain):
    check_state_past_2_32(tier_gpu, chain)


# ---------------------------------------------------------------- d. dither past 2^32 output frames
DITHER_CHAIN = (F.SRC, F.DST, F.CHUNK, 2.0, F.ATT)
_DITHER_REF = {}


def dither_plan():
    """T and three calls of CHUNK frames: the output frame number passes 2^32 inside the second one"""
    m = first_input_reaching(DITHER_CHAIN, nstreams(DITHER_CHAIN) - 1, B32)
    return m - F.CHUNK - F.CHUNK // 2, [F.CHUNK] * 3


def dither_reference(tier, nch):
    """(input, frames skipped, fp64 outputs per call) of a plain object skipped by the same T; once per tier and count"""
    key = (tier.gpu, nch)
    if key not in _DITHER_REF:
        T, lens = dither_plan()
        x = 0.9 * cases.make_input(nch, sum(lens), 101)
        b = tier.make(DITHER_CHAIN, nch=nch)
        j0 = cases.skip_silence(b, T)
        outs = [b.process_host(x[:, i:i + F.CHUNK]) for i in range(0, sum(lens), F.CHUNK)]
        for v in [x] + outs:
            v.setflags(write=False)
        _DITHER_REF[key] = (x, j0, outs)
    return _DITHER_REF[key]


def pcm_call(tier, a, x, fmt, interleaved):
    """F.Tier.call for either tier of this module (F.Tier tells the tiers apart by the library being None)"""
    nch, l = x.shape
    cap = max(a.max_out_len, 1)
    shape = ((cap, nch) if interleaved else (nch, cap)) + ((3,) if fmt == r8b.PCM_S24 else ())
    x = np.ascontiguousarray(x)
    if not tier.gpu:
        out = np.zeros(shape, dtype=F.NP_DTYPE[fmt])
        n = a.process_pcm_ptr(x.ctypes.data, r8b.PCM_F64, False, l, l, out.ctypes.data, fmt, interleaved,
                              nch if interleaved else cap)
    else:
        import torch
        xt = torch.tensor(x, device="cuda")
        ot = torch.zeros(shape, dtype=getattr(torch, np.dtype(F.NP_DTYPE[fmt]).name), device="cuda")
        n = a.process_pcm_ptr(xt.data_ptr(), r8b.PCM_F64, False, l, l, ot.data_ptr(), fmt, interleaved,
                              nch if interleaved else cap)
        torch.cuda.synchronize()
        out = ot.cpu().numpy()
    out = out[:n] if interleaved else out[:, :n]
    if fmt == r8b.PCM_S24:
        out = F.unpack24(out)
    return np.ascontiguousarray(out.T) if interleaved else out


def check_dither_past_2_32(tier, nch, fmt, interleaved):
    T, lens = dither_plan()
    x, j0, outs = dither_reference(tier, nch)
    n0 = outs[0].shape[1]
    assert j0 + n0 < B32 < j0 + n0 + outs[1].shape[1]     # frames cross 2^32 inside the second call
    a = tier.make(DITHER_CHAIN, nch=nch)
    a.set_dither(r8b.DITHER_TPDF, F.SEED)
    assert cases.skip_silence(a, T) == j0
    got = np.concatenate([pcm_call(tier, a, x[:, i:i + F.CHUNK], fmt, interleaved)
                          for i in range(0, sum(lens), F.CHUNK)], axis=1)
    v = np.concatenate(outs, axis=1)
    want, _ = F.np_encode(v, fmt, F.np_dither(F.SEED, 0, nch, j0, v.shape[1]))
    assert got.shape == want.shape and np.array_equal(got, want), (nch, fmt, interleaved, int(np.sum(got != want)))
    # (a frame number kept in 32 bits would give another sequence from frame 2^32 on)
    wrapped = np.concatenate([F.np_dither(F.SEED, 0, nch, j0, B32 - j0),
                              F.np_dither(F.SEED, 0, nch, 0, v.shape[1] - (B32 - j0))], axis=1)
    assert not np.array_equal(got, F.np_encode(v, fmt, wrapped)[0])


@pytest.mark.parametrize("interleaved", [False, True], ids=["planar", "interleaved"])
@pytest.mark.parametrize("fmt", [r8b.PCM_S16, r8b.PCM_S24], ids=["s16", "s24"])
@pytest.mark.parametrize("nch", [3, 65])
def test_dither_past_2_32_frames_emulated(tier_emul, nch, fmt, interleaved):
    check_dither_past_2_32(tier_emul, nch, fmt, interleaved)


@pytest.mark.gpu
@pytest.mark.parametrize("interleaved", [False, True], ids=["planar", "interleaved"])
@pytest.mark.parametrize("fmt", [r8b.PCM_S16, r8b.PCM_S24], ids=["s16", "s24"])
@pytest.mark.parametrize("nch", [3, 65])
def test_dither_past_2_32_frames_gpu(tier_gpu, nch, fmt, interleaved):
    check_dither_past_2_32(tier_gpu, nch, fmt, interleaved)


# ---------------------------------------------------------------- signed overflow on the host
@pytest.mark.slow
def test_positions_past_2_32_under_the_overflow_sanitizer():
    """tests/cxx_time_axis.cpp: the emulation's sources and a stand-alone driver as one program built with
    -fsanitize=signed-integer-overflow,shift -fno-sanitize-recover (tests/emul/Makefile `ubsan`, two minutes of
    compilation); three chains across 2^31 and 2^32 on the input and on the output side.  Host code only."""
    import os
    import subprocess
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul")
    out = subprocess.run(["make", "-j8", "ubsan"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and "runtime error" not in out.stdout and out.stdout.strip().endswith("OK"), out.stdout[-3000:]
    assert out.stdout.count(" across 2^") == 12 and "NOT CROSSED" not in out.stdout
