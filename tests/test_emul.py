"""CPU tier: the engine's schedule (rings, block anchoring, per-call ranges) and the kernels' index
arithmetic, exercised WITHOUT a GPU by tests/emul/ (the same r8b_kernel_phases.h run thread by
thread on the host; test infrastructure, not part of the product) and compared with the oracle.
The GPU tier (test_gpu_parity.py) repeats these cases on the real HIP path."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import cases
import r8b_oracle as O
from cases import (STREAM_CASES, SHORT_CASES, REBLOCK_CASES, SPLIT_CASES, SOLO_CASES, MINPHASE_CASES, MINPHASE_LONG_CASES, PAIR_SCALE_CASES, PARK_CASES, PARK_CASES_MINPHASE, RMS_TOL,
                   PEAK_TOL, compare_stream, make_input, check_pair_scales, check_parked_outputs)
from conftest import ROOT

r8b = importlib.import_module("r8brain-free-src_amd")


@pytest.fixture(scope="module")
def emul():
    return cases.emul_lib(test_hooks=True)


@pytest.mark.parametrize("case", STREAM_CASES)
def test_emulated_engine_matches_oracle(emul, case):
    src, dst, maxin, chunk, n, tb, att = case
    b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=2, lib=emul)
    rms, pk = compare_stream(b, src, dst, maxin, chunk, n, tb, att, 2)
    assert rms <= RMS_TOL and pk <= PEAK_TOL, (rms, pk)


@pytest.mark.parametrize("nch", [3, 2])
@pytest.mark.parametrize("case", SHORT_CASES)
def test_emulated_short_filters_in_block_groups(emul, case, nch):
    """shorter filters: the pair kernel with 2 ... 16 blocks per workgroup (r8b_convp.h); odd channel
    count = the last channel without a partner"""
    src, dst, maxin, chunk, n, tb, att, frag = case
    b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=nch, lib=emul)
    assert frag in b.describe(), b.describe()
    b.set_option("timing", 1)
    assert any(t[0].startswith("k_convp") for t in b.stage_timings()), b.stage_timings()
    b.set_option("timing", 0)
    rms, pk = compare_stream(b, src, dst, maxin, chunk, n, tb, att, nch)
    assert rms <= RMS_TOL and pk <= PEAK_TOL, (rms, pk)


@pytest.mark.parametrize("case", PAIR_SCALE_CASES)
def test_emulated_pair_partner_scales_and_silence(emul, case):
    """channel scales 1 : 1e-6, 1e-12 : 1 and 1 : 0 across a pair of the pair kernel -- every channel within RMS 1e-15 /
    peak 1e-13 of ITS OWN level (round 6: partners equalised per block by an exact power of two), exact zeros for silent
    channels whatever the partner carries (cases.check_pair_scales)"""
    src, dst, maxin, chunk, n, tb, att = case
    b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=9, lib=emul)
    rel_rms, rel_pk = check_pair_scales(b, case)
    assert rel_rms <= RMS_TOL and rel_pk <= PEAK_TOL


def run_poly_channel_groups(lib_kw):
    """convolver + polynomial interpolator walked in channel groups (Engine::process, option poly_groups): same
    samples bit for bit, same per-stage counts, more launches"""
    x = make_input(10, 6000, 3)

    def run(cap):
        b = r8b.BatchResampler(44100.0, 44101.0, 1024, 2.0, 180.15, nch=10, **lib_kw)
        b.set_option("poly_groups", cap)
        b.set_option("timing", 1)
        y = np.concatenate([b.process_host(x[:, i:i + 700]) for i in range(0, 6000, 700)], axis=1)
        return y, b.stage_timings()

    y0, t0 = run(0)
    y1, t1 = run(30)   # 30 KB between the stages per group: three groups of four / four / two channels
    assert np.array_equal(y0, y1) and y0.shape[1] > 0
    assert [t[0] for t in t0] == [t[0] for t in t1] == ["k_convp", "k_poly"]
    assert [t[2] for t in t1] == [3 * t[2] for t in t0]
    assert [(t[3], t[4]) for t in t0] == [(t[3], t[4]) for t in t1]


def test_emulated_poly_channel_groups(emul):
    run_poly_channel_groups({"lib": emul})


def exact_block_ratio(src, dst):
    """the ratios whose convolver decimates by 2^k in the SPECTRUM (reference CDSPBlockConvolver.h:329-344): the
    truncation residue depends on the block length, so they keep the reference's own 32768-point block (k_conv_big:
    forward array in global memory) instead of running the filter on 16384-point blocks"""
    return (src, dst) in ((32000.0, 48000.0), (64000.0, 48000.0))


@pytest.mark.parametrize("case", REBLOCK_CASES)
def test_emulated_long_filters_on_shorter_blocks(emul, refwrap, case):
    """radix-3 convolvers whose reference block is 32768 points: same filter on 16384-point
    blocks where overlap-save is exact for any block length (3/1, 1/3, 2/3), the reference's own block where it
    decimates in the spectrum (3/2, 3/4); per-call counts equal the reference's, samples to the usual tolerance"""
    src, dst, maxin, chunk, n, tb, att, rtol, ptol = case
    b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=2, lib=emul)
    assert "fft=32768" in b.describe() or "/32768" in b.describe()   # describes the reference's block
    b.set_option("timing", 1)
    x = make_input(2, n, 5)
    lens, ys, counts, pos = [], [], [], 0
    while pos < n:
        l = min(chunk, n - pos)
        y = b.process_host(x[:, pos:pos + l])
        lens.append(l)
        counts.append(y.shape[1])
        ys.append(y)
        pos += l
    r, p = refwrap.batch_check(src, dst, maxin, lens, x, np.concatenate(ys, axis=1), counts, tb, att)
    assert r.max() <= rtol and p.max() <= ptol, (r.max(), p.max())
    names = [t[0] for t in b.stage_timings()]
    assert (names == ["k_conv"]) == exact_block_ratio(src, dst), names


def run_exact_block_chunk_invariance(lib_kw, src, dst, maxin, tb):
    """the reference's 32768-point blocks (generic kernel, forward array in global memory; history by the copy kernel):
    ragged calls and checkpoints into fresh objects equal MaxInLen calls bit for bit, odd channel count"""
    n = maxin * 9 + 777
    x = make_input(3, n, 33)
    a = r8b.BatchResampler(src, dst, maxin, tb, 180.15, nch=3, **lib_kw)
    ya = np.concatenate([a.process_host(x[:, i:i + maxin]) for i in range(0, n, maxin)], axis=1)
    lens = [maxin, 1, 3, maxin // 2 + 7, 1, maxin, 17, maxin - 9, 40, maxin, 1, maxin // 3]
    b = r8b.BatchResampler(src, dst, maxin, tb, 180.15, nch=3, **lib_kw)
    ys, pos, k = [], 0, 0
    while pos < n:
        l = min(lens[k % len(lens)], n - pos)
        ys.append(b.process_host(x[:, pos:pos + l]))
        pos += l
        k += 1
        if k in (2, 5, 9):
            blob = b.state_dict()
            b = r8b.BatchResampler(src, dst, maxin, tb, 180.15, nch=3, **lib_kw)
            b.process_host(x[:, :333] * 0.25)
            b.load_state_dict(blob)
    yb = np.concatenate(ys, axis=1)
    assert ya.shape == yb.shape and ya.shape[1] > 0 and np.array_equal(ya, yb)


@pytest.mark.parametrize("src,dst,maxin,tb", [(32000.0, 48000.0, 5000, 0.5), (64000.0, 48000.0, 7000, 0.6)])
def test_emulated_exact_block_chunk_invariance(emul, src, dst, maxin, tb):
    run_exact_block_chunk_invariance({"lib": emul}, src, dst, maxin, tb)


def run_split_form_case(lib_kw, case, split, nch=3):
    """8192 -> 16384-point blocks on the pair kernel's split 2x up-sampling form (default) and on the one-channel
    kernel (option pair_split = 0): the same stream to the same tolerance, odd channel count"""
    src, dst, maxin, chunk, n, tb, att = case
    b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=nch, **lib_kw)
    assert "fft=8192/16384" in b.describe() or "fft=16384/32768" in b.describe(), b.describe()
    b.set_option("pair_split", split)
    b.set_option("timing", 1)
    names = [t[0] for t in b.stage_timings()]
    assert any(t.startswith("k_convp") for t in names) == bool(split), names
    assert any(t.startswith("k_convx") for t in names) == (not split), names
    b.set_option("timing", 0)
    r, p = compare_stream(b, src, dst, maxin, chunk, n, tb, att, nch)
    assert r <= RMS_TOL and p <= PEAK_TOL, (r, p)


@pytest.mark.parametrize("split", [1, 0])
@pytest.mark.parametrize("case", SPLIT_CASES)
def test_emulated_split_upsampling_form(emul, case, split):
    run_split_form_case({"lib": emul}, case, split)


def run_solo_form_case(lib_kw, case, solo, nch=3):
    """16384-point blocks on the pair kernel's one-channel form (default) and on the one-channel kernel (option
    pair_solo = 0): the same stream to the same tolerance, odd channel count"""
    src, dst, maxin, chunk, n, tb, att = case[:7]
    rtol, ptol = case[7:9] if len(case) > 7 else (RMS_TOL, PEAK_TOL)
    b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=nch, **lib_kw)
    assert "fft=16384/" in b.describe() or "fft=32768/" in b.describe(), b.describe()
    b.set_option("pair_solo", solo)
    b.set_option("timing", 1)
    names = [t[0] for t in b.stage_timings()]
    assert any(t.startswith("k_convx") for t in names) == (not solo), names
    assert any(t.startswith("k_convp") for t in names) or not solo, names
    b.set_option("timing", 0)
    r, p = compare_stream(b, src, dst, maxin, chunk, n, tb, att, nch)
    assert r <= rtol and p <= ptol, (r, p)


@pytest.mark.parametrize("solo", [1, 0])
@pytest.mark.parametrize("case", SOLO_CASES)
def test_emulated_one_channel_form(emul, case, solo):
    run_solo_form_case({"lib": emul}, case, solo)


MINPHASE_PAIR_TOPOLOGIES = [(44100.0, 96000.0, 2.0, 180.15), (96000.0, 44100.0, 5.0, 109.56),
                            (88200.0, 44100.0, 2.0, 180.15), (176400.0, 44100.0, 20.0, 80.0),
                            (44100.0, 132300.0, 5.0, 109.56), (48000.0, 32000.0, 2.0, 180.15),
                            (32000.0, 48000.0, 20.0, 80.0), (64000.0, 48000.0, 5.0, 109.56)]


def run_minphase_pair_vs_generic(lib_kw, topo):
    src, dst, tb, att = topo
    x = make_input(3, 24000, 9)
    ys = []
    for pair in (1, 0):
        b = r8b.BatchResampler(src, dst, 4096, tb, att, nch=3, phase=1, **lib_kw)
        b.set_option("pair_conv", pair)
        b.set_option("timing", 1)
        names = [t[0] for t in b.stage_timings()]
        assert any(n.startswith("k_convp") for n in names) == bool(pair), names
        b.set_option("timing", 0)
        ys.append(np.concatenate([b.process_host(x[:, i:i + 3000]) for i in range(0, 24000, 3000)], axis=1))
    assert ys[0].shape == ys[1].shape and ys[0].shape[1] > 1000
    assert np.abs(ys[0] - ys[1]).max() <= 5e-15, np.abs(ys[0] - ys[1]).max()


@pytest.mark.parametrize("topo", MINPHASE_PAIR_TOPOLOGIES)
def test_emulated_minphase_pair_kernel_vs_generic(emul, topo):
    """complex kernel spectrum (minimum phase) on the pair kernel -- 1:1, 2x up, decimating incl. the
    Nyquist fix-up, radix-3 edges -- against the generic kernel (which the loose reference tolerance of
    the minimum-phase cases cannot pin): the same samples to rounding"""
    run_minphase_pair_vs_generic({"lib": emul}, topo)


MINPHASE_NOISE_FACTOR = 3.0


def run_minphase_case(lib_kw, refwrap, case):
    """Minimum-phase chain with THIS library's designer against the compiled reference.  Per-call counts and the
    latency queries must be equal.  Samples cannot be: the cepstral transform that derives the filter amplifies the
    rounding noise of the FFT that computes it (reference CDSPRealFFT.h:681-785), so two correct builds of the
    REFERENCE differ as well -- the bound is therefore the reference's own noise, measured in the same run: the
    stream of the reference over its other FFT back-end (oracle/_ref/libr8bref_pffft.so, -DR8B_PFFFT_DOUBLE=1) against
    the default (Ooura) build, times MINPHASE_NOISE_FACTOR.  Both sides are single draws of that noise: on the twelve
    cases |ours - Ooura| / |PFFFT - Ooura| comes out between 0.41 and 2.64 (RMS and peak alike; 0.79 for most).
    Without the PFFFT build (no AVX on the host) the hand-entered tolerances of cases.MINPHASE_CASES are used."""
    src, dst, maxin, chunk, n, tb, att, rtol, ptol = case
    b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=2, phase=1, **lib_kw)
    x = make_input(2, n, 5)
    lens, ys, counts, pos = [], [], [], 0
    while pos < n:
        l = min(chunk, n - pos)
        y = b.process_host(x[:, pos:pos + l])
        lens.append(l)
        counts.append(y.shape[1])
        ys.append(y)
        pos += l
    y = np.concatenate(ys, axis=1)
    # raises if any call's count differs from the reference's
    r, p = refwrap.batch_check(src, dst, maxin, lens, x, y, counts, tb, att, phase=1)
    assert sum(counts) > 0
    pf = refwrap.pffft_lib()
    if pf is None:
        assert r.max() <= rtol and p.max() <= ptol, (r.max(), p.max())
    else:
        for c in range(2):
            yp = refwrap.RefResampler(src, dst, maxin, tb, att, phase=1, backend=pf).stream(x[c], chunk)
            assert len(yp) == y.shape[1]
            rn, pn = refwrap.batch_check(src, dst, maxin, lens, x[c:c + 1], yp[None, :], counts, tb, att, phase=1)
            assert rn[0] > 0.0
            assert r[c] <= MINPHASE_NOISE_FACTOR * rn[0] and p[c] <= MINPHASE_NOISE_FACTOR * pn[0], \
                (c, r[c], rn[0], p[c], pn[0])
    # the reference's bookkeeping queries see the same latencies
    ref = refwrap.RefResampler(src, dst, maxin, tb, att, phase=1)
    for q in (0, 1, 17, 1000):
        assert b.getInLenBeforeOutPos(q) == ref.inlen_before_outpos(q)


class reference_minphase_taps:
    """context: while active, the library's low-pass designer takes MINIMUM-PHASE filters from the compiled reference
    (taps recovered from its kernel block, refwrap.lpfilter_taps) through the parity-test hook
    r8b_design_set_lp_provider -- the kernels then run on the reference's own filter, so that the stream
    comparison measures the kernels and the fractional-latency plumbing, not the cepstral transform's conditioning"""

    def __init__(self, lib, refwrap):
        from importlib import import_module
        capi = import_module("r8brain-free-src_amd._capi")
        self.lib, self.calls = lib, []

        def provide(nf, tb, att, gain, phase, taps, cap, lat, latfrac, bits):
            if phase != 1:
                return 0
            t, la, lf = refwrap.lpfilter_taps(nf, tb, att, gain, 1)
            n = len(t)
            assert n <= cap
            for i in range(n):
                taps[i] = t[i]
            lat[0], latfrac[0] = la, lf
            b = 1
            while (1 << b) < n:   # CDSPFIRFilter::getBlockLenBits = getBitOccupancy(KernelLen - 1)
                b += 1
            bits[0] = max(1, int(n - 1).bit_length())
            self.calls.append((nf, tb, att, gain, n, la, lf))
            return n

        self.cb = capi.LP_PROVIDER(provide)

    def __enter__(self):
        import ctypes as C
        self.lib.r8b_design_set_lp_provider(C.cast(self.cb, C.c_void_p))
        return self

    def __exit__(self, *a):
        self.lib.r8b_design_set_lp_provider(None)


def run_minphase_reference_taps(lib, lib_kw, refwrap, case):
    src, dst, maxin, chunk, n, tb, att = case[:7]
    with reference_minphase_taps(lib, refwrap) as prov:
        b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=2, phase=1, **lib_kw)
        assert prov.calls, "the provider was not consulted"
        x = make_input(2, n, 5)
        lens, ys, counts, pos = [], [], [], 0
        while pos < n:
            l = min(chunk, n - pos)
            y = b.process_host(x[:, pos:pos + l])
            lens.append(l)
            counts.append(y.shape[1])
            ys.append(y)
            pos += l
        r, p = refwrap.batch_check(src, dst, maxin, lens, x, np.concatenate(ys, axis=1), counts, tb, att, phase=1)
        # One stated exception: 64000 -> 48000 decimates by 4 in the spectrum behind a latency that is not a multiple
        # of 4; the reference then delays its input by InputDelay samples (CDSPBlockConvolver.h:131-138), which moves
        # its blocks against ours, and with them the -219 dB residue of the spectrum truncation.
        rt, pt = (3e-12, 2e-10) if (src, dst) == (64000.0, 48000.0) else (RMS_TOL, PEAK_TOL)
        assert sum(counts) > 0 and r.max() <= rt and p.max() <= pt, (r.max(), p.max())
        ref = refwrap.RefResampler(src, dst, maxin, tb, att, phase=1)
        for q in (0, 1, 17, 1000):
            assert b.getInLenBeforeOutPos(q) == ref.inlen_before_outpos(q)


@pytest.mark.parametrize("case", MINPHASE_CASES)
def test_emulated_minimum_phase_kernels_on_reference_taps(emul, refwrap, case):
    """the minimum-phase chains with the REFERENCE's own minimum-phase taps (parity-test hook): complex
    kernel spectrum (pair-kernel modes 6 / 7), fractional-latency plumbing through every stage kind -- at the path's
    tolerance, RMS <= 1e-15 / peak <= 1e-13.  What remains loose in MINPHASE_CASES is the designer's conditioning only."""
    run_minphase_reference_taps(emul, {"lib": emul}, refwrap, case)


@pytest.mark.parametrize("case", MINPHASE_LONG_CASES)
def test_emulated_minimum_phase_long_blocks_on_reference_taps(emul, refwrap, case):
    """cases.MINPHASE_LONG_CASES: the split and one-channel forms of the pair kernel with a complex kernel spectrum"""
    src, dst, maxin, chunk, n, tb, att = case
    b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=2, phase=1, lib=emul)
    b.set_option("timing", 1)
    assert any(t[0].startswith("k_convp") for t in b.stage_timings()), b.stage_timings()
    run_minphase_reference_taps(emul, {"lib": emul}, refwrap, case)


def test_minimum_phase_latency_split_matches_reference(emul, refwrap):
    """the designer's group-delay split (integer Latency / LatencyFrac) against the reference's for the
    filters of the presets -- an integer-boundary disagreement would shift a whole stream by one sample"""
    import ctypes as C
    bb, la, lf = C.c_int(), C.c_int(), C.c_double()
    for nf, tb, att, gain in ((0.5, 2.0, 180.15, 2.0), (0.5, 2.0, 136.45, 2.0), (0.5, 2.0, 109.56, 2.0),
                              (0.459375, 2.0, 180.15, 1.0), (0.25, 2.0, 180.15, 0.5), (1.0 / 3.0, 2.0, 180.15, 3.0),
                              (0.5, 5.0, 109.56, 2.0), (0.5, 0.5, 109.56, 2.0)):
        emul.r8b_design_lpfilter_ex(nf, tb, att, gain, 1, bb, la, lf, None, 0)
        _, rla, rlf = refwrap.lpfilter_taps(nf, tb, att, gain, 1)
        assert la.value == rla, (nf, tb, att, la.value, rla)
        assert abs(lf.value - rlf) < 0.02, (nf, tb, att, lf.value, rlf)   # (1/3-band at 180 dB: 0.011 samples)


LATFRAC_TOPOLOGIES = [(44100.0, 88200.0), (44100.0, 96000.0), (96000.0, 44100.0), (44100.0, 44101.0),
                      (44100.0, 176400.0), (176400.0, 44100.0), (88200.0, 44100.0), (44100.0, 192000.0),
                      (64000.0, 48000.0), (48000.0, 32000.0)]


def check_latency_frac(lib, lib_kw, refwrap, provider):
    """CDSPResampler::getLatencyFrac (reference CDSPResampler.h:491-494, 688: what the chain's LAST stage reports).
    Linear phase: exactly 0.0, as the reference.  Minimum phase on the REFERENCE's own taps (test-build hook): the
    chain's bookkeeping alone is compared -- equal to 1e-9; with this library's designer the filter's own group-delay
    fraction differs by up to 0.011 samples (test_minimum_phase_latency_split_matches_reference), scaled by the
    chain's rate ratio."""
    for src, dst in LATFRAC_TOPOLOGIES:
        lin = r8b.BatchResampler(src, dst, 1024, 2.0, 180.15, nch=1, **lib_kw)
        assert lin.getLatencyFrac() == 0.0 == refwrap.RefResampler(src, dst, 1024, 2.0, 180.15).latency_frac()
        want = refwrap.RefResampler(src, dst, 1024, 2.0, 180.15, phase=1).latency_frac()
        own = r8b.BatchResampler(src, dst, 1024, 2.0, 180.15, nch=1, phase=1, **lib_kw).getLatencyFrac()
        assert abs(own - want) < 0.02 * max(1.0, dst / src), (src, dst, own, want)
        if provider is not None:
            with provider as prov:
                got = r8b.BatchResampler(src, dst, 1024, 2.0, 180.15, nch=1, phase=1, **lib_kw).getLatencyFrac()
                assert prov.calls
            assert abs(got - want) < 1e-9, (src, dst, got, want)
    # the Python mirror of the front-end class
    m = r8b.CDSPResampler(44100.0, 96000.0, 1024, 2.0, 180.15, ReqPhase=1, **lib_kw)
    assert m.getLatencyFrac() == r8b.BatchResampler(44100.0, 96000.0, 1024, 2.0, 180.15, nch=1, phase=1,
                                                    **lib_kw).getLatencyFrac() != 0.0


def test_emulated_latency_frac_matches_reference(emul, refwrap):
    check_latency_frac(emul, {"lib": emul}, refwrap, reference_minphase_taps(emul, refwrap))


@pytest.mark.parametrize("case", MINPHASE_CASES)
def test_emulated_minimum_phase_chains(emul, refwrap, case):
    """fprMinPhase: counts and latency bookkeeping equal the reference's, samples
    to the stated (reference-noise limited) tolerance"""
    run_minphase_case({"lib": emul}, refwrap, case)


def test_minimum_phase_filter_is_what_it_claims(emul):
    """independent of the reference's noise: same magnitude response as the linear-phase kernel, DC
    gain as requested, causal with the energy up front"""
    import ctypes as C
    bb, la, lf = C.c_int(), C.c_int(), C.c_double()
    dp = C.POINTER(C.c_double)
    for nf, gain in ((0.5, 2.0), (1.0 / 3.0, 2.0), (0.459375, 1.0)):
        n = emul.r8b_design_lpfilter_ex(nf, 2.0, 180.15, gain, 1, bb, la, lf, None, 0)
        tm, tl = np.zeros(n), np.zeros(n)
        emul.r8b_design_lpfilter_ex(nf, 2.0, 180.15, gain, 1, bb, la, lf, tm.ctypes.data_as(dp), n)
        emul.r8b_design_lpfilter_ex(nf, 2.0, 180.15, gain, 0, bb, None, None, tl.ctypes.data_as(dp), n)
        assert abs(tm.sum() - gain) < 1e-12
        N = 1 << 18
        hm, hl = np.abs(np.fft.rfft(tm, N)), np.abs(np.fft.rfft(tl, N))
        band = slice(0, int(N / 2 * nf * 0.8))
        assert np.abs(hm[band] / hl[band] - 1.0).max() < 2e-5
        assert np.abs(hm[int(N / 2 * nf * 1.1):]).max() < 1e-8 * gain      # still a 180 dB stop band
        e = np.cumsum(tm * tm) / np.sum(tm * tm)
        assert e[n // 8] > 0.98 and e[4 * la.value + 8] > 0.85 and e[n // 4] > 0.998   # energy up front
        el = np.cumsum(tl * tl) / np.sum(tl * tl)
        assert el[n // 4] < 1e-6                                            # (the linear-phase kernel: centred)
        assert 0.0 <= lf.value < 1.0 and 0 < la.value < n // 8


@pytest.mark.parametrize("radix,threads", [(2, 64), (4, 256), (16, 128)])
def test_emulated_transform_plans(emul, radix, threads):
    """every radix mix of the in-LDS FFT gives the same stream"""
    src, dst, maxin, chunk, n, tb, att = STREAM_CASES[0]
    b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=1, lib=emul)
    b.set_option("conv_radix", radix)
    b.set_option("conv_threads", threads)
    rms, pk = compare_stream(b, src, dst, maxin, chunk, n, tb, att, 1)
    assert rms <= RMS_TOL and pk <= PEAK_TOL, (rms, pk)


def test_emulated_chunk_invariance_is_bitwise(emul):
    """blocks are anchored to absolute stream positions, so -- like the reference --
    the stream does not depend on how the input is cut into calls"""
    x = make_input(1, 9000, 11)
    ref = None
    for chunk in (1024, 1000, 777, 64):
        b = r8b.BatchResampler(44100.0, 96000.0, 1024, 2.0, 180.15, nch=1, lib=emul)
        y = np.concatenate([b.process_host(x[:, i:i + chunk])[0] for i in range(0, 9000, chunk)])
        if ref is None:
            ref = y
        else:
            assert np.array_equal(y, ref)


def test_emulated_clear(emul):
    x = make_input(2, 5000, 5)
    b = r8b.BatchResampler(96000.0, 44100.0, 1024, 2.0, 180.15, nch=2, lib=emul)
    y1 = np.concatenate([b.process_host(x[:, i:i + 1000]) for i in range(0, 5000, 1000)], axis=1)
    b.clear()
    y2 = np.concatenate([b.process_host(x[:, i:i + 1000]) for i in range(0, 5000, 1000)], axis=1)
    assert np.array_equal(y1, y2)


def test_emulated_dll_abi(emul):
    """r8b_create ... r8b_process called the way a C host calls the reference DLL"""
    x = O.splitmix_uniform(9, 4096)
    d = r8b.DLLResampler(44100.0, 96000.0, 1024, 2.0, r8b.DLLResampler.r8brr24, lib=emul)
    o = O.OracleResampler(44100.0, 96000.0, 1024, 2.0, 180.15)
    assert d.inlen(1) == o.input_required(1)
    for i in range(0, 4096, 1024):
        a = d.process(x[i:i + 1024])
        b = o.process(x[i:i + 1024])
        assert len(a) == len(b)
        if len(a):
            assert np.abs(a - b).max() <= PEAK_TOL
    d.clear()
    assert len(d.process(x[:1024])) == 0


@pytest.mark.parametrize("opts", [{"pair_conv": 0}, {"pair_conv": 0, "fuse": 0}, {"pair_two": 0},
                                  {"fuse": 0}])
@pytest.mark.parametrize("case", [STREAM_CASES[0], STREAM_CASES[1], STREAM_CASES[6], STREAM_CASES[13]])
def test_emulated_alternative_fast_paths(emul, case, opts):
    """the forms behind the engine options: one-channel fast path (r8b_convx.h) instead of the pair
    kernel (r8b_convp.h), one phase per thread instead of two, unfused"""
    src, dst, maxin, chunk, n, tb, att = case
    b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=2, lib=emul)
    for k, v in opts.items():
        b.set_option(k, v)
    b.set_option("timing", 1)
    names = [t[0] for t in b.stage_timings()]
    if opts.get("pair_conv", 1) == 0:
        assert not any(t.startswith("k_convp") for t in names), names
    b.set_option("timing", 0)
    rms, pk = compare_stream(b, src, dst, maxin, chunk, n, tb, att, 2)
    assert rms <= RMS_TOL and pk <= PEAK_TOL, (rms, pk)


def test_unsupported_geometry_fails_loudly(emul):
    """Every filter the reference accepts (transition band >= 0.5 %, attenuation <= 218 dB) is
    supported (tests above: the longest ones on shorter blocks); OUTSIDE the reference's parameter
    range a filter that cannot fit a workgroup's LDS must fail at creation with a message, not fall
    back to anything."""
    r8b.BatchResampler(32000.0, 96000.0, 1024, 0.5, 218.0, nch=1, lib=emul)   # longest radix-3 case
    with pytest.raises(RuntimeError, match="too long"):
        r8b.BatchResampler(64000.0, 48000.0, 1024, 0.2, 218.0, nch=1, lib=emul)
    # minimum phase: the longest blocks -- 2x up-sampling, 1:1 and 2x decimating at 16384 points -- run on the pair
    # kernel's long-block forms with a complex spectrum (round 4; refused or on the generic kernel in place before)
    for src, dst in ((44100.0, 88200.0), (96000.0, 44100.0), (88200.0, 44100.0), (32000.0, 48000.0), (48000.0, 32000.0)):
        r8b.BatchResampler(src, dst, 1024, 0.5, 218.0, nch=1, phase=1, lib=emul)
    with pytest.raises(RuntimeError, match="too long"):
        r8b.BatchResampler(64000.0, 48000.0, 1024, 0.2, 218.0, nch=1, phase=1, lib=emul)


CKPT_CASES = [(44100.0, 96000.0), (96000.0, 44100.0), (44100.0, 44101.0), (44100.0, 2822400.0),
              (176400.0, 44100.0), (48000.0, 32000.0)]


def checkpoint_roundtrip(make, src, dst):
    """Stream A runs straight through; stream B is checkpointed mid-way, the blob is loaded into
    a fresh object C, and C's continuation must equal A's bit for bit."""
    nch, chunk, n = 3, 700, 700 * 9
    x = make_input(nch, n)
    a, b, c = make(), make(), make()
    ya = [a.process_host(x[:, i:i + chunk]) for i in range(0, n, chunk)]
    for i in range(0, 4 * chunk, chunk):
        b.process_host(x[:, i:i + chunk])
    blob = b.state_dict()
    c.process_host(x[:, :chunk] * 0.5)  # c has seen unrelated input before the load
    c.load_state_dict(blob)
    for k, i in enumerate(range(4 * chunk, n, chunk)):
        yc = c.process_host(x[:, i:i + chunk])
        assert yc.shape == ya[4 + k].shape and np.array_equal(yc, ya[4 + k]), (src, dst, k)
    return blob


@pytest.mark.parametrize("src,dst", CKPT_CASES)
def test_emulated_checkpoint_resume(emul, src, dst):
    checkpoint_roundtrip(lambda: r8b.BatchResampler(src, dst, 700, 2.0, 136.45, nch=3, lib=emul),
                         src, dst)


@pytest.mark.parametrize("src,dst", [(44100.0, 96000.0), (44100.0, 88200.0), (88200.0, 44100.0), (48000.0, 32000.0)])
def test_emulated_checkpoint_resume_on_the_half_array_forms(emul, src, dst):
    """... on kernel modes 23 / 21 / 27 / 22 (options half = 2, half_fused = 2: forced on the small batch); the forms keep
    the state where the full-array kernels keep it, a blob is bound to the options all the same (they round differently on
    the device), and the options are refused once the stream has started"""
    def make(h=2):
        b = r8b.BatchResampler(src, dst, 700, 2.0, 180.15, nch=3, lib=emul)
        b.set_option("half", h)
        b.set_option("half_fused", h)
        return b
    blob = checkpoint_roundtrip(make, src, dst)
    with pytest.raises(RuntimeError, match="differently configured"):
        make(0).load_state_dict(blob)
    b = make()
    b.process_host(make_input(3, 700))
    with pytest.raises((KeyError, RuntimeError)):
        b.set_option("half", 0)
    b.clear()
    b.set_option("half", 0)


def test_emulated_checkpoint_rejects_other_configuration(emul):
    a = r8b.BatchResampler(44100.0, 96000.0, 700, 2.0, 136.45, nch=3, lib=emul)
    a.process_host(make_input(3, 700))
    blob = a.state_dict()
    for other in (r8b.BatchResampler(44100.0, 96000.0, 700, 2.0, 136.45, nch=2, lib=emul),
                  r8b.BatchResampler(44100.0, 88200.0, 700, 2.0, 136.45, nch=3, lib=emul)):
        with pytest.raises(RuntimeError, match="differently configured|ring size"):
            other.load_state_dict(blob)
    with pytest.raises(RuntimeError, match="truncated|wrong size"):
        a.load_state_dict(blob[:100])


# ---- hardening of the batch ABI (engine logic, exercised through the emulation library) ----------

def test_emulated_state_blob_is_validated_before_anything_changes(emul):
    x = make_input(2, 6000, 17)
    b = r8b.BatchResampler(44100.0, 96000.0, 1024, 2.0, 180.15, nch=2, lib=emul)
    size0 = emul.r8b_batch_state_size(b._h)
    b.process_host(x[:, :1024])
    b.process_host(x[:, 1024:2048])
    assert emul.r8b_batch_state_size(b._h) == size0      # a constant of the object
    blob = b.state_dict()
    assert blob.size == size0
    y_next = b.process_host(x[:, 2048:3072])
    # a truncated blob and a blob with impossible counters are refused as a whole ...
    c = r8b.BatchResampler(44100.0, 96000.0, 1024, 2.0, 180.15, nch=2, lib=emul)
    c.process_host(x[:, :1024])
    keep = c.state_dict()
    with pytest.raises(RuntimeError):
        c.load_state_dict(blob[:-8])
    bad = blob.copy()
    bad[32:40] = 255                                       # first stage counter m = -1
    with pytest.raises(RuntimeError):
        c.load_state_dict(bad)
    assert np.array_equal(c.state_dict(), keep)            # ... and leave the object untouched
    # the intact blob resumes bit-identically
    c.load_state_dict(blob)
    assert np.array_equal(c.process_host(x[:, 2048:3072]), y_next)


def test_emulated_structural_options_are_frozen_while_a_stream_runs(emul):
    x = make_input(1, 3000, 19)
    b = r8b.BatchResampler(44100.0, 96000.0, 1024, 2.0, 180.15, nch=1, lib=emul)
    b.set_option("fuse", 0)          # before the first sample: fine
    b.set_option("fuse", 1)
    b.process_host(x[:, :1024])
    with pytest.raises(KeyError):
        b.set_option("fuse", 0)      # would move the history to rings the fused kernel never wrote
    b.set_option("fuse", 1)          # unchanged value: fine
    b.set_option("timing", 0)        # non-structural: fine
    b.clear()
    b.set_option("fuse", 0)          # after clear(): fine again
    # "park" decides where the outputs behind a call's last block live (park buffer / ahead in a ring): structural too
    c = r8b.BatchResampler(44100.0, 96000.0, 1024, 2.0, 180.15, nch=1, lib=emul)
    c.process_host(x[:, :1024])
    with pytest.raises(KeyError):
        c.set_option("park", 0)
    c.set_option("park", 1)
    c.process_host(x[:, 1024:2048])
    c.process_host(x[:, 2048:3000])
    # counters: known names only
    assert c.stat("conv_blocks") > 0 and c.stat("park_only_calls") == 0
    with pytest.raises(KeyError):
        c.stat("no_such_counter")
    # a checkpoint of an object with parked outputs is refused by an object that does not park (other option set)
    d = r8b.BatchResampler(44100.0, 96000.0, 1024, 2.0, 180.15, nch=1, lib=emul)
    d.set_option("park", 0)
    with pytest.raises(RuntimeError, match="differently configured"):
        d.load_state_dict(c.state_dict())


# every structural option (frozen once a stream has started): (default, another value) ...
STRUCTURAL_OPTIONS = {"fuse": (1, 0), "fuse_hb": (1, 0), "fuse_hbd": (2, 0), "fuse_hbconv": (0, 1), "fold_tail": (1, 0),
                      "fast_conv": (1, 0), "pair_conv": (1, 0), "pair_two": (1, 0), "pair_split": (1, 0),
                      "pair_solo": (1, 0), "align_groups": (1, 0), "park": (1, 0), "fuse_latency": (1, 0),
                      "solo_fuse": (1, 0), "up3_poly": (1, 0), "half": (1, 0), "half_fused": (1, 0), "quad": (0, 1),
                      "form_channels": (0, 130)}
# ... and every other option with its default
FREE_OPTIONS = {"conv_radix": 8, "conv_threads": 256, "whole_tile": 4096, "hb_tile": 1024, "hbd_span": 2048,
                "hbc_tile": 0, "timing": 0, "poly_tiled": 1, "poly_groups": 0, "walk": 1, "walk_len": 0}


def test_emulated_every_option_is_frozen_or_free_as_listed(emul):
    b = r8b.BatchResampler(44100.0, 96000.0, 700, 2.0, 136.45, nch=3, lib=emul)
    with pytest.raises(KeyError):
        b.set_option("no_such_option", 0)
    b.process_host(make_input(3, 700))
    for name, (default, other) in STRUCTURAL_OPTIONS.items():
        with pytest.raises(KeyError):
            b.set_option(name, other)
        b.set_option(name, default)      # unchanged value: fine
    for name, default in FREE_OPTIONS.items():
        b.set_option(name, default)
    with pytest.raises(KeyError):
        b.set_option("no_such_option", 0)
    b.clear()
    for name, (default, other) in STRUCTURAL_OPTIONS.items():
        b.set_option(name, other)        # after clear(): fine


def config_field(b):
    """the configuration hash in a checkpoint's header (bytes 8:16 of the blob, after the magic)"""
    return int.from_bytes(b.state_dict()[8:16].tobytes(), "little")


def test_emulated_checkpoint_config_hash_is_pinned(emul):
    """Blobs saved by one build must load in another: the hash over the chain and the options (names, values) stays
    what it was (the literals were recorded while the options still lived in a string map).  The default hash covers the
    name and default of every hashed option at once."""
    def hashed(**opts):
        b = r8b.BatchResampler(44100.0, 96000.0, 700, 2.0, 136.45, nch=3, lib=emul)
        for k, v in opts.items():
            b.set_option(k, v)
        return config_field(b)
    assert hashed() == 0xe731cb8350f3f105
    assert hashed(half=0, half_fused=0) == 0xaf158f58abe77d27
    assert hashed(form_channels=130) == 0x7b1b53137ff92831
    # (options that change neither the state nor a bit of the stream stay out of it)
    assert hashed(timing=1, walk=0, walk_len=3) == hashed()


def test_emulated_every_counter_is_known(emul):
    b = r8b.BatchResampler(44100.0, 96000.0, 700, 2.0, 136.45, nch=3, lib=emul)
    b.process_host(make_input(3, 700))
    for name in ("conv_blocks", "walk_blocks", "tail_launches", "park_calls", "park_only_calls", "pcm_staged_sides",
                 "hbc_tile_8192", "poly_front"):
        assert b.stat(name) >= 0, name
    with pytest.raises(KeyError):
        b.stat("conv_block")


def test_emulated_process_rejects_overlapping_rows_and_null_pointers(emul):
    import ctypes as C
    b = r8b.BatchResampler(44100.0, 96000.0, 1024, 2.0, 180.15, nch=2, lib=emul)
    x = np.zeros((2, 1024))
    y = np.zeros((2, b.max_out_len))
    ok = emul.r8b_batch_process(b._h, x.ctypes.data_as(C.c_void_p), 1024, 1024,
                                y.ctypes.data_as(C.c_void_p), b.max_out_len, None)
    assert ok >= 0
    for args in [(None, 1024, 1024, y.ctypes.data_as(C.c_void_p), b.max_out_len),     # null input
                 (x.ctypes.data_as(C.c_void_p), 1024, 1024, None, b.max_out_len),     # null output
                 (x.ctypes.data_as(C.c_void_p), 1000, 1024, y.ctypes.data_as(C.c_void_p), b.max_out_len),
                 (x.ctypes.data_as(C.c_void_p), 1024, 1024, y.ctypes.data_as(C.c_void_p), 100)]:
        assert emul.r8b_batch_process(b._h, args[0], args[1], args[2], args[3], args[4], None) == -1
        assert emul.r8b_last_error()
    with pytest.raises(Exception):
        r8b.BatchResampler(0, 0, 1024, nch=1, lib=emul, stage=(7, 0.0, 0.0, 0.0, 0.0, 0, 0))


def test_emulated_paired_rows_equal_the_unpaired_row_bitwise(emul):
    """identical data in every channel: the even rows of a batch (real halves of the pair kernel's transforms) equal
    the row of a one-channel object BIT FOR BIT across calls -- whichever of the interpolator's loops (whole groups /
    masked groups) and of the loaders (caller's buffer / history ring) produced an output.  (What
    tests/cxx_batch.cpp checks on the GPU; an order of additions that differs between the two loops shows here.)"""
    L = 2000
    b5 = r8b.BatchResampler(44100.0, 96000.0, L, 2.0, 180.15, nch=5, lib=emul)
    b1 = r8b.BatchResampler(44100.0, 96000.0, L, 2.0, 180.15, nch=1, lib=emul)
    rng = np.random.default_rng(3)
    for c in range(6):
        x = rng.uniform(-1.0, 1.0, L)
        y5 = b5.process_host(np.ascontiguousarray(np.tile(x, (5, 1))))
        y1 = b1.process_host(x[None, :].copy())
        assert y5.shape[1] == y1.shape[1]
        for ch in (0, 2, 4):
            assert np.array_equal(y5[ch], y1[0]), (c, ch)
        for ch in (1, 3):
            assert np.abs(y5[ch] - y1[0]).max() <= 4e-15, (c, ch)


@pytest.mark.parametrize("src,dst,att", [(44100.0, 1411200.0, 49.5), (44100.0, 2822400.0, 50.38), (11025.0, 384000.0, 50.38)])
def test_one_tap_halfband_start_of_stream(emul, refwrap, src, dst, att):
    """Chains that contain a ONE-tap half-band up-sampler (attenuations below ~55 dB with four or more doubling stages).
    The reference's CDSPHBUpsampler reads rp[1] of its ring's overrun area for the stream's first odd output, a slot its
    constructor neither mirrors nor clears when the filter has one tap (CDSPHBUpsampler.h:606-607 flo = fll + fl2 = 1,
    :668-671 nothing cleared, :688-693 one sample mirrored; `double Buf[BufLen + 27]` is an uninitialised member) -- the
    reference's value there is indeterminate.  This library computes the stated filter (= the numpy restatement) for every
    sample; it must agree with the reference everywhere else.  (Found by tools/wide_fuzz.py, round 3.)"""
    maxin, tb = 1024, 1.49
    b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=1, lib=emul)
    assert "taps=1 " in b.describe(), b.describe()
    ref = refwrap.RefResampler(src, dst, maxin, tb, att)
    orc = O.OracleResampler(src, dst, maxin, tb, att)
    x = O.splitmix_uniform(48, 1500)
    pos, seen = 0, 0
    for l in (300, 400, 200, 600):
        y = b.process_host(x[None, pos:pos + l])[0]
        yr, yo = ref.process(x[pos:pos + l]), orc.process(x[pos:pos + l])
        assert len(y) == len(yr) == len(yo)
        if len(y):
            assert np.abs(y - yo).max() <= PEAK_TOL
            bad = np.nonzero(np.abs(y - yr) > PEAK_TOL)[0] + seen
            # (only among the first outputs of the stream: one per one-tap stage, spread by the stages behind it)
            assert len(bad) <= 4 and (len(bad) == 0 or bad.max() < 8), bad
        seen += len(y)
        pos += l
    assert seen > 100


# (src, dst, maxin, transition band): the last four on the split 2x up-sampling form and the one-channel form of the pair kernel
TAIL_TOPOLOGIES = [(44100.0, 96000.0, 8192, 2.0), (96000.0, 44100.0, 16384, 2.0), (88200.0, 44100.0, 12000, 2.0),
                   (44100.0, 88200.0, 6000, 2.0), (48000.0, 32000.0, 16384, 2.0),
                   (44100.0, 88200.0, 9000, 0.5), (96000.0, 44100.0, 16384, 0.5), (88200.0, 44100.0, 12000, 0.5),
                   (48000.0, 16000.0, 30000, 0.5),
                   # (a half-band stage carries the copy: stage 0's own launch, or a later stage's in calls without a block)
                   (176400.0, 44100.0, 16384, 2.0), (192000.0, 44100.0, 8192, 0.5), (44100.0, 2822400.0, 1024, 2.0),
                   (2822400.0, 176400.0, 8192, 2.0)]


@pytest.mark.parametrize("src,dst,maxin,tb", TAIL_TOPOLOGIES)
def test_emulated_history_from_registers_equals_the_copy_kernel(emul, src, dst, maxin, tb):
    """the stream's history for the next call, three ways: stored by the blocks that hold it in registers plus the last
    block's fetch (long calls, r8b_convp.h convp_tail_owners), copied in slices by every block (calls shorter than a
    window) and by a kernel of its own (option fold_tail = 0) -- the outputs are the same BIT FOR BIT, with an odd channel
    count (a block pair without a partner) and calls of every length in between"""
    run_history_three_ways({"lib": emul}, src, dst, maxin, tb)


def run_history_three_ways(lib_kw, src, dst, maxin, tb):
    lens = [min(l, maxin) for l in (maxin, maxin, maxin // 3, 300, maxin, 17, 1, maxin - 5, 2500, maxin)]
    a = r8b.BatchResampler(src, dst, maxin, tb, 180.15, nch=3, **lib_kw)
    b = r8b.BatchResampler(src, dst, maxin, tb, 180.15, nch=3, **lib_kw)
    b.set_option("fold_tail", 0)
    rng = np.random.default_rng(5)
    for i, l in enumerate(lens):
        x = rng.uniform(-1.0, 1.0, (3, l))
        ya, yb = a.process_host(x), b.process_host(x)
        assert ya.shape == yb.shape and np.array_equal(ya, yb), (i, l)
    assert b.stat("tail_launches") == len(lens) and a.stat("tail_launches") < len(lens)


HBCONV_TOPOLOGIES = [(176400.0, 44100.0, 7000), (352800.0, 44100.0, 8192)]


def run_hbconv_fused(lib_kw, refwrap, src, dst, maxin, nch=3):
    """a half-band decimator taken in the load of the decimating convolver behind it (kernel mode 20, option
    fuse_hbconv): one launch instead of two, the SAME samples bit for bit (the decimator's sums in k_hbdown's order),
    over ragged calls, a checkpoint into a fresh object, an odd channel count; and the reference's stream to the usual
    tolerance"""
    a = r8b.BatchResampler(src, dst, maxin, 2.0, 180.15, nch=nch, **lib_kw)
    b = r8b.BatchResampler(src, dst, maxin, 2.0, 180.15, nch=nch, **lib_kw)
    for o in (a, b):
        o.set_option("fuse_hbd", 0)   # (the decimating cascade sums in another order than k_hbdown)
        o.set_option("timing", 1)
    a.set_option("fuse_hbconv", 1)    # (not the default: measured slower, profiles/r06_experiments.txt)
    lens = [min(l, maxin) for l in (maxin, maxin, maxin // 3, 300, maxin, 17, 1, maxin - 5, 2500, maxin, 9, maxin)]
    x = make_input(nch, sum(lens), 17)
    ya, yb, counts, pos = [], [], [], 0
    for i, l in enumerate(lens):
        xi = x[:, pos:pos + l]
        pos += l
        u, v = a.process_host(xi), b.process_host(xi)
        assert u.shape == v.shape and np.array_equal(u, v), (i, l)
        ya.append(u)
        counts.append(u.shape[1])
        if i == 5:
            blob = a.state_dict()
            a = r8b.BatchResampler(src, dst, maxin, 2.0, 180.15, nch=nch, **lib_kw)
            a.set_option("fuse_hbd", 0)
            a.set_option("fuse_hbconv", 1)
            a.set_option("timing", 1)
            a.process_host(x[:, :200] * 0.5)
            a.load_state_dict(blob)
    na, nb = [t[0] for t in a.stage_timings()], [t[0] for t in b.stage_timings()]
    assert "k_convp_hb" in na and "k_convp_hb" not in nb and len(na) == len(nb), (na, nb)
    r, p = refwrap.batch_check(src, dst, maxin, lens, x, np.concatenate(ya, axis=1), counts, 2.0, 180.15)
    assert r.max() <= RMS_TOL and p.max() <= PEAK_TOL, (r.max(), p.max())


@pytest.mark.parametrize("src,dst,maxin", HBCONV_TOPOLOGIES)
def test_emulated_half_band_front_of_the_convolver(emul, refwrap, src, dst, maxin):
    run_hbconv_fused({"lib": emul}, refwrap, src, dst, maxin)


HB_CARRY_TOPOLOGIES = [(176400.0, 44100.0, 16384, 2.0), (192000.0, 44100.0, 8192, 0.5), (44100.0, 2822400.0, 1024, 2.0),
                       (2822400.0, 176400.0, 8192, 2.0), (352800.0, 44100.0, 4096, 2.0)]


def run_history_copy_carried(lib_kw, src, dst, maxin, tb):
    """chains whose first stage is a half-band decimator, and the SACD chain in calls without a convolver block: the
    history copy rides on a half-band launch of the call -- no k_tail launch in whole calls --, same samples as with the
    copy kernel bit for bit"""
    a = r8b.BatchResampler(src, dst, maxin, tb, 180.15, nch=5, **lib_kw)
    b = r8b.BatchResampler(src, dst, maxin, tb, 180.15, nch=5, **lib_kw)
    b.set_option("fold_tail", 0)
    rng = np.random.default_rng(9)
    n = 0
    for i in range(12):
        x = rng.uniform(-1.0, 1.0, (5, maxin))
        ya, yb = a.process_host(x), b.process_host(x)
        assert ya.shape == yb.shape and np.array_equal(ya, yb), i
        n += ya.shape[1]
    assert n > 0 and b.stat("tail_launches") == 12
    # (the first calls of a stream may have no half-band work yet)
    assert a.stat("tail_launches") <= 2, a.stat("tail_launches")


@pytest.mark.parametrize("src,dst,maxin,tb", HB_CARRY_TOPOLOGIES)
def test_emulated_history_copy_carried_by_a_half_band_launch(emul, src, dst, maxin, tb):
    run_history_copy_carried({"lib": emul}, src, dst, maxin, tb)


def run_parked_outputs(lib_kw, case, phase=0):
    src, dst, maxin, tb, att, kind = case[:6]

    def make(park):
        r = r8b.BatchResampler(src, dst, maxin, tb, att, nch=3, phase=phase, **lib_kw)
        for k, v in (case[6] if len(case) > 6 else {}).items():
            r.set_option(k, v)
        r.set_option("park", park)
        return r

    return check_parked_outputs(make, case)


@pytest.mark.parametrize("case", PARK_CASES)
def test_emulated_parked_outputs_equal_recomputation(emul, case):
    """cases.check_parked_outputs on the emulated engine"""
    run_parked_outputs({"lib": emul}, case)


@pytest.mark.parametrize("case", PARK_CASES_MINPHASE)
def test_emulated_parked_outputs_minimum_phase(emul, case):
    run_parked_outputs({"lib": emul}, case, phase=1)


def test_emulated_every_block_once_with_parked_outputs(emul):
    """BASELINE's cfg2 / cfg3 call size: 13.4 / 7.5 blocks per call with the last block computed twice, 12.4 / 6.5
    with its outputs parked (one block per call less)"""
    for src, dst, per_call in ((44100.0, 96000.0, 32768.0 / 2646.0), (96000.0, 44100.0, 16384.0 / 2530.0)):
        r = r8b.BatchResampler(src, dst, 16384, 2.0, 180.15, nch=1, lib=emul)
        x = make_input(1, 16384, 3)
        calls = 12
        for _ in range(calls):
            r.process_host(x)
        nblk = r.stat("conv_blocks")
        assert abs(nblk / calls - per_call) < 0.6 / calls + 0.25, (src, dst, nblk / calls, per_call)
        assert nblk / calls < per_call + 0.35


def run_chunk_invariance_with_no_work_calls_and_checkpoints(lib_kw, src, dst, maxin, tb=2.0, phase=0):
    """the history a call leaves is cut to what the NEXT call's first block reads back to (launch_fused /
    launch_conv_stage), older ring positions keep stale samples, calls served from the park buffer alone keep the history
    with the copy kernel, and checkpoints carry rings and park buffer as they are (state blobs are not canonical:
    bytes nobody reads again depend on how the stream was cut).  None of that may show: a stream cut into ragged
    calls -- single samples and other calls without a block of their own among them -- and resumed from checkpoints
    in fresh objects at those points equals the stream cut into MaxInLen calls bit for bit."""
    n = maxin * 5 + 1234
    x = make_input(3, n, 21)
    a = r8b.BatchResampler(src, dst, maxin, tb, 180.15, nch=3, phase=phase, **lib_kw)
    ya = np.concatenate([a.process_host(x[:, i:i + maxin]) for i in range(0, n, maxin)], axis=1)
    lens = [maxin, 1, 1, 3, maxin // 2 + 7, 1, maxin, 17, 2, 1, maxin - 9, 40, 5, maxin, 1, 1, maxin // 3]
    b = r8b.BatchResampler(src, dst, maxin, tb, 180.15, nch=3, phase=phase, **lib_kw)
    ys, pos, k = [], 0, 0
    while pos < n:
        l = min(lens[k % len(lens)], n - pos)
        ys.append(b.process_host(x[:, pos:pos + l]))
        pos += l
        k += 1
        if k in (2, 3, 6, 9, 10, 15):
            # (behind single-sample calls, behind a long call, behind a call served from the park buffer)
            blob = b.state_dict()
            b = r8b.BatchResampler(src, dst, maxin, tb, 180.15, nch=3, phase=phase, **lib_kw)
            b.process_host(x[:, :min(333, maxin)] * 0.25)   # unrelated history before the load
            b.load_state_dict(blob)
    yb = np.concatenate(ys, axis=1)
    assert ya.shape == yb.shape and np.array_equal(ya, yb)


@pytest.mark.parametrize("src,dst,maxin,tb", TAIL_TOPOLOGIES)
def test_emulated_chunk_invariance_with_no_work_calls_and_checkpoints(emul, src, dst, maxin, tb):
    run_chunk_invariance_with_no_work_calls_and_checkpoints({"lib": emul}, src, dst, maxin, tb)


# minimum-phase chains whose convolver + interpolator run as one launch (Engine::fused_shift: emitted outputs renumbered
# onto the canonical stream), alone and in front of further stages, and the long-block forms with a complex spectrum
MINPHASE_CHUNK_TOPOLOGIES = [(44100.0, 96000.0, 8192, 2.0), (96000.0, 44100.0, 16384, 2.0), (44100.0, 192000.0, 4096, 2.0),
                             (48000.0, 44100.0, 6000, 2.0), (44100.0, 88200.0, 9000, 0.5), (96000.0, 44100.0, 16384, 0.5)]


@pytest.mark.parametrize("src,dst,maxin,tb", MINPHASE_CHUNK_TOPOLOGIES)
def test_emulated_chunk_invariance_minimum_phase(emul, src, dst, maxin, tb):
    run_chunk_invariance_with_no_work_calls_and_checkpoints({"lib": emul}, src, dst, maxin, tb, phase=1)


@pytest.mark.parametrize("src,dst,maxin,tb", MINPHASE_CHUNK_TOPOLOGIES[:4])
def test_emulated_fused_minimum_phase_equals_unfused(emul, src, dst, maxin, tb):
    """option fuse_latency = 0 (convolver and interpolator as two launches, the form of rounds 1-4) against the fused
    launch: the same stream to rounding, the same counts per call, ragged calls"""
    x = make_input(3, maxin * 4 + 777, 8)
    lens = [maxin, 1, maxin // 3, 17, maxin, maxin - 5, 300, maxin]
    ys = []
    for fl in (1, 0):
        b = r8b.BatchResampler(src, dst, maxin, tb, 180.15, nch=3, phase=1, lib=emul)
        b.set_option("fuse_latency", fl)
        b.set_option("timing", 1)
        names = [t[0] for t in b.stage_timings()]
        assert any(t == "k_convp_whole" for t in names) == bool(fl), names
        b.set_option("timing", 0)
        out, pos = [], 0
        for l in lens:
            l = min(l, x.shape[1] - pos)
            out.append(b.process_host(x[:, pos:pos + l]))
            pos += l
        ys.append(out)
    assert [o.shape for o in ys[0]] == [o.shape for o in ys[1]]
    d = np.abs(np.concatenate(ys[0], axis=1) - np.concatenate(ys[1], axis=1))
    assert d.shape[1] > 1000 and d.max() <= 2e-14, d.max()


@pytest.mark.parametrize("src,dst,knob", [(48000.0, 16000.0, "pair_solo"), (88200.0, 44100.0, "pair_solo"),
                                          (44100.0, 96000.0, "pair_two"), (44100.0, 88200.0, "pair_conv"),
                                          # (round 5's two structural options -- the one-channel long-block
                                          # form with the interpolator fused in, 0.5 % band; the polyphase 3x form)
                                          (96000.0, 44100.0, "solo_fuse"), (16000.0, 48000.0, "up3_poly")])
@pytest.mark.parametrize("first", [1, 0])
def test_emulated_park_buffers_follow_structural_options_after_clear(emul, src, dst, knob, first):
    """clear() + a structural option that changes the park rows' length (one-channel / pair form, ...)
    must not leave the old buffers, stride or buffer index behind: the checkpoint is exactly state_size() bytes and the
    stream after the toggle equals that of an object created with the option (bit for bit), both ways."""
    tb = 0.5 if knob in ("pair_solo", "solo_fuse") else 2.0
    nch, chunk = 2, 1500
    x = make_input(nch, 6 * chunk, 23)

    def fresh(v):
        o = r8b.BatchResampler(src, dst, chunk, tb, 136.45, nch=nch, lib=emul)
        o.set_option(knob, v)
        return o

    ref = fresh(1 - first)
    y_ref = [ref.process_host(x[:, i:i + chunk]) for i in range(0, 6 * chunk, chunk)]
    b = fresh(first)
    for i in range(0, 3 * chunk, chunk):          # an odd number of parking calls: the buffer index may be 1
        b.process_host(x[:, i:i + chunk])
    b.clear()
    b.set_option(knob, 1 - first)
    size = emul.r8b_batch_state_size(b._h)
    guard = np.full(size + 4096, 0xA5, dtype=np.uint8)
    n = emul.r8b_batch_state_save(b._h, guard.ctypes.data, size, None)
    assert n == size and np.all(guard[size:] == 0xA5)  # nothing written past the caller's buffer
    ys = []
    for k, i in enumerate(range(0, 6 * chunk, chunk)):
        ys.append(b.process_host(x[:, i:i + chunk]))
        if k == 2:
            blob = b.state_dict()
            assert blob.size == emul.r8b_batch_state_size(b._h)
            c = fresh(1 - first)
            c.load_state_dict(blob)
            assert np.array_equal(c.process_host(x[:, 3 * chunk:4 * chunk]), y_ref[3])
    for a, r in zip(ys, y_ref):
        assert a.shape == r.shape and np.array_equal(a, r)


def test_emulated_state_blob_with_too_much_written_ahead_is_refused(emul):
    """a stage that writes its call's last block AHEAD into the next ring has counters but no buffer;
    a blob whose counters claim more than one block's outputs would make the next calls skip their blocks."""
    import struct
    b = r8b.BatchResampler(44100.0, 2822400.0, 1024, 2.0, 180.15, nch=2, lib=emul)  # convolver in front of a cascade
    x = make_input(2, 2048, 29)
    b.process_host(x[:, :1024])
    blob = b.state_dict()
    # StateHeader 32 bytes; StageState: m, done, rpos, ring_size, has_ring, pos_frac, pos_shift, in_counter, in_pos_int,
    # park_len, park_base, park_end
    st = list(struct.unpack_from("<5q2d5q", blob, 32))
    assert st[9] == 0 and st[11] >= st[10]          # no buffer; something may be written ahead
    bad = blob.copy()
    st[11] = st[10] + 10 ** 6
    struct.pack_into("<5q2d5q", bad, 32, *st)
    keep = b.state_dict()
    with pytest.raises(RuntimeError, match="impossible counters"):
        b.load_state_dict(bad)
    assert np.array_equal(b.state_dict(), keep)
    b.load_state_dict(blob)


def test_emulated_live_engine_keeps_its_tables_through_a_ratio_sweep(emul):
    """Bounded caches (reference r8bconf.h:90,103): an engine that is alive while a host sweeps 130 other ratios through
    the same library -- more than any of the three caches holds -- goes on bit for bit like one that ran alone, and the
    lane-table cache of the fused interpolator stays at its bound."""
    import ctypes as C
    x = make_input(2, 4096, 31)
    alone = r8b.BatchResampler(44100.0, 96000.0, 1024, 2.0, 180.15, nch=2, lib=emul)
    y_alone = [alone.process_host(x[:, i:i + 1024]) for i in range(0, 4096, 1024)]
    a = r8b.BatchResampler(44100.0, 96000.0, 1024, 2.0, 180.15, nch=2, lib=emul)
    ya = [a.process_host(x[:, i:i + 1024]) for i in range(0, 2048, 1024)]
    for i in range(130):
        o = r8b.BatchResampler(44100.0, 44100.0 * (161 + i) / 147, 512, 2.0 + 0.005 * i, 120.0 + 0.1 * i, nch=2, lib=emul)
        if i % 40 == 0:
            o.process_host(x[:, :512])
        del o
    f, b, t = C.c_int(), C.c_int(), C.c_int()
    emul.r8b_design_cache_counts(C.byref(f), C.byref(b), C.byref(t))
    assert f.value <= 98 and b.value <= 13 and 90 <= t.value <= 96, (f.value, b.value, t.value)
    ya += [a.process_host(x[:, i:i + 1024]) for i in range(2048, 4096, 1024)]
    for u, v in zip(ya, y_alone):
        assert np.array_equal(u, v)
    # a new object of the swept-out ratio gets the same tables again (deterministic search): same stream
    again = r8b.BatchResampler(44100.0, 96000.0, 1024, 2.0, 180.15, nch=2, lib=emul)
    assert np.array_equal(again.process_host(x[:, :1024]), y_alone[0])


def _build_cxx_threads(tmp_path, libdir, extra=()):
    exe = str(tmp_path / "cxx_threads")
    subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", *extra, os.path.join(ROOT, "tests", "cxx_threads.cpp"),
                    "-L" + libdir, "-lr8bsrc_emul", "-Wl,-rpath," + libdir, "-o", exe], check=True)
    return exe


def test_threading_contract_host_side(emul, tmp_path):
    """VERDICT r4 weak #2 / reference README.md:52-55: ten host threads create and drive objects at once (eight ratios, one
    of them three times: cache hits and double designs under contention), every stream equals the single-threaded run
    bit for bit, r8b_last_error() is per thread (tests/cxx_threads.cpp; the GPU tier runs it on the HIP library with
    device buffers and a stream per thread)."""
    exe = _build_cxx_threads(tmp_path, os.path.join(ROOT, "tests", "emul", "_build"))
    for _ in range(3):
        out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert out.returncode == 0 and out.stdout.strip().endswith("OK"), (out.returncode, out.stdout[-2000:])


@pytest.mark.skipif(os.environ.get("R8B_TSAN") != "1", reason="a minute of compilation: R8B_TSAN=1 runs it")
def test_threading_contract_under_thread_sanitizer(tmp_path):
    """the same program against a ThreadSanitizer build of the host side (designer, caches, plan, engine, C ABI): no
    data race reported (round 5: clean)"""
    d = os.path.join(ROOT, "tests", "emul")
    subprocess.run(["make", "tsan"], cwd=d, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    exe = _build_cxx_threads(tmp_path, os.path.join(d, "_build", "tsan"), extra=("-g", "-fsanitize=thread"))
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and "ThreadSanitizer" not in out.stdout and out.stdout.strip().endswith("OK"), out.stdout[-3000:]


# (the last field: the case is known to walk -- a 2048 -> 4096-point fused pair with an even number of phases)
WALK_CASES = [(44100.0, 96000.0, 16384, 2.0, 180.15, 0, True), (44100.0, 96000.0, 6000, 2.0, 180.15, 1, False),
              (22050.0, 48000.0, 16384, 2.0, 180.15, 0, True), (96000.0, 44100.0, 16384, 2.0, 180.15, 0, False),
              (44100.0, 96000.0, 16384, 3.0, 150.0, 0, False)]


def run_walk_form_case(lib_kw, case, walk_len, nch=5):
    """the walk form of the fused pair kernel (r8b_convp.h convp_walk: a workgroup per channel pair takes the call's
    interior blocks one after the other, rows and twiddles kept; a call's first and last blocks on the general body in
    the same launch) against a workgroup per block: the same stream bit for bit, ragged calls, odd channel count"""
    src, dst, maxin, tb, att, phase, _ = case

    def mk(w):
        b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=nch, phase=phase, **lib_kw)
        b.set_option("walk", w)
        b.set_option("walk_len", walk_len)
        return b

    a, b = mk(0), mk(2)
    w0 = b.stat("walk_blocks")
    x = make_input(nch, 6 * maxin, 37)
    lens = [maxin, maxin, maxin // 3, 300, maxin, 17, 1, maxin - 5, 2500, maxin]
    pos = 0
    for l in lens:
        if pos + l > x.shape[1]:
            break
        ya, yb = a.process_host(x[:, pos:pos + l]), b.process_host(x[:, pos:pos + l])
        pos += l
        assert ya.shape == yb.shape and np.array_equal(ya, yb), (case, walk_len, pos)
    return b.stat("walk_blocks") - w0, a.stat("conv_blocks")


@pytest.mark.parametrize("walk_len", [0, 1, 3])
@pytest.mark.parametrize("case", WALK_CASES)
def test_emulated_walk_form_equals_one_block_form(emul, case, walk_len):
    walked, blocks = run_walk_form_case({"lib": emul}, case, walk_len)
    if case[6]:
        assert walked >= blocks // 3, (walked, blocks)   # (the long calls do walk: most of their blocks are interior ones)
    # (a call whose blocks were walked names the walk kernel, as on the device -- tests/test_channel_axis.py)
    src, dst, maxin, tb, att, phase, _ = case
    b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=5, phase=phase, lib=emul)
    b.set_option("walk", 2)
    b.set_option("walk_len", walk_len)
    b.set_option("timing", 1)
    x = make_input(5, maxin, 37)
    for _ in range(2):
        w0 = b.stat("walk_blocks")
        b.process_host(x)
        call_walked = b.stat("walk_blocks") > w0
        assert call_walked or not case[6], case
        if call_walked:
            assert any(s.startswith("k_convp_walk<") for s in b.stage_symbols()), b.stage_symbols()


UP3_CASES = [(16000.0, 48000.0, 3000, 2.0, 180.15, 0), (16000.0, 48000.0, 16384, 2.0, 180.15, 0),
             (8000.0, 48000.0, 2000, 2.0, 180.15, 0),     # ... in front of a half-band up-sampler (written ahead into its ring)
             (32000.0, 96000.0, 4096, 1.0, 180.15, 0),    # 4253 taps
             (44100.0, 132300.0, 2500, 3.0, 140.0, 0),    # a shorter filter: another window length
             (16000.0, 48000.0, 3000, 2.0, 180.15, 1)]    # minimum phase: one-sided components of a causal filter


def run_polyphase_up3_case(lib_kw, refwrap, case, nch=3):
    """3x up-sampling convolvers in the polyphase form (r8b_convp.h mode 19: one forward transform of the INPUT samples,
    three backward ones) against the zero-stuffing block (option up3_poly = 0): same counts per call, samples to
    rounding (another block anchoring), ragged calls, odd channel count; linear phase also against the oracle"""
    src, dst, maxin, tb, att, phase = case
    objs = []
    for v in (1, 0):
        b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=nch, phase=phase, **lib_kw)
        b.set_option("up3_poly", v)
        objs.append(b)
    x = make_input(nch, 45000, 41)
    lens = [maxin, maxin // 3, 300, maxin, 17, 1, maxin - 5] * 30
    pos, worst, n = 0, 0.0, 0
    for l in lens:
        if pos + l > x.shape[1]:
            break
        ya, yb = objs[0].process_host(x[:, pos:pos + l]), objs[1].process_host(x[:, pos:pos + l])
        pos += l
        assert ya.shape == yb.shape, (case, pos)
        if ya.shape[1]:
            worst = max(worst, float(np.abs(ya - yb).max()))
            n += ya.shape[1]
    assert n > 10000 and worst <= 1e-14, (case, n, worst)
    # (more blocks of the shorter window for the same stream: the form is the one that ran)
    assert objs[0].stat("conv_blocks") > objs[1].stat("conv_blocks"), case
    if phase == 0:
        b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=2, **lib_kw)
        r, p = compare_stream(b, src, dst, maxin, min(maxin, 1500), 30000, tb, att, 2)
        assert r <= RMS_TOL and p <= PEAK_TOL, (case, r, p)


@pytest.mark.parametrize("case", UP3_CASES)
def test_emulated_polyphase_up3_equals_zero_stuffing(emul, refwrap, case):
    run_polyphase_up3_case({"lib": emul}, refwrap, case)


SOLO_FUSE_CASES = [(96000.0, 44100.0, 3000, 0.5), (96000.0, 44100.0, 16384, 0.5), (192000.0, 44100.0, 5000, 0.5),
                   (96000.0, 44100.0, 8192, 0.6)]


def run_solo_fused_case(lib_kw, case, nch=3):
    """16384-point 1:1 blocks with the whole-step interpolator fused in (mode 18) against the two launches (option
    solo_fuse = 0): same counts per call, samples to rounding; fused: ragged calls == whole calls bit for bit"""
    src, dst, maxin, tb = case
    x = make_input(nch, 70000, 43)

    def run(fuse, lens):
        b = r8b.BatchResampler(src, dst, maxin, tb, 180.15, nch=nch, **lib_kw)
        b.set_option("solo_fuse", fuse)
        b.set_option("timing", 1)
        names = [t[0] for t in b.stage_timings()]
        b.set_option("timing", 0)
        pos, ys = 0, []
        for l in lens:
            if pos + l > x.shape[1]:
                break
            ys.append(b.process_host(x[:, pos:pos + l]))
            pos += l
        return np.concatenate(ys, axis=1), names

    ragged = [maxin, maxin // 3, 300, maxin, 17, 1, maxin - 5] * 40
    y1, n1 = run(1, ragged)
    y0, n0 = run(0, ragged)
    assert "k_convp_whole" in n1 and "k_convp_whole" not in n0, (n1, n0)
    assert y1.shape == y0.shape and y1.shape[1] > 5000 and float(np.abs(y1 - y0).max()) <= 1e-14, (case, y1.shape)
    y2, _ = run(1, [maxin] * 60)
    n = min(y1.shape[1], y2.shape[1])
    assert np.array_equal(y1[:, :n], y2[:, :n]), case


@pytest.mark.parametrize("case", SOLO_FUSE_CASES)
def test_emulated_one_channel_form_fused_with_the_interpolator(emul, case):
    run_solo_fused_case({"lib": emul}, case)


# (src, dst, MaxInLen, transition band, attenuation, phase): a chain per form that stores output PAIRS -- the fused
# two-phase pair form (even and odd phase counts), the walk form, the split 2x and the decimating one-channel forms, the
# polyphase 3x form -- and neighbours that do not (one-channel form with the interpolator, half-band cascade)
COLUMN_CASES = [(44100.0, 96000.0, 6000, 2.0, 180.15, 0), (44100.0, 96000.0, 16384, 2.0, 180.15, 0),
                (96000.0, 44100.0, 6000, 2.0, 180.15, 0), (44100.0, 88200.0, 9000, 0.5, 180.15, 0),
                (88200.0, 44100.0, 12000, 0.5, 180.15, 0), (16000.0, 48000.0, 6000, 2.0, 180.15, 0),
                (96000.0, 44100.0, 9000, 0.5, 180.15, 0), (44100.0, 176400.0, 3000, 2.0, 180.15, 0),
                (44100.0, 96000.0, 6000, 2.0, 180.15, 1)]


def run_output_columns_case(lib_kw, case, device_buffers, nch=3):
    """Every call's outputs at column 4 + c, c = 0 ... 3, of rows filled with NaN: the same values as a column-0 caller
    gets, bit for bit (a pair of outputs at an odd column is ONE 16-byte store at element alignment -- R8B_OUT_STORE16U,
    r8b_convp.h -- instead of two 8-byte ones), and not a byte outside the call's n outputs.  device_buffers(x, rows,
    cols) -> (input pointer, input row stride, output buffer object, its pointer, read-back function)."""
    src, dst, maxin, tb, att, phase = case

    def mk():
        b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=nch, phase=phase, **lib_kw)
        b.set_option("walk", 2)
        return b

    ref, objs = mk(), [mk() for _ in range(4)]
    cap = ref.max_out_len
    pitch = cap + 16
    x = make_input(nch, 6 * maxin, 23)
    pos = 0
    for l in [maxin, maxin // 3, maxin, 301, maxin - 5, maxin]:
        xa = np.ascontiguousarray(x[:, pos:pos + l])
        pos += l
        yref = ref.process_host(xa)
        for c, o in enumerate(objs):
            col = 4 + c
            ip, istride, obuf, op, back = device_buffers(xa, nch, pitch)
            n = o.process_ptr(ip, istride, l, op + 8 * col, pitch)
            got = back(obuf)
            assert n == yref.shape[1], (case, l, c)
            assert np.array_equal(got[:, col:col + n], yref), (case, l, c)
            assert np.isnan(got[:, :col]).all() and np.isnan(got[:, col + n:]).all(), (case, l, c)


def _host_buffers(xa, rows, cols):
    obuf = np.full((rows, cols), np.nan)
    return xa.ctypes.data, xa.shape[1], obuf, obuf.ctypes.data, lambda b: b


@pytest.mark.parametrize("case", COLUMN_CASES)
def test_emulated_output_columns_are_bitwise_alike(emul, case):
    run_output_columns_case({"lib": emul}, case, _host_buffers)


# ---- eight elements per thread (r8b_convq.h, engine option "quad"; round 6) ------------------------------------------------
def _qswz(e):
    return e ^ (((e >> 4) & 1) * 2) ^ (((e >> 5) & 1) * 13) ^ (((e >> 6) & 1) * 9)


def _qfmap(p):
    return ((p >> 8) << 9) | (p & 255)


def test_convq_swizzle_is_conflict_free():
    """r8b_convq.h qswz(): in every pass of the 512-thread form the sixteen lanes LDS serves together (16-byte accesses)
    touch sixteen different 16-byte bank groups -- forward passes address forward positions through qfmap()"""
    def check(name, elems_of_lane):
        # elems_of_lane(b) -> the element indices lane b touches, one per access of the pass (same order in every lane)
        for g0 in range(0, 512, 16):
            per_access = list(zip(*[elems_of_lane(b) for b in range(g0, g0 + 16)]))
            for acc in per_access:
                banks = {_qswz(e) & 15 for e in acc}
                assert len(banks) == 16, (name, g0, acc)

    for n in (2048, 512, 128, 32, 8):        # forward DIF passes, radix 4
        q = n // 4
        check("fwd %d" % n, lambda b: [_qfmap((b // q) * n + b % q + p * q) for p in range(4)])
    check("middle read", lambda b: [_qfmap(4 * b + c) for c in range(4)])
    check("middle write", lambda b: [8 * b + p for p in range(8)])
    for n in (64, 512, 4096):                # backward DIT passes, radix 8
        q = n // 8
        check("bwd %d" % n, lambda b: [(b // q) * n + b % q + p * q for p in range(8)])
    # ... and the map is a permutation of the array
    assert sorted(_qswz(e) for e in range(4096)) == list(range(4096))


QUAD_CASES = [(44100.0, 88200.0, 6000, 2.0, 180.15, {}),
              (44100.0, 88200.0, 6000, 2.0, 180.15, {"park": 0}),
              (44100.0, 88200.0, 2500, 2.0, 180.15, {"fold_tail": 0}),
              (44100.0, 2822400.0, 1024, 2.0, 180.15, {}),       # in front of the half-band cascade (written ahead into its ring)
              (44100.0, 44101.0, 3000, 2.0, 180.15, {})]         # ... of the polynomial interpolator


def run_quad_case(lib_kw, case, nch=5):
    """the 2048 -> 4096-point convolver-only block pair on 512 threads (eight elements per thread, r8b_convq.h) against
    the 256-thread form: same counts per call, samples to rounding (other radices), ragged calls, odd channel count,
    history tail and parked outputs through the same mechanisms; channel 0 against the oracle"""
    src, dst, maxin, tb, att, opts = case
    x = make_input(nch, 5 * maxin, 41)
    lens = [maxin, maxin, maxin // 5, 17, 1, maxin - 1, maxin // 2]
    outs = []
    for q in (0, 1):
        b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=nch, **lib_kw)
        for k, v in opts.items():
            b.set_option(k, v)
        b.set_option("quad", q)
        ys, pos = [], 0
        for l in lens:
            ys.append(b.process_host(x[:, pos:pos + l]))
            pos += l
        outs.append(ys)
    assert [y.shape for y in outs[0]] == [y.shape for y in outs[1]]
    y0, y1 = np.concatenate(outs[0], axis=1), np.concatenate(outs[1], axis=1)
    assert y1.shape[1] > 1000
    d = y0 - y1
    assert np.sqrt((d * d).mean()) <= RMS_TOL and np.abs(d).max() <= PEAK_TOL
    assert d.any()   # (another rounding: the 512-thread kernel really ran)
    o = O.OracleResampler(src, dst, maxin, tb, att)
    yo, pos = [], 0
    for l in lens:
        yo.append(o.process(x[0, pos:pos + l]))
        pos += l
    do = y1[0] - np.concatenate(yo)
    assert np.sqrt((do * do).mean()) <= RMS_TOL and np.abs(do).max() <= PEAK_TOL


# ---- half-array form (r8b_convp.h cp_ha_*, kernel mode 21, engine option "half"; round 6) ----------------------------------
def _dswz(e):
    return e ^ ((e >> 4) & 15) ^ (((e >> 8) & 1) << 4)


def test_half_array_swizzle_is_conflict_free():
    """r8b_convp.h dswz(): every access pattern of the half-array form's two exchanges (8-byte accesses to an array of 4096
    doubles) meets 16 different slots mod 16 in each 16 consecutive lanes (ds_write_b64: 4 x 16 lanes, 32 banks of 4 bytes)
    and 32 different slots mod 32 in each 32 (ds_read_b64: 2 x 32 lanes, 64 banks); the map is a permutation"""
    def check(name, elems_of_lane, group):
        for g0 in range(0, 256, group):
            per_access = list(zip(*[elems_of_lane(b) for b in range(g0, g0 + group)]))
            for acc in per_access:
                assert len({_dswz(e) & (group - 1) for e in acc}) == group, (name, g0, acc)

    mid = lambda lt: [16 * lt + p for p in range(16)]
    b1 = lambda lt: [(lt >> 4) * 256 + (lt & 15) + 16 * p for p in range(16)]
    b2 = lambda lt: [lt + 256 * i for i in range(16)]
    check("middle write", mid, 16)
    check("sub-length 256 read", b1, 32)
    check("sub-length 256 write", b1, 16)
    check("last pass read", b2, 32)
    assert sorted(_dswz(e) for e in range(4096)) == list(range(4096))
    # linear over XOR: slot(e0 | d) = (slot(e0) ^ (dswz(d) & 31)) + (d & ~31) for offsets d that share no bit with e0
    for e0, ds in ((16 * 37, range(16)), ((5 << 8) + 9, [16 * p for p in range(16)]), (201, [256 * i for i in range(16)])):
        for d in ds:
            assert e0 & d == 0 and _dswz(e0 | d) == (_dswz(e0) ^ (_dswz(d) & 31)) + (d & ~31)


def run_half_case(lib_kw, case, nch=5, bitwise=True):
    """the half-array form of the 2048 -> 4096-point convolver-only block pair against the 64 KB form: the same arithmetic
    on the same values -- BITWISE equal under host emulation (no contraction), to rounding on the GPU (the device
    compiler contracts multiply-adds differently in the two kernels) -- over ragged calls, odd channel counts, history
    tail and parked outputs; option values 0 / 2 = never / always (1 = objects whose largest call holds 512 workgroups and more: Engine::half_worth)"""
    src, dst, maxin, tb, att, opts = case
    x = make_input(nch, 5 * maxin, 43)
    lens = [maxin, maxin, maxin // 5, 17, 1, maxin - 1, maxin // 2]
    outs = []
    opts = dict(opts)
    phase = opts.pop("_phase", 0)   # (1: minimum-phase filters -- complex kernel spectra, kernel modes 31 / 32)
    for h in (0, 1):
        b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=nch, phase=phase, **lib_kw)
        for k, v in opts.items():
            b.set_option(k, v)
        b.set_option("half", 2 * h)
        ys, pos = [], 0
        for l in lens:
            ys.append(b.process_host(x[:, pos:pos + l]))
            pos += l
        outs.append(ys)
    assert [y.shape for y in outs[0]] == [y.shape for y in outs[1]]
    y0, y1 = np.concatenate(outs[0], axis=1), np.concatenate(outs[1], axis=1)
    assert y1.shape[1] > 1000 and np.isfinite(y1).all()
    if bitwise:
        assert np.array_equal(y0, y1)
    else:
        d = y0 - y1
        assert np.sqrt((d * d).mean()) <= 2e-16 and np.abs(d).max() <= 4e-15
    # (the form really ran: the stage's last launch by its device symbol)
    b.set_option("timing", 1)
    b.process_host(x[:, :maxin])
    assert any(sym in b.stage_symbols() for sym in ("k_convp<11, 1, 21, 24>", "k_convp<11, 1, 22, 24>", "k_convp<12, 1, 21, 24>",
                                                    "k_convp<12, 1, 22, 24>", "k_convp<12, -1, 27, 24>",
                                                    "k_convp<12, -1, 28, 24>", "k_convp<11, 1, 31, 24>", "k_convp<11, 1, 32, 24>",
                                                    "k_convp<12, 1, 31, 24>", "k_convp<12, 1, 32, 24>")), b.stage_symbols()
    return y1


# (the 2048 -> 4096-point block pair in the chains of QUAD_CASES; the 3x strided store behind it; the 4096 -> 8192-point
# geometry -- 512 threads, 64 KB instead of 128 -- alone and in front of the strided store)
HALF_CASES = QUAD_CASES + [(48000.0, 32000.0, 6000, 3.0, 150.0, {}),
                           (44100.0, 88200.0, 12000, 1.0, 180.15, {}), (44100.0, 88200.0, 7000, 1.0, 180.15, {"park": 0}),
                           (48000.0, 32000.0, 13000, 2.0, 180.15, {}), (96000.0, 64000.0, 5000, 2.0, 180.15, {"fold_tail": 0}),
                           # the decimating 4096 -> 2048-point geometry (kernel modes 27 / 28): alone, behind a half-band
                           # decimator, in front of the strided store
                           (88200.0, 44100.0, 16384, 2.0, 180.15, {}), (88200.0, 44100.0, 5000, 2.0, 180.15, {"park": 0}),
                           (176400.0, 44100.0, 12000, 2.0, 180.15, {}), (88200.0, 44100.0, 3000, 2.0, 180.15, {"fold_tail": 0}),
                           (32000.0, 48000.0, 6000, 3.0, 180.15, {}), (64000.0, 96000.0, 9000, 3.0, 180.15, {"park": 0}),
                           # minimum phase (complex kernel spectra: kernel modes 31 / 32)
                           (44100.0, 88200.0, 6000, 2.0, 180.15, {"_phase": 1}), (48000.0, 32000.0, 6000, 3.0, 150.0, {"_phase": 1}),
                           (44100.0, 88200.0, 9000, 1.0, 180.15, {"_phase": 1}), (48000.0, 32000.0, 9000, 2.0, 180.15, {"_phase": 1})]


@pytest.mark.parametrize("case", range(len(HALF_CASES)))
def test_emulated_half_array_form_is_bitwise_the_full_one(emul, case):
    run_half_case({"lib": emul}, HALF_CASES[case])


def test_emulated_half_array_forms_are_chosen_by_the_objects_size(emul):
    """option half = 1 (the default): channel pairs x blocks of the object's LARGEST call >= 512 (Engine::half_worth) -- a
    constant of the object, whatever the calls it then gets"""
    x = make_input(2, 3000, 7)
    for maxin, sym in ((16384, "k_convp<11, 1, 0, 24>"), (700000, "k_convp<11, 1, 21, 24>")):
        b = r8b.BatchResampler(44100.0, 88200.0, maxin, 2.0, 180.15, nch=2, lib=emul)
        b.set_option("timing", 1)
        b.process_host(x)
        assert b.stage_symbols() == [sym], (maxin, b.stage_symbols())
    b = r8b.BatchResampler(44100.0, 96000.0, 700000, 2.0, 180.15, nch=2, lib=emul)
    b.set_option("timing", 1)
    b.process_host(x)
    assert b.stage_symbols()[0] == "k_convp<11, 1, 23, 24>", b.stage_symbols()


def test_emulated_half_array_levels_and_silence(emul):
    """... with partners of very different level and silent channels (cases.check_pair_scales)"""
    case = PAIR_SCALE_CASES[2]   # 44100 -> 88200, convolver alone
    src, dst, maxin, chunk, n, tb, att = case
    b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=9, lib=emul)
    b.set_option("half", 2)
    rel_rms, rel_pk = check_pair_scales(b, case)
    assert rel_rms <= RMS_TOL and rel_pk <= PEAK_TOL


# (the fused two-phase block pair in the half-array form: kernel mode 23, engine option "half_fused")
HALF_FUSED_CASES = [(44100.0, 96000.0, 16384, 2.0, 180.15, {}), (44100.0, 96000.0, 6000, 2.0, 180.15, {"park": 0}),
                    (22050.0, 48000.0, 16384, 2.0, 180.15, {}), (44100.0, 96000.0, 5000, 2.0, 180.15, {"fold_tail": 0}),
                    (44100.0, 96000.0, 16384, 3.0, 150.0, {}),       # another filter: 1024 -> 2048-point blocks, stays on mode 4
                    (44100.0, 48000.0, 16384, 2.0, 180.15, {}),      # 147 / 160 ... / 80 phases
                    (44100.0, 96000.0, 16384, 2.0, 180.15, {"_phase": 1}), (44100.0, 48000.0, 6000, 2.0, 180.15, {"_phase": 1}),
                    # In > Out with a long input step (320 / 147): the run ends 48 slots short of the array, masked lanes read nothing
                    (48000.0, 44100.0, 16384, 2.0, 180.15, {}), (96000.0, 88200.0, 7000, 2.0, 180.15, {"park": 0}),
                    (48000.0, 44100.0, 5000, 2.0, 180.15, {"_phase": 1}),
                    # the 1:1 geometry (kernel mode 33: both transforms' exchanges by parts; BASELINE's cfg3)
                    (96000.0, 44100.0, 16384, 2.0, 180.15, {}), (96000.0, 44100.0, 5000, 2.0, 180.15, {"park": 0}),
                    (44100.0, 16000.0, 9000, 2.0, 180.15, {"fold_tail": 0}),
                    # a run that ends 4 slots short of the array (input step 320, run offset 336, in_len 2680)
                    (16000.0, 44100.0, 16384, 2.0, 180.15, {}), (32000.0, 88200.0, 6000, 2.0, 180.15, {"park": 0})]


def run_half_fused_case(lib_kw, case, nch=5, bitwise=True, must_run=None):
    """kernel mode 23 (the 2048 -> 4096-point block pair + whole-step interpolator with the transforms' backward exchanges
    by parts and the interpolator's run in a 49 KB array) against a workgroup per block of mode 4: the same arithmetic on
    the same values -- bit for bit under emulation, to rounding on the device --, ragged calls, odd channel counts"""
    src, dst, maxin, tb, att, opts = case

    opts = dict(opts)
    phase = opts.pop("_phase", 0)   # (1: minimum-phase filters -- kernel modes 29 / 30 against 16 / 17)

    def mk(h):
        b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=nch, phase=phase, **lib_kw)
        for k, v in opts.items():
            b.set_option(k, v)
        b.set_option("walk", 0)
        b.set_option("half_fused", 2 * h)
        b.set_option("timing", 1)
        return b

    a, b = mk(0), mk(1)
    x = make_input(nch, 6 * maxin, 39)
    lens = [maxin, maxin, maxin // 3, 300, maxin, 17, 1, maxin - 5, 2500, maxin]
    pos = 0
    ran = False
    for l in lens:
        if pos + l > x.shape[1]:
            break
        ya, yb = a.process_host(x[:, pos:pos + l]), b.process_host(x[:, pos:pos + l])
        pos += l
        assert ya.shape == yb.shape and np.isfinite(yb).all()
        if bitwise:
            assert np.array_equal(ya, yb), (case, pos)
        elif ya.size:   # (a one-sample call of a decimating chain may owe no output)
            d = ya - yb
            assert np.sqrt((d * d).mean()) <= 2e-16 and np.abs(d).max() <= 4e-15, (case, pos)
        ran = ran or any(s in ("k_convp<11, 1, 23, 24>", "k_convp<11, 1, 25, 24>", "k_convp<11, 1, 29, 24>", "k_convp<11, 1, 30, 24>",
                               "k_convp<12, 0, 33, 24>") for s in b.stage_symbols())
    if must_run is not None:
        assert ran == must_run, b.stage_symbols()
    return ran


@pytest.mark.parametrize("case", range(len(HALF_FUSED_CASES)))
def test_emulated_half_array_fused_form_is_bitwise_mode_4(emul, case):
    run_half_fused_case({"lib": emul}, HALF_FUSED_CASES[case], must_run=case not in (4,))


@pytest.mark.parametrize("case", QUAD_CASES)
def test_emulated_eight_elements_per_thread_form(emul, case):
    run_quad_case({"lib": emul}, case)
    # (the form really ran: the stage's device symbol, as test_gpu_parity.py asserts on the device)
    src, dst, _, tb, att, _ = case
    b = r8b.BatchResampler(src, dst, 4096, tb, att, nch=2, lib=emul)
    b.set_option("quad", 1)
    b.set_option("timing", 1)
    b.process_host(make_input(2, 4096, 3))
    assert "k_convq" in b.stage_symbols(), b.stage_symbols()


def test_emulated_eight_elements_per_thread_levels_and_silence(emul):
    """... with partners of very different level and silent channels (cases.check_pair_scales)"""
    case = PAIR_SCALE_CASES[2]   # 44100 -> 88200, convolver alone
    src, dst, maxin, chunk, n, tb, att = case
    b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=9, lib=emul)
    b.set_option("quad", 1)
    rel_rms, rel_pk = check_pair_scales(b, case)
    assert rel_rms <= RMS_TOL and rel_pk <= PEAK_TOL


# The size-driven choices on both sides of their thresholds, emulated: small objects put on either side by option
# form_channels (the channel count the choices are made for -- what a shard of a larger batch sets), the same rows and
# calls on both sides; the GPU twins with real channel counts are in tests/test_channel_axis.py.

def _run_twins(lib, src, dst, maxin, nch, lens, sides, seed=29):
    x = make_input(nch, sum(lens), seed)
    res = []
    for opts in sides:
        b = r8b.BatchResampler(src, dst, maxin, 2.0, 180.15, nch=nch, lib=lib)
        for k, v in opts.items():
            b.set_option(k, v)
        b.set_option("timing", 1)
        ys, pos = [], 0
        for l in lens:
            ys.append(b.process_host(x[:, pos:pos + l]))
            pos += l
        res.append((np.concatenate(ys, axis=1), b.stage_symbols(), b))
    return res


def test_emulated_walk_form_threshold(emul):
    """the walk form from 256 channels (Engine::form_nch; half-array forms pinned off)"""
    (ya, sa, a), (yb, sb, b) = _run_twins(emul, 44100.0, 96000.0, 16384, 5, [16384, 9000],
                                          [{"half": 0, "half_fused": 0, "form_channels": 254},
                                           {"half": 0, "half_fused": 0, "form_channels": 256}])
    assert sa[0] == "k_convp<11, 1, 4, 24>" and sb[0] == "k_convp_walk<11, 1, 4, 24>", (sa, sb)
    assert a.stat("walk_blocks") == 0 and b.stat("walk_blocks") > 0 and np.array_equal(ya, yb)


def test_emulated_half_array_threshold(emul):
    """channel pairs x blocks = 511 / 512 (Engine::half_worth) through form_channels: the fused pair kernel's full-array
    mode below, its half-array mode 23 at the threshold; bitwise equal under emulation"""
    probe = r8b.BatchResampler(44100.0, 96000.0, 1024, 2.0, 180.15, nch=2, lib=emul)
    m = __import__("re").search(r"in_len=(\d+) io=(\d+)/", probe.describe())
    maxin = 7 * (int(m.group(1)) // int(m.group(2)))        # 7 blocks: 73 pairs are 511 workgroups, 74 are 518
    (ya, sa, _), (yb, sb, _) = _run_twins(emul, 44100.0, 96000.0, maxin, 3, [maxin, 1000, maxin],
                                          [{"form_channels": 146}, {"form_channels": 147}])
    assert sa[0] == "k_convp<11, 1, 4, 24>" and sb[0] == "k_convp<11, 1, 23, 24>", (sa, sb)
    assert np.array_equal(ya, yb)


def test_emulated_half_band_cascade_tile_threshold(emul):
    """the cascade's 8192-output tile from channels x tiles >= 1536 (launch_cascade), 4096 below: calls of 1000 samples
    at 44100 -> 2822400 give the cascade (all five half-band stages) 64 000 outputs, eight tiles of 8192"""
    tiles = -(-1000 * 64 // 8192)
    hi = -(-256 * 6 // tiles)
    (ya, _, a), (yb, _, b) = _run_twins(emul, 44100.0, 2822400.0, 1024, 3, [1000] * 4,
                                        [{"half": 0, "half_fused": 0, "form_channels": hi - 2},
                                         {"half": 0, "half_fused": 0, "form_channels": hi}])
    assert "k_hbcascade" in [t[0] for t in b.stage_timings()]
    assert a.stat("hbc_tile_8192") == 0 and b.stat("hbc_tile_8192") > 0, (a.stat("hbc_tile_8192"), b.stat("hbc_tile_8192"))
    assert np.array_equal(ya, yb)


def test_emulated_poly_groups_ending_on_an_unpaired_channel(emul):
    """convolver + polynomial interpolator in channel groups over an odd channel count: the last group holds the
    channel without a partner; bitwise the ungrouped object, the group count's launches"""
    (y0, _, a), (y1, _, b) = _run_twins(emul, 44100.0, 44101.0, 1024, 11, [1000, 700, 1000, 3],
                                        [{"poly_groups": 0}, {"poly_groups": 40}])
    t0, t1 = a.stage_timings(), b.stage_timings()
    # (40 KB between the stages per group, ~2000 doubles per channel and call: groups of 2 ... 4 channels)
    assert [t[2] for t in t1] > [t[2] for t in t0] and np.array_equal(y0, y1), (t0, t1)


def test_65536_channels_are_refused(emul):
    """the channel index rides on the grid's y dimension: 65535 channels is the largest object"""
    assert not emul.r8b_batch_create(44100.0, 96000.0, 128, 2.0, 180.15, 65536, -1)
    assert "65535" in emul.r8b_last_error().decode()


# ---- which kernel form runs each stage (Engine::resolve_forms) ----------------------------------------------------
# Chains: every topology of cases.check_parked_outputs (linear and minimum phase), the minimum-phase chains of cases.py
# (fractional latencies), a polyphase 3x chain, a 16384-point one-channel chain, an 8192 -> 16384-point split chain, a
# half-band decimator in front of its convolver, a run of half-band stages each way.  (src, dst, maxin, tb, atten, phase)
FORM_CHAINS = sorted(set(
    [c[:5] + (0,) for c in PARK_CASES] + [c[:5] + (1,) for c in PARK_CASES_MINPHASE] +
    [(c[0], c[1], c[2], c[5], c[6], 1) for c in MINPHASE_CASES + MINPHASE_LONG_CASES] +
    [(44100.0, 132300.0, 1024, 2.0, 180.15, 0),       # polyphase 3x
     (96000.0, 44100.0, 8192, 0.5, 180.15, 0),        # 16384 points, one-channel form
     (44100.0, 88200.0, 2048, 0.5, 180.15, 0),        # 8192 -> 16384 points, split form
     (176400.0, 44100.0, 4096, 2.0, 180.15, 0),       # half-band decimator + 4096 -> 2048-point convolver
     (44100.0, 2822400.0, 1024, 2.0, 180.15, 0),      # five half-band up-samplers
     (2822400.0, 176400.0, 4096, 2.0, 180.15, 0)]))   # four half-band decimators
# the defaults, and each option set to the value(s) it does not have by default
FORM_VARIANTS = [None] + [(o, 0) for o in ("fast_conv", "pair_conv", "pair_two", "pair_split", "pair_solo", "solo_fuse", "fuse",
                                           "fuse_latency", "fuse_hb", "fuse_hbd", "up3_poly", "half", "half_fused", "park")] + \
    [("fuse_hbd", 1), ("fuse_hbconv", 1), ("half", 2), ("half_fused", 2), ("quad", 1)]


def form_probe(lib, chain, variant, nch=3):
    """(describe() text, state_size, [(the engine's label, kernel symbol) per stage]) of the chain's object under the
    option variant.  Symbols of the compile-time-sized convolver kernels only -- the launchers whose symbol the emulator
    notes --, taken from calls of MaxInLen samples with timing on: until each of them has run, sixteen at the most."""
    src, dst, maxin, tb, att, phase = chain
    b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=nch, phase=phase, lib=lib)
    if variant is not None:
        b.set_option(*variant)
    b.set_option("timing", 1)
    size = lib.r8b_batch_state_size(b._h)
    labels = [t[0] for t in b.stage_timings()]
    fast = [i for i, n in enumerate(labels) if n.startswith(("k_convp", "k_convx"))]
    x = make_input(nch, maxin, 3)
    for _ in range(16):
        b.process_host(x)
        syms = b.stage_symbols()
        if all(syms[i] for i in fast):
            break
    assert lib.r8b_batch_state_size(b._h) == size
    return b.describe(), size, [(n, syms[i] if i in fast else "") for i, n in enumerate(labels)]
# recorded from the build before the per-stage record existed: chain -> (describe() text, {option variant: (state_size,
# ["label|symbol" per stage])}); a variant that is not listed gives what the defaults (None) give
FORM_PINS = {
    (44100.0, 44101.0, 1024, 2.0, 180.15, 1): ('BlockConvolver: flt_len=1417 in_len=2680 io=2/1 fft=2048/4096 latency=2688 nfreq=0.5 tb=2 gain=2\nFracInterpolator: 88200->44101 whole=0 step=0/0 taps=24 fracs=864 order=2\n', {
        None: (295136, ['k_convp|k_convp<11, 1, 6, 24>', 'k_poly|']),
        ('fast_conv', 0): (295136, ['k_conv|', 'k_poly|']),
        ('pair_conv', 0): (295136, ['k_conv|', 'k_poly|']),
        ('half', 2): (295136, ['k_convp|k_convp<11, 1, 31, 24>', 'k_poly|']),
    }),
    (44100.0, 44101.0, 4096, 2.0, 180.15, 0): ('BlockConvolver: flt_len=1417 in_len=2680 io=2/1 fft=2048/4096 latency=3388 nfreq=0.5 tb=2 gain=2\nFracInterpolator: 88200->44101 whole=0 step=0/0 taps=24 fracs=864 order=2\n', {
        None: (491744, ['k_convp|k_convp<11, 1, 0, 24>', 'k_poly|']),
        ('fast_conv', 0): (491744, ['k_conv|', 'k_poly|']),
        ('pair_conv', 0): (491744, ['k_convx|k_convx<10, 1, 0, 24>', 'k_poly|']),
        ('half', 2): (491744, ['k_convp|k_convp<11, 1, 21, 24>', 'k_poly|']),
        ('quad', 1): (491744, ['k_convp|k_convq', 'k_poly|']),
    }),
    (44100.0, 48000.0, 5000, 2.0, 180.15, 0): ('BlockConvolver: flt_len=1417 in_len=2680 io=2/1 fft=2048/4096 latency=3388 nfreq=0.5 tb=2 gain=2\nFracInterpolator: 88200->48000 whole=1 step=147/80 taps=24 fracs=80 order=0\n', {
        None: (133472, ['k_convp_whole|k_convp<11, 1, 5, 24>', 'k_whole|']),
        ('fast_conv', 0): (491744, ['k_conv|', 'k_whole|']),
        ('pair_conv', 0): (295136, ['k_convx_whole|k_convx<10, 1, 1, 24>', 'k_whole|']),
        ('pair_two', 0): (98528, ['k_convp_whole|k_convp<11, 1, 1, 24>', 'k_whole|']),
        ('fuse', 0): (491744, ['k_convp|k_convp<11, 1, 0, 24>', 'k_whole|']),
        ('park', 0): (98528, ['k_convp_whole|k_convp<11, 1, 5, 24>', 'k_whole|']),
        ('half_fused', 2): (133472, ['k_convp_whole|k_convp<11, 1, 25, 24>', 'k_whole|']),
    }),
    (44100.0, 88200.0, 2048, 0.5, 180.15, 0): ('BlockConvolver: flt_len=5671 in_len=10714 io=2/1 fft=8192/16384 latency=13549 nfreq=0.5 tb=0.5 gain=2\n', {
        None: (650816, ['k_convp|k_convp<13, 0, 8, 24>']),
        ('pair_conv', 0): (786560, ['k_convx|k_convx<12, 1, 0, 24>']),
        ('pair_split', 0): (786560, ['k_convx|k_convx<12, 1, 0, 24>']),
        ('park', 0): (393344, ['k_convp|k_convp<13, 0, 8, 24>']),
    }),
    (44100.0, 88200.0, 2048, 0.5, 180.15, 1): ('BlockConvolver: flt_len=5671 in_len=10714 io=2/1 fft=8192/16384 latency=10722 nfreq=0.5 tb=0.5 gain=2\n', {
        None: (650816, ['k_convp|k_convp<13, 0, 12, 24>']),
        ('park', 0): (393344, ['k_convp|k_convp<13, 0, 12, 24>']),
    }),
    (44100.0, 88200.0, 2048, 2.0, 180.15, 1): ('BlockConvolver: flt_len=1417 in_len=2680 io=2/1 fft=2048/4096 latency=2688 nfreq=0.5 tb=2 gain=2\n', {
        None: (163136, ['k_convp|k_convp<11, 1, 6, 24>']),
        ('fast_conv', 0): (98432, ['k_conv|']),
        ('pair_conv', 0): (98432, ['k_conv|']),
        ('park', 0): (98432, ['k_convp|k_convp<11, 1, 6, 24>']),
        ('half', 2): (163136, ['k_convp|k_convp<11, 1, 31, 24>']),
    }),
    (44100.0, 88200.0, 4096, 0.5, 180.15, 1): ('BlockConvolver: flt_len=5671 in_len=10714 io=2/1 fft=8192/16384 latency=10722 nfreq=0.5 tb=0.5 gain=2\n', {
        None: (650816, ['k_convp|k_convp<13, 0, 12, 24>']),
        ('park', 0): (393344, ['k_convp|k_convp<13, 0, 12, 24>']),
    }),
    (44100.0, 88200.0, 4096, 2.0, 180.15, 1): ('BlockConvolver: flt_len=1417 in_len=2680 io=2/1 fft=2048/4096 latency=2688 nfreq=0.5 tb=2 gain=2\n', {
        None: (163136, ['k_convp|k_convp<11, 1, 6, 24>']),
        ('fast_conv', 0): (98432, ['k_conv|']),
        ('pair_conv', 0): (98432, ['k_conv|']),
        ('park', 0): (98432, ['k_convp|k_convp<11, 1, 6, 24>']),
        ('half', 2): (163136, ['k_convp|k_convp<11, 1, 31, 24>']),
    }),
    (44100.0, 88200.0, 6000, 2.0, 180.15, 0): ('BlockConvolver: flt_len=1417 in_len=2680 io=2/1 fft=2048/4096 latency=3388 nfreq=0.5 tb=2 gain=2\n', {
        None: (163136, ['k_convp|k_convp<11, 1, 0, 24>']),
        ('fast_conv', 0): (98432, ['k_conv|']),
        ('pair_conv', 0): (491648, ['k_convx|k_convx<10, 1, 0, 24>']),
        ('park', 0): (98432, ['k_convp|k_convp<11, 1, 0, 24>']),
        ('half', 2): (163136, ['k_convp|k_convp<11, 1, 21, 24>']),
        ('quad', 1): (163136, ['k_convp|k_convq']),
    }),
    (44100.0, 96000.0, 1024, 2.0, 136.45, 1): ('BlockConvolver: flt_len=1081 in_len=3016 io=2/1 fft=2048/4096 latency=3022 nfreq=0.5 tb=2 gain=2\nFracInterpolator: 88200->96000 whole=1 step=147/160 taps=18 fracs=160 order=0\n', {
        None: (179552, ['k_convp_whole|k_convp<11, 1, 16, 24>', 'k_whole|']),
        ('fast_conv', 0): (295136, ['k_conv|', 'k_whole|']),
        ('pair_conv', 0): (295136, ['k_conv|', 'k_whole|']),
        ('pair_two', 0): (295136, ['k_convp|k_convp<11, 1, 6, 24>', 'k_whole|']),
        ('fuse', 0): (295136, ['k_convp|k_convp<11, 1, 6, 24>', 'k_whole|']),
        ('fuse_latency', 0): (295136, ['k_convp|k_convp<11, 1, 6, 24>', 'k_whole|']),
        ('park', 0): (98528, ['k_convp_whole|k_convp<11, 1, 16, 24>', 'k_whole|']),
    }),
    (44100.0, 96000.0, 2048, 0.5, 180.15, 0): ('BlockConvolver: flt_len=5671 in_len=10714 io=2/1 fft=8192/16384 latency=13549 nfreq=0.5 tb=0.5 gain=2\nFracInterpolator: 88200->96000 whole=1 step=147/160 taps=24 fracs=160 order=0\n', {
        None: (786656, ['k_convp|k_convp<13, 0, 8, 24>', 'k_whole|']),
        ('pair_conv', 0): (786656, ['k_convx_whole|k_convx<12, 1, 1, 24>', 'k_whole|']),
        ('pair_split', 0): (786656, ['k_convx_whole|k_convx<12, 1, 1, 24>', 'k_whole|']),
    }),
    (44100.0, 96000.0, 2048, 2.0, 180.15, 1): ('BlockConvolver: flt_len=1417 in_len=2680 io=2/1 fft=2048/4096 latency=2688 nfreq=0.5 tb=2 gain=2\nFracInterpolator: 88200->96000 whole=1 step=147/160 taps=24 fracs=160 order=0\n', {
        None: (168032, ['k_convp_whole|k_convp<11, 1, 16, 24>', 'k_whole|']),
        ('fast_conv', 0): (295136, ['k_conv|', 'k_whole|']),
        ('pair_conv', 0): (295136, ['k_conv|', 'k_whole|']),
        ('pair_two', 0): (295136, ['k_convp|k_convp<11, 1, 6, 24>', 'k_whole|']),
        ('fuse', 0): (295136, ['k_convp|k_convp<11, 1, 6, 24>', 'k_whole|']),
        ('fuse_latency', 0): (295136, ['k_convp|k_convp<11, 1, 6, 24>', 'k_whole|']),
        ('park', 0): (98528, ['k_convp_whole|k_convp<11, 1, 16, 24>', 'k_whole|']),
        ('half_fused', 2): (168032, ['k_convp_whole|k_convp<11, 1, 29, 24>', 'k_whole|']),
    }),
    (44100.0, 96000.0, 4096, 0.5, 180.15, 1): ('BlockConvolver: flt_len=5671 in_len=10714 io=2/1 fft=8192/16384 latency=10722 nfreq=0.5 tb=0.5 gain=2\nFracInterpolator: 88200->96000 whole=1 step=147/160 taps=24 fracs=160 order=0\n', {
        None: (1179872, ['k_convp|k_convp<13, 0, 12, 24>', 'k_whole|']),
    }),
    (44100.0, 96000.0, 4096, 2.0, 109.56, 0): ('BlockConvolver: flt_len=869 in_len=1180 io=2/1 fft=1024/2048 latency=1614 nfreq=0.5 tb=2 gain=2\nFracInterpolator: 88200->96000 whole=1 step=147/160 taps=14 fracs=160 order=0\n', {
        None: (80096, ['k_convp_whole|k_convp<10, 1, 4, 24>', 'k_whole|']),
        ('fast_conv', 0): (442592, ['k_conv|', 'k_whole|']),
        ('pair_conv', 0): (442592, ['k_convx_whole|k_convx<9, 1, 1, 24>', 'k_whole|']),
        ('pair_two', 0): (49376, ['k_convp_whole|k_convp<10, 1, 1, 24>', 'k_whole|']),
        ('fuse', 0): (442592, ['k_convp|k_convp<10, 1, 0, 24>', 'k_whole|']),
        ('park', 0): (49376, ['k_convp_whole|k_convp<10, 1, 4, 24>', 'k_whole|']),
    }),
    (44100.0, 96000.0, 4096, 2.0, 180.15, 1): ('BlockConvolver: flt_len=1417 in_len=2680 io=2/1 fft=2048/4096 latency=2688 nfreq=0.5 tb=2 gain=2\nFracInterpolator: 88200->96000 whole=1 step=147/160 taps=24 fracs=160 order=0\n', {
        None: (168032, ['k_convp_whole|k_convp<11, 1, 16, 24>', 'k_whole|']),
        ('fast_conv', 0): (491744, ['k_conv|', 'k_whole|']),
        ('pair_conv', 0): (491744, ['k_conv|', 'k_whole|']),
        ('pair_two', 0): (491744, ['k_convp|k_convp<11, 1, 6, 24>', 'k_whole|']),
        ('fuse', 0): (491744, ['k_convp|k_convp<11, 1, 6, 24>', 'k_whole|']),
        ('fuse_latency', 0): (491744, ['k_convp|k_convp<11, 1, 6, 24>', 'k_whole|']),
        ('park', 0): (98528, ['k_convp_whole|k_convp<11, 1, 16, 24>', 'k_whole|']),
        ('half_fused', 2): (168032, ['k_convp_whole|k_convp<11, 1, 29, 24>', 'k_whole|']),
    }),
    (44100.0, 96000.0, 4096, 10.0, 109.56, 0): ('BlockConvolver: flt_len=175 in_len=338 io=2/1 fft=256/512 latency=425 nfreq=0.5 tb=10 gain=2\nFracInterpolator: 88200->96000 whole=1 step=147/160 taps=14 fracs=160 order=0\n', {
        None: (24800, ['k_convp_whole|k_convp<8, 1, 1, 24>', 'k_whole|']),
        ('fast_conv', 0): (418016, ['k_conv|', 'k_whole|']),
        ('pair_conv', 0): (418016, ['k_conv|', 'k_whole|']),
        ('fuse', 0): (418016, ['k_convp|k_convp<8, 1, 0, 24>', 'k_whole|']),
    }),
    (44100.0, 96000.0, 8192, 2.0, 180.15, 0): ('BlockConvolver: flt_len=1417 in_len=2680 io=2/1 fft=2048/4096 latency=3388 nfreq=0.5 tb=2 gain=2\nFracInterpolator: 88200->96000 whole=1 step=147/160 taps=24 fracs=160 order=0\n', {
        None: (168032, ['k_convp_whole|k_convp<11, 1, 4, 24>', 'k_whole|']),
        ('fast_conv', 0): (884960, ['k_conv|', 'k_whole|']),
        ('pair_conv', 0): (884960, ['k_convx_whole|k_convx<10, 1, 1, 24>', 'k_whole|']),
        ('pair_two', 0): (98528, ['k_convp_whole|k_convp<11, 1, 1, 24>', 'k_whole|']),
        ('fuse', 0): (884960, ['k_convp|k_convp<11, 1, 0, 24>', 'k_whole|']),
        ('park', 0): (98528, ['k_convp_whole|k_convp<11, 1, 4, 24>', 'k_whole|']),
        ('half_fused', 2): (168032, ['k_convp_whole|k_convp<11, 1, 23, 24>', 'k_whole|']),
    }),
    (44100.0, 132300.0, 1024, 2.0, 180.15, 0): ('BlockConvolver: flt_len=2127 in_len=6066 io=3/1 fft=8192/8192 latency=7129 nfreq=0.333333 tb=2 gain=3\n', {
        None: (293312, ['k_convp|k_convp<11, 0, 19, 24>']),
        ('fast_conv', 0): (196736, ['k_conv|']),
        ('pair_conv', 0): (589952, ['k_convx|k_convx<12, 0, 3, 24>']),
        ('up3_poly', 0): (342656, ['k_convp|k_convp<13, 0, 3, 24>']),
        ('park', 0): (196736, ['k_convp|k_convp<11, 0, 19, 24>']),
    }),
    (44100.0, 132300.0, 2048, 1.0, 180.15, 1): ('BlockConvolver: flt_len=4253 in_len=12132 io=3/1 fft=16384/16384 latency=12147 nfreq=0.333333 tb=1 gain=3\n', {
        None: (586496, ['k_convp|k_convp<12, 0, 19, 24>']),
        ('fast_conv', 0): (393344, ['k_conv|']),
        ('pair_conv', 0): (393344, ['k_conv|']),
        ('up3_poly', 0): (684800, ['k_convp|k_convp<13, 0, 15, 24>']),
        ('park', 0): (393344, ['k_convp|k_convp<12, 0, 19, 24>']),
    }),
    (44100.0, 132300.0, 3000, 0.5, 180.15, 0): ('BlockConvolver: flt_len=8507 in_len=24262 io=3/1 fft=32768/32768 latency=28515 nfreq=0.333333 tb=0.5 gain=3\n', {
        None: (582656, ['k_convp|k_convp<13, 0, 11, 24>']),
        ('fast_conv', 0): (393344, ['k_conv|']),
        ('pair_conv', 0): (1179776, ['k_convx|k_convx<13, 0, 3, 24>']),
        ('pair_solo', 0): (1179776, ['k_convx|k_convx<13, 0, 3, 24>']),
        ('park', 0): (393344, ['k_convp|k_convp<13, 0, 11, 24>']),
    }),
    (44100.0, 132300.0, 3000, 10.0, 109.56, 0): ('BlockConvolver: flt_len=261 in_len=764 io=3/1 fft=1024/1024 latency=894 nfreq=0.333333 tb=10 gain=3\n', {
        None: (43328, ['k_convp|k_convp<10, 0, 3, 24>']),
        ('fast_conv', 0): (24704, ['k_conv|']),
        ('pair_conv', 0): (417920, ['k_convx|k_convx<9, 0, 3, 24>']),
        ('park', 0): (24704, ['k_convp|k_convp<10, 0, 3, 24>']),
    }),
    (44100.0, 176400.0, 1024, 2.0, 180.15, 1): ('BlockConvolver: flt_len=1417 in_len=2680 io=2/1 fft=2048/4096 latency=2688 nfreq=0.5 tb=2 gain=2\nHBUpsampler: sti=0 third=0 taps=11 att=183.80\n', {
        None: (295136, ['k_convp|k_convp<11, 1, 6, 24>', 'k_hbup|']),
        ('fast_conv', 0): (295136, ['k_conv|', 'k_hbup|']),
        ('pair_conv', 0): (295136, ['k_conv|', 'k_hbup|']),
        ('half', 2): (295136, ['k_convp|k_convp<11, 1, 31, 24>', 'k_hbup|']),
    }),
    (44100.0, 192000.0, 1024, 2.0, 180.15, 1): ('BlockConvolver: flt_len=1417 in_len=2680 io=2/1 fft=2048/4096 latency=2688 nfreq=0.5 tb=2 gain=2\nFracInterpolator: 352800->192000 whole=1 step=147/80 taps=24 fracs=80 order=0\nBlockConvolver: flt_len=611 in_len=1438 io=2/1 fft=1024/2048 latency=1446 nfreq=0.5 tb=4.64286 gain=2\nHBUpsampler: sti=0 third=0 taps=11 att=183.80\n', {
        None: (393632, ['k_convp_whole|k_convp<11, 1, 17, 24>', 'k_whole|', 'k_convp|k_convp<10, 1, 6, 24>', 'k_hbup|']),
        ('fast_conv', 0): (590240, ['k_conv|', 'k_whole|', 'k_conv|', 'k_hbup|']),
        ('pair_conv', 0): (590240, ['k_conv|', 'k_whole|', 'k_conv|', 'k_hbup|']),
        ('pair_two', 0): (590240, ['k_convp|k_convp<11, 1, 6, 24>', 'k_whole|', 'k_convp|k_convp<10, 1, 6, 24>', 'k_hbup|']),
        ('fuse', 0): (590240, ['k_convp|k_convp<11, 1, 6, 24>', 'k_whole|', 'k_convp|k_convp<10, 1, 6, 24>', 'k_hbup|']),
        ('fuse_latency', 0): (590240, ['k_convp|k_convp<11, 1, 6, 24>', 'k_whole|', 'k_convp|k_convp<10, 1, 6, 24>', 'k_hbup|']),
        ('half_fused', 2): (393632, ['k_convp_whole|k_convp<11, 1, 30, 24>', 'k_whole|', 'k_convp|k_convp<10, 1, 6, 24>', 'k_hbup|']),
    }),
    (44100.0, 192000.0, 2048, 2.0, 180.15, 0): ('BlockConvolver: flt_len=1417 in_len=2680 io=2/1 fft=2048/4096 latency=3388 nfreq=0.5 tb=2 gain=2\nFracInterpolator: 352800->192000 whole=1 step=147/80 taps=24 fracs=80 order=0\nBlockConvolver: flt_len=611 in_len=1438 io=2/1 fft=1024/2048 latency=1743 nfreq=0.5 tb=4.64286 gain=2\nHBUpsampler: sti=0 third=0 taps=11 att=183.80\n', {
        None: (491936, ['k_convp_whole|k_convp<11, 1, 5, 24>', 'k_whole|', 'k_convp|k_convp<10, 1, 0, 24>', 'k_hbup|']),
        ('fast_conv', 0): (688544, ['k_conv|', 'k_whole|', 'k_conv|', 'k_hbup|']),
        ('pair_conv', 0): (491936, ['k_convx_whole|k_convx<10, 1, 1, 24>', 'k_whole|', 'k_convx|k_convx<9, 1, 0, 24>', 'k_hbup|']),
        ('pair_two', 0): (491936, ['k_convp_whole|k_convp<11, 1, 1, 24>', 'k_whole|', 'k_convp|k_convp<10, 1, 0, 24>', 'k_hbup|']),
        ('fuse', 0): (688544, ['k_convp|k_convp<11, 1, 0, 24>', 'k_whole|', 'k_convp|k_convp<10, 1, 0, 24>', 'k_hbup|']),
        ('half_fused', 2): (491936, ['k_convp_whole|k_convp<11, 1, 25, 24>', 'k_whole|', 'k_convp|k_convp<10, 1, 0, 24>', 'k_hbup|']),
    }),
    (44100.0, 2822400.0, 512, 2.0, 180.15, 1): ('BlockConvolver: flt_len=1417 in_len=2680 io=2/1 fft=2048/4096 latency=2688 nfreq=0.5 tb=2 gain=2\nHBUpsampler: sti=0 third=0 taps=11 att=183.80\nHBUpsampler: sti=1 third=0 taps=6 att=181.25\nHBUpsampler: sti=2 third=0 taps=5 att=213.50\nHBUpsampler: sti=3 third=0 taps=4 att=220.65\nHBUpsampler: sti=4 third=0 taps=3 att=203.30\n', {
        None: (197216, ['k_convp|k_convp<11, 1, 6, 24>', 'k_hbcascade|', 'k_hbcascade|', 'k_hbcascade|', 'k_hbcascade|', 'k_hbup|']),
        ('fast_conv', 0): (197216, ['k_conv|', 'k_hbcascade|', 'k_hbcascade|', 'k_hbcascade|', 'k_hbcascade|', 'k_hbup|']),
        ('pair_conv', 0): (197216, ['k_conv|', 'k_hbcascade|', 'k_hbcascade|', 'k_hbcascade|', 'k_hbcascade|', 'k_hbup|']),
        ('fuse_latency', 0): (1671776, ['k_convp|k_convp<11, 1, 6, 24>', 'k_hbup|', 'k_hbup|', 'k_hbup|', 'k_hbup|', 'k_hbup|']),
        ('fuse_hb', 0): (1671776, ['k_convp|k_convp<11, 1, 6, 24>', 'k_hbup|', 'k_hbup|', 'k_hbup|', 'k_hbup|', 'k_hbup|']),
        ('half', 2): (197216, ['k_convp|k_convp<11, 1, 31, 24>', 'k_hbcascade|', 'k_hbcascade|', 'k_hbcascade|', 'k_hbcascade|', 'k_hbup|']),
    }),
    (44100.0, 2822400.0, 1024, 2.0, 180.15, 0): ('BlockConvolver: flt_len=1417 in_len=2680 io=2/1 fft=2048/4096 latency=3388 nfreq=0.5 tb=2 gain=2\nHBUpsampler: sti=0 third=0 taps=11 att=183.80\nHBUpsampler: sti=1 third=0 taps=6 att=181.25\nHBUpsampler: sti=2 third=0 taps=5 att=213.50\nHBUpsampler: sti=3 third=0 taps=4 att=220.65\nHBUpsampler: sti=4 third=0 taps=3 att=203.30\n', {
        None: (295520, ['k_convp|k_convp<11, 1, 0, 24>', 'k_hbcascade|', 'k_hbcascade|', 'k_hbcascade|', 'k_hbcascade|', 'k_hbup|']),
        ('fast_conv', 0): (295520, ['k_conv|', 'k_hbcascade|', 'k_hbcascade|', 'k_hbcascade|', 'k_hbcascade|', 'k_hbup|']),
        ('pair_conv', 0): (295520, ['k_convx|k_convx<10, 1, 0, 24>', 'k_hbcascade|', 'k_hbcascade|', 'k_hbcascade|', 'k_hbcascade|', 'k_hbup|']),
        ('fuse_hb', 0): (3244640, ['k_convp|k_convp<11, 1, 0, 24>', 'k_hbup|', 'k_hbup|', 'k_hbup|', 'k_hbup|', 'k_hbup|']),
        ('half', 2): (295520, ['k_convp|k_convp<11, 1, 21, 24>', 'k_hbcascade|', 'k_hbcascade|', 'k_hbcascade|', 'k_hbcascade|', 'k_hbup|']),
        ('quad', 1): (295520, ['k_convp|k_convq', 'k_hbcascade|', 'k_hbcascade|', 'k_hbcascade|', 'k_hbcascade|', 'k_hbup|']),
    }),
    (48000.0, 16000.0, 8192, 0.5, 180.15, 0): ('BlockConvolver: flt_len=8507 in_len=24262 io=1/3 fft=32768/32768 latency=28515 nfreq=0.333333 tb=0.5 gain=1\n', {
        None: (1636352, ['k_convp|k_convp<13, 0, 11, 24>']),
        ('fast_conv', 0): (1572992, ['k_conv|']),
        ('pair_conv', 0): (1769600, ['k_convx|k_convx<13, 0, 3, 24>']),
        ('pair_solo', 0): (1769600, ['k_convx|k_convx<13, 0, 3, 24>']),
        ('park', 0): (1572992, ['k_convp|k_convp<13, 0, 11, 24>']),
    }),
    (48000.0, 16000.0, 8192, 1.0, 180.15, 1): ('BlockConvolver: flt_len=4253 in_len=12132 io=1/3 fft=16384/16384 latency=12147 nfreq=0.333333 tb=1 gain=1\n', {
        None: (883904, ['k_convp|k_convp<13, 0, 15, 24>']),
        ('fast_conv', 0): (786560, ['k_conv|']),
        ('pair_conv', 0): (786560, ['k_conv|']),
        ('pair_solo', 0): (786560, ['k_conv|']),
        ('park', 0): (786560, ['k_convp|k_convp<13, 0, 15, 24>']),
    }),
    (48000.0, 32000.0, 2048, 2.0, 180.15, 1): ('BlockConvolver: flt_len=2127 in_len=6066 io=2/3 fft=4096/8192 latency=6080 nfreq=0.333333 tb=2 gain=2\n', {
        None: (245504, ['k_convp|k_convp<12, 1, 7, 24>']),
        ('fast_conv', 0): (196736, ['k_conv|']),
        ('pair_conv', 0): (196736, ['k_conv|']),
        ('park', 0): (196736, ['k_convp|k_convp<12, 1, 7, 24>']),
        ('half', 2): (245504, ['k_convp|k_convp<12, 1, 32, 24>']),
    }),
    (48000.0, 32000.0, 4096, 0.5, 180.15, 0): ('BlockConvolver: flt_len=8507 in_len=24262 io=2/3 fft=16384/32768 latency=28515 nfreq=0.333333 tb=0.5 gain=2\n', {
        None: (849920, ['k_convp|k_convp<13, 0, 9, 24>']),
        ('pair_conv', 0): (983168, ['k_convx|k_convx<12, 1, 3, 24>']),
        ('pair_split', 0): (983168, ['k_convx|k_convx<12, 1, 3, 24>']),
        ('park', 0): (786560, ['k_convp|k_convp<13, 0, 9, 24>']),
    }),
    (48000.0, 32000.0, 4096, 0.5, 180.15, 1): ('BlockConvolver: flt_len=8507 in_len=24262 io=2/3 fft=16384/32768 latency=24277 nfreq=0.333333 tb=0.5 gain=2\n', {
        None: (849920, ['k_convp|k_convp<13, 0, 13, 24>']),
        ('park', 0): (786560, ['k_convp|k_convp<13, 0, 13, 24>']),
    }),
    (48000.0, 32000.0, 8192, 2.0, 180.15, 1): ('BlockConvolver: flt_len=2127 in_len=6066 io=2/3 fft=4096/8192 latency=6080 nfreq=0.333333 tb=2 gain=2\n', {
        None: (245504, ['k_convp|k_convp<12, 1, 7, 24>']),
        ('fast_conv', 0): (196736, ['k_conv|']),
        ('pair_conv', 0): (196736, ['k_conv|']),
        ('park', 0): (196736, ['k_convp|k_convp<12, 1, 7, 24>']),
        ('half', 2): (245504, ['k_convp|k_convp<12, 1, 32, 24>']),
    }),
    (48000.0, 32000.0, 16384, 2.0, 180.15, 0): ('BlockConvolver: flt_len=2127 in_len=6066 io=2/3 fft=4096/8192 latency=7129 nfreq=0.333333 tb=2 gain=2\n', {
        None: (245504, ['k_convp|k_convp<12, 1, 3, 24>']),
        ('fast_conv', 0): (196736, ['k_conv|']),
        ('pair_conv', 0): (589952, ['k_convx|k_convx<11, 1, 3, 24>']),
        ('park', 0): (196736, ['k_convp|k_convp<12, 1, 3, 24>']),
        ('half', 2): (245504, ['k_convp|k_convp<12, 1, 22, 24>']),
    }),
    (48000.0, 36000.0, 6000, 0.7, 180.15, 0): ('BlockConvolver: flt_len=8103 in_len=8280 io=3/4 fft=16384/4096 latency=12331 nfreq=0.25 tb=0.7 gain=3\n', {
        None: (443264, ['k_convp|k_convp<13, -2, 11, 24>']),
        ('fast_conv', 0): (393344, ['k_conv|']),
        ('pair_conv', 0): (589952, ['k_convx|k_convx<13, -2, 3, 24>']),
        ('pair_solo', 0): (589952, ['k_convx|k_convx<13, -2, 3, 24>']),
        ('park', 0): (393344, ['k_convp|k_convp<13, -2, 11, 24>']),
    }),
    (48000.0, 44100.0, 6000, 2.0, 109.56, 0): ('BlockConvolver: flt_len=947 in_len=1102 io=2/1 fft=1024/2048 latency=1575 nfreq=0.459375 tb=2 gain=2\nFracInterpolator: 96000->44100 whole=1 step=320/147 taps=14 fracs=147 order=0\n', {
        None: (61664, ['k_convp_whole|k_convp<10, 1, 5, 24>', 'k_whole|']),
        ('fast_conv', 0): (442592, ['k_conv|', 'k_whole|']),
        ('pair_conv', 0): (245984, ['k_convx_whole|k_convx<9, 1, 1, 24>', 'k_whole|']),
        ('pair_two', 0): (49376, ['k_convp_whole|k_convp<10, 1, 1, 24>', 'k_whole|']),
        ('fuse', 0): (442592, ['k_convp|k_convp<10, 1, 0, 24>', 'k_whole|']),
        ('park', 0): (49376, ['k_convp_whole|k_convp<10, 1, 5, 24>', 'k_whole|']),
    }),
    (64000.0, 48000.0, 2048, 2.0, 180.15, 1): ('BlockConvolver: flt_len=2835 in_len=5356 io=3/4 fft=8192/2048 latency=5377 nfreq=0.25 tb=2 gain=3\n', {
        None: (229184, ['k_convp|k_convp<13, -2, 7, 24>']),
        ('fast_conv', 0): (196736, ['k_conv|']),
        ('pair_conv', 0): (196736, ['k_conv|']),
        ('park', 0): (196736, ['k_convp|k_convp<13, -2, 7, 24>']),
    }),
    (88200.0, 44100.0, 2048, 2.0, 180.15, 1): ('BlockConvolver: flt_len=1417 in_len=2680 io=1/2 fft=4096/2048 latency=2688 nfreq=0.5 tb=2 gain=1\n', {
        None: (229184, ['k_convp|k_convp<12, -1, 6, 24>']),
        ('fast_conv', 0): (196736, ['k_conv|']),
        ('pair_conv', 0): (196736, ['k_conv|']),
        ('park', 0): (196736, ['k_convp|k_convp<12, -1, 6, 24>']),
    }),
    (88200.0, 44100.0, 8192, 0.5, 180.15, 1): ('BlockConvolver: flt_len=5671 in_len=10714 io=1/2 fft=16384/8192 latency=10722 nfreq=0.5 tb=0.5 gain=1\n', {
        None: (915392, ['k_convp|k_convp<13, -1, 14, 24>']),
        ('park', 0): (786560, ['k_convp|k_convp<13, -1, 14, 24>']),
    }),
    (88200.0, 44100.0, 12000, 2.0, 180.15, 0): ('BlockConvolver: flt_len=1417 in_len=2680 io=1/2 fft=4096/2048 latency=3388 nfreq=0.5 tb=2 gain=1\n', {
        None: (229184, ['k_convp|k_convp<12, -1, 0, 24>']),
        ('fast_conv', 0): (196736, ['k_conv|']),
        ('pair_conv', 0): (393344, ['k_convx|k_convx<11, -1, 0, 24>']),
        ('park', 0): (196736, ['k_convp|k_convp<12, -1, 0, 24>']),
        ('half', 2): (229184, ['k_convp|k_convp<12, -1, 27, 24>']),
    }),
    (96000.0, 44100.0, 2048, 2.0, 180.15, 1): ('BlockConvolver: flt_len=1543 in_len=2554 io=1/1 fft=4096/4096 latency=2563 nfreq=0.459375 tb=2 gain=1\nFracInterpolator: 96000->44100 whole=1 step=320/147 taps=24 fracs=147 order=0\n', {
        None: (226592, ['k_convp_whole|k_convp<12, 0, 17, 24>', 'k_whole|']),
        ('fast_conv', 0): (393440, ['k_conv|', 'k_whole|']),
        ('pair_conv', 0): (393440, ['k_conv|', 'k_whole|']),
        ('pair_two', 0): (393440, ['k_convp|k_convp<12, 0, 6, 24>', 'k_whole|']),
        ('fuse', 0): (393440, ['k_convp|k_convp<12, 0, 6, 24>', 'k_whole|']),
        ('fuse_latency', 0): (393440, ['k_convp|k_convp<12, 0, 6, 24>', 'k_whole|']),
        ('park', 0): (196832, ['k_convp_whole|k_convp<12, 0, 17, 24>', 'k_whole|']),
    }),
    (96000.0, 44100.0, 4096, 2.0, 180.15, 1): ('BlockConvolver: flt_len=1543 in_len=2554 io=1/1 fft=4096/4096 latency=2563 nfreq=0.459375 tb=2 gain=1\nFracInterpolator: 96000->44100 whole=1 step=320/147 taps=24 fracs=147 order=0\n', {
        None: (226592, ['k_convp_whole|k_convp<12, 0, 17, 24>', 'k_whole|']),
        ('fast_conv', 0): (393440, ['k_conv|', 'k_whole|']),
        ('pair_conv', 0): (393440, ['k_conv|', 'k_whole|']),
        ('pair_two', 0): (393440, ['k_convp|k_convp<12, 0, 6, 24>', 'k_whole|']),
        ('fuse', 0): (393440, ['k_convp|k_convp<12, 0, 6, 24>', 'k_whole|']),
        ('fuse_latency', 0): (393440, ['k_convp|k_convp<12, 0, 6, 24>', 'k_whole|']),
        ('park', 0): (196832, ['k_convp_whole|k_convp<12, 0, 17, 24>', 'k_whole|']),
    }),
    (96000.0, 44100.0, 8192, 0.5, 180.15, 0): ('BlockConvolver: flt_len=6173 in_len=10212 io=1/1 fft=16384/16384 latency=13298 nfreq=0.459375 tb=0.5 gain=1\nFracInterpolator: 96000->44100 whole=1 step=320/147 taps=24 fracs=147 order=0\n', {
        None: (899360, ['k_convp_whole|k_convp<13, 0, 18, 24>', 'k_whole|']),
        ('fast_conv', 0): (1573088, ['k_conv|', 'k_whole|']),
        ('pair_conv', 0): (1179872, ['k_convx_whole|k_convx<13, 0, 1, 24>', 'k_whole|']),
        ('pair_solo', 0): (1179872, ['k_convx_whole|k_convx<13, 0, 1, 24>', 'k_whole|']),
        ('solo_fuse', 0): (1573088, ['k_convp|k_convp<13, 0, 10, 24>', 'k_whole|']),
        ('fuse', 0): (1573088, ['k_convp|k_convp<13, 0, 10, 24>', 'k_whole|']),
        ('park', 0): (786656, ['k_convp_whole|k_convp<13, 0, 18, 24>', 'k_whole|']),
    }),
    (96000.0, 44100.0, 8192, 0.5, 180.15, 1): ('BlockConvolver: flt_len=6173 in_len=10212 io=1/1 fft=16384/16384 latency=10222 nfreq=0.459375 tb=0.5 gain=1\nFracInterpolator: 96000->44100 whole=1 step=320/147 taps=24 fracs=147 order=0\n', {
        None: (1573088, ['k_convp|k_convp<13, 0, 14, 24>', 'k_whole|']),
        ('fast_conv', 0): (1573088, ['k_conv|', 'k_whole|']),
        ('pair_conv', 0): (1573088, ['k_conv|', 'k_whole|']),
        ('pair_solo', 0): (1573088, ['k_conv|', 'k_whole|']),
    }),
    (96000.0, 44100.0, 16384, 2.0, 180.15, 0): ('BlockConvolver: flt_len=1543 in_len=2554 io=1/1 fft=4096/4096 latency=3325 nfreq=0.459375 tb=2 gain=1\nFracInterpolator: 96000->44100 whole=1 step=320/147 taps=24 fracs=147 order=0\n', {
        None: (225056, ['k_convp_whole|k_convp<12, 0, 5, 24>', 'k_whole|']),
        ('fast_conv', 0): (983264, ['k_conv|', 'k_whole|']),
        ('pair_conv', 0): (590048, ['k_convx_whole|k_convx<11, 0, 1, 24>', 'k_whole|']),
        ('pair_two', 0): (196832, ['k_convp_whole|k_convp<12, 0, 1, 24>', 'k_whole|']),
        ('fuse', 0): (983264, ['k_convp|k_convp<12, 0, 0, 24>', 'k_whole|']),
        ('park', 0): (196832, ['k_convp_whole|k_convp<12, 0, 5, 24>', 'k_whole|']),
        ('half_fused', 2): (225056, ['k_convp_whole|k_convp<12, 0, 33, 24>', 'k_whole|']),
    }),
    (176400.0, 44100.0, 4096, 2.0, 180.15, 0): ('HBDownsampler: sti=0 third=0 taps=11 att=183.80\nBlockConvolver: flt_len=1417 in_len=2680 io=1/2 fft=4096/2048 latency=3388 nfreq=0.5 tb=2 gain=0.5\n', {
        None: (819104, ['k_hbdown|', 'k_convp|k_convp<12, -1, 0, 24>']),
        ('fast_conv', 0): (786656, ['k_hbdown|', 'k_conv|']),
        ('pair_conv', 0): (884960, ['k_hbdown|', 'k_convx|k_convx<11, -1, 0, 24>']),
        ('park', 0): (786656, ['k_hbdown|', 'k_convp|k_convp<12, -1, 0, 24>']),
        ('fuse_hbconv', 1): (425888, ['k_convp_hb|k_convp<12, -1, 20, 24>', 'k_convp|']),
        ('half', 2): (819104, ['k_hbdown|', 'k_convp|k_convp<12, -1, 27, 24>']),
    }),
    (176400.0, 44100.0, 4096, 2.0, 180.15, 1): ('HBDownsampler: sti=0 third=0 taps=11 att=183.80\nBlockConvolver: flt_len=1417 in_len=2680 io=1/2 fft=4096/2048 latency=2688 nfreq=0.5 tb=2 gain=0.5\n', {
        None: (428960, ['k_hbdown|', 'k_convp|k_convp<12, -1, 6, 24>']),
        ('fast_conv', 0): (396512, ['k_hbdown|', 'k_conv|']),
        ('pair_conv', 0): (396512, ['k_hbdown|', 'k_conv|']),
        ('park', 0): (396512, ['k_hbdown|', 'k_convp|k_convp<12, -1, 6, 24>']),
    }),
    (176400.0, 44100.0, 9000, 2.0, 180.15, 0): ('HBDownsampler: sti=0 third=0 taps=11 att=183.80\nBlockConvolver: flt_len=1417 in_len=2680 io=1/2 fft=4096/2048 latency=3388 nfreq=0.5 tb=2 gain=0.5\n', {
        None: (819104, ['k_hbdown|', 'k_convp|k_convp<12, -1, 0, 24>']),
        ('fast_conv', 0): (786656, ['k_hbdown|', 'k_conv|']),
        ('pair_conv', 0): (884960, ['k_hbdown|', 'k_convx|k_convx<11, -1, 0, 24>']),
        ('park', 0): (786656, ['k_hbdown|', 'k_convp|k_convp<12, -1, 0, 24>']),
        ('fuse_hbconv', 1): (425888, ['k_convp_hb|k_convp<12, -1, 20, 24>', 'k_convp|']),
        ('half', 2): (819104, ['k_hbdown|', 'k_convp|k_convp<12, -1, 27, 24>']),
    }),
    (176400.0, 44100.0, 16384, 0.5, 180.15, 0): ('HBDownsampler: sti=0 third=0 taps=11 att=183.80\nBlockConvolver: flt_len=5671 in_len=10714 io=1/2 fft=16384/8192 latency=13549 nfreq=0.5 tb=0.5 gain=0.5\n', {
        None: (1704992, ['k_hbdown|', 'k_convp|k_convp<13, -1, 10, 24>']),
        ('pair_conv', 0): (1969376, ['k_hbdown|', 'k_convx|k_convx<13, -1, 0, 24>']),
        ('pair_solo', 0): (1969376, ['k_hbdown|', 'k_convx|k_convx<13, -1, 0, 24>']),
        ('park', 0): (1576160, ['k_hbdown|', 'k_convp|k_convp<13, -1, 10, 24>']),
    }),
    (176400.0, 44100.0, 16384, 0.5, 180.15, 1): ('HBDownsampler: sti=0 third=0 taps=11 att=183.80\nBlockConvolver: flt_len=5671 in_len=10714 io=1/2 fft=16384/8192 latency=10722 nfreq=0.5 tb=0.5 gain=0.5\n', {
        None: (1704992, ['k_hbdown|', 'k_convp|k_convp<13, -1, 14, 24>']),
        ('park', 0): (1576160, ['k_hbdown|', 'k_convp|k_convp<13, -1, 14, 24>']),
    }),
    (192000.0, 44100.0, 8192, 0.5, 180.15, 0): ('HBDownsampler: sti=0 third=0 taps=11 att=183.80\nBlockConvolver: flt_len=6173 in_len=10212 io=1/1 fft=16384/16384 latency=13298 nfreq=0.459375 tb=0.5 gain=0.5\nFracInterpolator: 192000->88200 whole=1 step=320/147 taps=24 fracs=147 order=0\n', {
        None: (1688960, ['k_hbdown|', 'k_convp_whole|k_convp<13, 0, 18, 24>', 'k_whole|']),
        ('fast_conv', 0): (1969472, ['k_hbdown|', 'k_conv|', 'k_whole|']),
        ('pair_conv', 0): (1772864, ['k_hbdown|', 'k_convx_whole|k_convx<13, 0, 1, 24>', 'k_whole|']),
        ('pair_solo', 0): (1772864, ['k_hbdown|', 'k_convx_whole|k_convx<13, 0, 1, 24>', 'k_whole|']),
        ('solo_fuse', 0): (1969472, ['k_hbdown|', 'k_convp|k_convp<13, 0, 10, 24>', 'k_whole|']),
        ('fuse', 0): (1969472, ['k_hbdown|', 'k_convp|k_convp<13, 0, 10, 24>', 'k_whole|']),
        ('park', 0): (1576256, ['k_hbdown|', 'k_convp_whole|k_convp<13, 0, 18, 24>', 'k_whole|']),
    }),
    (2822400.0, 176400.0, 4096, 2.0, 180.15, 0): ('HBDownsampler: sti=2 third=0 taps=5 att=213.50\nHBDownsampler: sti=1 third=0 taps=6 att=181.25\nHBDownsampler: sti=0 third=0 taps=11 att=183.80\nBlockConvolver: flt_len=1417 in_len=2680 io=1/2 fft=4096/2048 latency=3388 nfreq=0.5 tb=2 gain=0.125\n', {
        None: (241760, ['k_hbdcascade|', 'k_hbdcascade|', 'k_hbdown|', 'k_convp|k_convp<12, -1, 0, 24>']),
        ('fast_conv', 0): (209312, ['k_hbdcascade|', 'k_hbdcascade|', 'k_hbdown|', 'k_conv|']),
        ('pair_conv', 0): (258464, ['k_hbdcascade|', 'k_hbdcascade|', 'k_hbdown|', 'k_convx|k_convx<11, -1, 0, 24>']),
        ('fuse_hb', 0): (733280, ['k_hbdown|', 'k_hbdown|', 'k_hbdown|', 'k_convp|k_convp<12, -1, 0, 24>']),
        ('fuse_hbd', 0): (733280, ['k_hbdown|', 'k_hbdown|', 'k_hbdown|', 'k_convp|k_convp<12, -1, 0, 24>']),
        ('park', 0): (209312, ['k_hbdcascade|', 'k_hbdcascade|', 'k_hbdown|', 'k_convp|k_convp<12, -1, 0, 24>']),
        ('fuse_hbconv', 1): (438368, ['k_hbdcascade|', 'k_hbdown|', 'k_convp_hb|k_convp<12, -1, 20, 24>', 'k_convp|']),
        ('half', 2): (241760, ['k_hbdcascade|', 'k_hbdcascade|', 'k_hbdown|', 'k_convp|k_convp<12, -1, 27, 24>']),
    }),
}


@pytest.mark.parametrize("chain", FORM_CHAINS)
def test_emulated_stage_forms_are_pinned(emul, chain):
    """the kernel form of every stage -- the engine's label and, for the compile-time-sized convolvers, the kernel symbol
    with its mode --, the chain's describe() text and state_size, under the default options and with each structural
    choice flipped singly: as recorded before the per-stage record (StageForm) replaced the predicates"""
    text, pins = FORM_PINS[chain]
    assert set(pins) <= set(FORM_VARIANTS)
    for variant in FORM_VARIANTS:
        d, size, stages = form_probe(emul, chain, variant)
        assert d == text, (variant, d)
        assert (size, ["%s|%s" % tuple(st) for st in stages]) == pins.get(variant, pins[None]), (variant, size, stages)
