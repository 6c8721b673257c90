"""Pins the oracle (oracle/r8b_oracle.py, numpy restatement) against
  (a) the committed golden fixtures generated from the real reference (tests/golden/),
  (b) the known-answer vectors of SURVEY.md Appendix B,
  (c) the real reference itself (oracle/_ref) when it is available.
CPU only.  Tolerances: SURVEY.md section 8(c) -- RMS <= 1e-15, peak <= 1e-13 on +-1.0 noise
(the reference's own cross-build noise floor is 3e-16 / 2.3e-15).
"""
import json
import os

import numpy as np
import pytest

import cases
import r8b_oracle as O
from conftest import GOLDEN, rms, peak

RMS_TOL = 1e-15
PEAK_TOL = 1e-13

CASE_NAMES = ["cfg2_44k_96k", "cfg3_96k_44k", "cfg5_44k_2822k", "hbdown_176k_44k",
              "sacd_down_2822k_176k", "poly_44100_44101", "up3_44k_132k", "down3_48k_32k",
              "ratio32_32k_48k", "interm_44k_192k", "res16_44k_48k", "res16ir_48k_44k",
              "impulse_44k_96k"]


def case_input(params):
    src, dst, maxin, chunk, n, tb, att, seed = params
    n, seed = int(n), int(seed)
    if seed == 0:
        x = np.zeros(n)
        x[0] = 1.0
    else:
        x = O.splitmix_uniform(seed, n)
    return src, dst, int(maxin), int(chunk), x, tb, att


def test_splitmix_kat():
    # SURVEY Appendix B lists the three values in reverse (printf argument order); the stream
    # order is pinned by KAT 1 below, which reproduces the reference's outputs from seed 1.
    v = O.splitmix_uniform(42, 3)
    assert v[0] == 0.48312975754364662
    assert v[1] == -0.68017921424615979
    assert v[2] == -0.44279773948972267


@pytest.mark.parametrize("name", CASE_NAMES)
def test_oracle_matches_golden_stream(golden_streams, name):
    src, dst, maxin, chunk, x, tb, att = case_input(golden_streams[name + "/params"])
    o = O.OracleResampler(src, dst, maxin, tb, att)
    outs = [o.process(x[i:i + chunk]) for i in range(0, len(x), chunk)]
    counts = np.array([len(v) for v in outs])
    assert np.array_equal(counts, golden_streams[name + "/counts"])
    y = np.concatenate(outs)
    g = golden_streams[name + "/y"]
    y = y[:len(g)]
    assert rms(y - g) <= RMS_TOL and peak(y - g) <= PEAK_TOL, (rms(y - g), peak(y - g))


def test_appendix_b_kats():
    """SURVEY.md Appendix B (generated from the reference in the survey session)."""
    kats = [
        (44100.0, 96000.0, 16384, 1, [31966, 35666, 35665, 35666, 35666, 35666],
         [0.16836127972661949, 0.23875843113075113, 0.40333285862527624, 0.74279777311647388],
         281627, 416.32782402753885, 91935.459564724697),
        (96000.0, 44100.0, 16384, 1, [5994, 7526, 7527, 7526, 7527, 7526],
         [0.35835467097959206, 0.37844316656790128, 0.2180723565225566, 0.35991812420970659],
         58679, 74.200982314605877, 8844.2688919531152),
        (44100.0, 96000.0, 1024, 7, [0, 758, 2229, 2229, 2229, 2230],
         [-0.25545409978296257, -0.85844298828084797, -0.99717659157724259,
          -0.33971927734210905], 14133, -61.230530042340409, 4543.154761789436),
    ]
    for src, dst, L, seed, counts6, first4, total, sy, sy2 in kats:
        o = O.OracleResampler(src, dst, L)
        x = O.splitmix_uniform(seed, L * 8)
        outs = [o.process(x[i * L:(i + 1) * L]) for i in range(8)]
        assert [len(v) for v in outs[:6]] == counts6
        y = np.concatenate(outs)
        assert len(y) == total
        assert np.allclose(y[:4], first4, rtol=0, atol=5e-15)
        assert abs(y.sum() - sy) < 1e-9 and abs((y * y).sum() - sy2) < 1e-7


def test_appendix_b_dsd_counts():
    o = O.OracleResampler(44100.0, 2822400.0, 1024)
    x = O.splitmix_uniform(1, 1024 * 4)
    counts = [len(o.process(x[i * 1024:(i + 1) * 1024])) for i in range(4)]
    assert counts == [0, 22146, 65536, 65536]


def test_appendix_b_impulse():
    for src, dst, n, first6 in [
        (44100.0, 96000.0, 31966, [0.98220881966260754, 0.70425124515306403, 0.0851759876575129,
                                   -0.19274720254103048, -0.10817635155028549,
                                   0.10402549873820793]),
        (96000.0, 44100.0, 5994, [0.45120217653234385, 0.015903101647205486,
                                  -0.0058019483195100655, 0.0083755005728551428,
                                  -0.0080890341004010644, 0.008051083784245041])]:
        o = O.OracleResampler(src, dst, 16384)
        x = np.zeros(16384)
        x[0] = 1.0
        y = o.process(x)
        assert len(y) == n
        assert np.allclose(y[:6], first6, rtol=0, atol=2e-15)


def test_lp_filter_tables(golden_tables):
    i = 0
    while "lp%d/params" % i in golden_tables:
        nf, tb, att, g, klen, bits, lat = golden_tables["lp%d/params" % i]
        f = O.lp_filter(nf, tb, att, g)
        assert f["kernel_len"] == int(klen) and f["block_len_bits"] == int(bits)
        assert f["fl2"] == int(lat)
        n = 2 << int(bits)
        hz = np.zeros(n)
        hz[:f["fl2"] + 1] = f["taps"][f["fl2"]:]
        hz[n - f["fl2"]:] = f["taps"][:f["fl2"]]
        H = np.fft.rfft(hz).real * (2.0 / n)  # reference block is pre-scaled by InvMulConst
        Hg = golden_tables["lp%d/H" % i]
        assert peak(H - Hg) <= 4e-16 * peak(Hg) + 1e-18
        i += 1
    assert i >= 5
    # Appendix B table KAT
    Hg = golden_tables["lp0/H"]
    assert Hg[0] == 0.00097656249999999967
    assert abs(Hg[1] - 0.00097656250000218337) < 1e-18


def test_frac_bank_tables(golden_tables):
    i = 0
    while "ws%d/params" % i in golden_tables:
        fr, att, third, flen = golden_tables["ws%d/params" % i]
        b = O.frac_bank(int(fr), 1, 2, att, bool(third))
        assert b["filter_len"] == int(flen)
        assert peak(b["table"] - golden_tables["ws%d/table" % i]) <= 2e-15
        i += 1
    assert i >= 3
    i = 0
    while "poly%d/params" % i in golden_tables:
        att, third, flen, fracs = golden_tables["poly%d/params" % i]
        b = O.frac_bank(-1, 3, 8, att, bool(third))
        assert b["filter_len"] == int(flen) and b["fracs"] == int(fracs)
        rows = golden_tables["poly%d/rows" % i]
        assert peak(b["table"][rows] - golden_tables["poly%d/table" % i]) <= 1e-14
        i += 1
    assert i >= 2
    # Appendix B: bank(160) filter 1 taps 10..13
    t = O.frac_bank(160, 1, 2, 180.15, False)["table"]
    assert np.allclose(t[1][10:14], [-0.0058312762850098367, 0.99993331793992124,
                                     0.0059138397855352867, -0.0024442971837628563],
                       rtol=0, atol=1e-15)
    assert abs(t[0][11] - 1.0) < 1e-15


def test_inlen_matches_golden():
    with open(os.path.join(GOLDEN, "inlen.json")) as f:
        g = json.load(f)
    with np.load(os.path.join(GOLDEN, "streams.npz")) as st:
        for name, rec in g.items():
            src, dst, maxin, chunk, n, tb, att, seed = st[name + "/params"]
            o = O.OracleResampler(src, dst, int(maxin), tb, att)
            assert o.max_out_len == rec["max_out_len"], name
            assert [o.input_required(k) for k in rec["n"]] == rec["inlen"], name


def test_chunk_invariance():
    x = O.splitmix_uniform(11, 9000)
    ref = None
    for chunk in (1024, 1000, 777, 64):
        o = O.OracleResampler(44100.0, 96000.0, 1024)
        y = o.stream(x, chunk)
        if ref is None:
            ref = y
        else:
            assert len(y) == len(ref) and np.array_equal(y, ref)


def test_clear_restores_state():
    x = O.splitmix_uniform(5, 5000)
    o = O.OracleResampler(96000.0, 44100.0, 1024)
    y1 = o.stream(x, 1000)
    o.clear()
    y2 = o.stream(x, 1000)
    assert np.array_equal(y1, y2)


# ------------------------------------------------------------------ against the real reference

REF_CASES = [
    (44100.0, 96000.0, 16384, 16384, 16384 * 3, 2.0, 180.15),
    (96000.0, 44100.0, 16384, 16384, 16384 * 3, 2.0, 180.15),
    (44100.0, 2822400.0, 1024, 1024, 4096, 2.0, 180.15),
    (176400.0, 44100.0, 4096, 1000, 30000, 2.0, 180.15),
    (44100.0, 44101.0, 1024, 100, 5000, 2.0, 180.15),
    (44100.0, 96000.0, 1024, 1, 2500, 2.0, 180.15),
    (48000.0, 44111.0, 512, 512, 5000, 2.0, 136.45),
    (64000.0, 48000.0, 1024, 333, 15000, 2.0, 180.15),
    (11025.0, 96000.0, 512, 512, 3000, 2.0, 136.45),
    (96000.0, 11025.0, 512, 512, 30000, 2.0, 136.45),
    (44100.0, 529200.0, 512, 512, 3000, 2.0, 180.15),
    (96000.0, 48000.0, 512, 512, 9000, 5.0, 109.56),
    (44100.0, 48000.0, 512, 512, 9000, 0.5, 109.56),
    (44100.0, 88200.0, 512, 512, 6000, 45.0, 49.0),
]


@pytest.mark.parametrize("case", REF_CASES)
def test_oracle_matches_real_reference(refwrap, case):
    src, dst, maxin, chunk, n, tb, att = case
    x = O.splitmix_uniform(123, n)
    r = refwrap.RefResampler(src, dst, maxin, tb, att)
    o = O.OracleResampler(src, dst, maxin, tb, att)
    for i in range(0, n, chunk):
        a = r.process(x[i:i + chunk])
        b = o.process(x[i:i + chunk])
        assert len(a) == len(b)
        if len(a):
            assert rms(a - b) <= RMS_TOL and peak(a - b) <= PEAK_TOL, (i, rms(a - b), peak(a - b))
    for p in (0, 1, 2, 3, 17, 1000, 54321):
        assert r.inlen_before_outpos(p) == o.in_len_before_out_pos(p)
    assert r.maxout == o.max_out_len


def test_reference_c_abi_matches_shim(refwrap):
    """The reference's own DLL C ABI (DLL/r8bsrc.cpp) and the shim agree bit for bit."""
    import ctypes as C
    d = refwrap.dll()
    x = O.splitmix_uniform(9, 4096)
    h = d.r8b_create(44100.0, 96000.0, 1024, 2.0, 2)
    r = refwrap.RefResampler(44100.0, 96000.0, 1024, 2.0, 180.15)
    for i in range(0, 4096, 1024):
        xin = np.ascontiguousarray(x[i:i + 1024])
        op = C.POINTER(C.c_double)()
        n = d.r8b_process(h, xin.ctypes.data_as(C.POINTER(C.c_double)), 1024, C.byref(op))
        a = np.ctypeslib.as_array(op, shape=(n,)).copy() if n else np.zeros(0)
        b = r.process(xin)
        assert n == len(b) and np.array_equal(a, b)
    assert d.r8b_inlen(h, 1) == r.input_required(1)
    d.r8b_delete(h)


# ------------------------------------------------------------------ skip_silence(): hours of leading silence

# (src, dst, maxin, tb, atten): every stage kind the closed forms know, in every position of a chain
SKIP_CHAINS = [
    (44100.0, 96000.0, 1024, 2.0, 136.45), (96000.0, 44100.0, 1024, 2.0, 136.45), (44100.0, 2822400.0, 256, 2.0, 136.45),
    (2822400.0, 176400.0, 2048, 2.0, 136.45), (176400.0, 44100.0, 1024, 2.0, 136.45), (44100.0, 132300.0, 512, 2.0, 136.45),
    (48000.0, 32000.0, 512, 2.0, 136.45), (64000.0, 48000.0, 512, 2.0, 136.45), (32000.0, 48000.0, 512, 2.0, 136.45),
    (11025.0, 96000.0, 256, 2.0, 136.45), (44100.0, 192000.0, 256, 2.0, 136.45),
]


def run_behind_silence(make, chain, T, real):
    """T zero samples -- fed in calls of MaxInLen (real) or skipped --, then noise in calls of MaxInLen, three calls
    past the chain's latency: (outputs of the silence, [outputs of each call])"""
    o = make(*chain)
    maxin = chain[2]
    ncalls = O.OracleResampler(*chain).in_len_before_out_pos(0) // maxin + 4
    if real:
        nz = 0
        for i in range(0, T, maxin):
            y = o.process(np.zeros(min(maxin, T - i)))
            assert not np.any(y)
            nz += len(y)
    else:
        nz = o.skip_silence(T)
    x = O.splitmix_uniform(7, maxin * ncalls)
    return nz, [o.process(x[i:i + maxin]) for i in range(0, len(x), maxin)]


@pytest.mark.parametrize("chain", SKIP_CHAINS)
def test_skip_silence_equals_real_zeros(chain):
    T = 3 * chain[2] + 17
    nz_a, ya = run_behind_silence(O.OracleResampler, chain, T, True)
    nz_b, yb = run_behind_silence(O.OracleResampler, chain, T, False)
    assert nz_a == nz_b
    assert sum(len(y) for y in ya) > 0
    for u, v in zip(ya, yb):
        assert len(u) == len(v) and np.array_equal(u, v)


@pytest.mark.parametrize("chain", SKIP_CHAINS)
def test_skip_silence_past_2_31_and_2_32(chain):
    """the chain input crosses the boundary in the second call of noise: counts per call and levels are those of the
    same chain at small positions (the counts to the one sample by which a call's share depends on the position)"""
    src, dst, maxin = chain[:3]
    lat = O.OracleResampler(*chain).in_len_before_out_pos(0)
    _, near = run_behind_silence(O.OracleResampler, chain, lat + 3 * maxin + 17, False)
    for B in (1 << 31, 1 << 32):
        o = O.OracleResampler(*chain)
        nz = o.skip_silence(B - maxin - 5)
        assert abs(nz - (B - maxin - 5 - lat) * dst / src) <= len(o.stages) * max(1.0, dst / src) + 2   # (lat truncates once per stage)
        nz2, far = run_behind_silence(O.OracleResampler, chain, B - maxin - 5, False)
        assert nz2 == nz
        assert abs(sum(len(y) for y in far) - sum(len(y) for y in near)) <= 2 * dst / src + 2
        yf, yn = np.concatenate(far), np.concatenate(near)
        assert 0.5 * rms(yn) < rms(yf) < 2.0 * rms(yn) and peak(yf) < 2.0 * peak(yn)


def test_skip_silence_refuses_what_it_cannot_do():
    o = O.OracleResampler(44100.0, 44101.0, 1024)
    with pytest.raises(ValueError):
        o.skip_silence(10)
    assert all(getattr(s, "zeros", 0) == 0 for s in o.stages)   # nothing moved
    o = O.OracleResampler(44100.0, 96000.0, 1024)
    o.process(np.zeros(5))
    with pytest.raises(ValueError):
        o.skip_silence(10)


@pytest.mark.parametrize("chain", SKIP_CHAINS)
def test_skip_silence_matches_real_reference(refwrap, chain):
    """the compiled reference fed real zeros, then noise, against the oracle that skipped them"""
    T = 3 * chain[2] + 17
    nz_r, yr = run_behind_silence(refwrap.RefResampler, chain, T, True)
    nz_o, yo = run_behind_silence(O.OracleResampler, chain, T, False)
    assert nz_r == nz_o
    for a, b in zip(yr, yo):
        assert len(a) == len(b)
        if len(a):
            sc = cases.tol_scale(float(np.sum(a * a)), len(a))
            assert rms(a - b) <= RMS_TOL * sc and peak(a - b) <= PEAK_TOL * sc, (rms(a - b), peak(a - b))
