"""The fused half-array pair kernels' final-store phase after its integer diet (r8b_convp.h: cp_final_store<.., HAF>, whose
lanes leave at the first element past in_len instead of masking all sixteen; cp_rows2_fetch, whose 25 / 27 row loads share
one lane offset; cp_nonzero_bits / cp_level_words, which form a sample's high word without its sign once), on both tiers
like tests/test_lone_sample.py: the emulation tier (CPU, tests/emul -- the same bodies compiled for the host) and the GPU
tier (-m gpu).

Small objects -- 3 channels (one full pair and a lone channel whose partner row does not exist) and 4, MaxInLen 4096 --
with the half-array fused form forced (option half_fused = 2) and the symbol that ran asserted from stage_symbols().  One
conversion per code path (CASES); each feeds 12 000 samples of splitmix noise per channel, about nine convolver blocks:
the blocks that hold the stream's start (zeros in front of the run), interior blocks, the last block with parked outputs.

Every case runs twice, cut into calls two ways; the second cut has a call that ends one sample short of a block boundary
-- found from the object's own block counter, _cuts -- and a one-sample call behind it, which completes that block.  Asserted:
  1. the two cuts are bitwise equal;
  2. every channel is inside the project's bound (cases.RMS_TOL / PEAK_TOL: RMS 1e-15, peak 1e-13 of the channel's level,
     full scale here) against the compiled reference (refwrap.batch_check), the minimum-phase case on the reference's own
     taps (test_emul.reference_minphase_taps) as everywhere else in the suite;
  3. under emulation the forced half-array result is bitwise the full-array one (half_fused = 0)."""
import importlib
import os
import re

import numpy as np
import pytest

from cases import PEAK_TOL, RMS_TOL, make_input
import cases
from conftest import ROOT

r8b = importlib.import_module("r8brain-free-src_amd")

MAXIN = 4096
N_IN = 12000

# name, src, dst, transition band, attenuation, phase, the symbol of the first stage, its in_len, what the case exercises
# (FULL: the full-array kernel that stands behind each half-array form, r8b_convp_mode.h ConvpMode::full)
CASES = [
    ("up23", 44100.0, 96000.0, 2.0, 180.15, 0, "k_convp<11, 1, 23, 24>", 2680),      # 25-entry rows, even phase count
    ("down25", 48000.0, 44100.0, 2.0, 180.15, 0, "k_convp<11, 1, 25, 24>", 2554),    # 27-entry rows, 147 phases: idle lanes, odd pair count
    ("one33", 96000.0, 44100.0, 2.0, 180.15, 0, "k_convp<12, 0, 33, 24>", 2554),     # the 1:1 geometry
    ("minphase29", 44100.0, 96000.0, 2.0, 180.15, 1, "k_convp<11, 1, 29, 24>", 2680),  # shifted run: fl2r and t_zero non-trivial
    # another filter on the 2048 -> 4096-point geometry: in_len falls into element 8 of a thread's sixteen (2072 / 256),
    # where cfg2's falls into element 10 (2680 / 256) -- the element that straddles in_len moves
    ("narrow23", 44100.0, 96000.0, 1.4, 180.15, 0, "k_convp<11, 1, 23, 24>", 2072),
]
FULL = {"up23": "k_convp<11, 1, 4, 24>", "down25": "k_convp<11, 1, 5, 24>", "one33": "k_convp<12, 0, 5, 24>",
        "minphase29": "k_convp<11, 1, 16, 24>", "narrow23": "k_convp<11, 1, 4, 24>"}
_PARAMS = [(c, nch) for c in CASES for nch in (3, 4)]
_IDS = ["%s-%s-%dch" % (c[0], c[6].replace(" ", ""), nch) for c, nch in _PARAMS]


@pytest.fixture(scope="module")
def emul():
    return cases.emul_lib(test_hooks=True)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "no ROCm device"
    assert os.path.exists(r8b.lib_path()), "libr8bsrc_hip.so missing: no CPU fallback exists"
    return t


_INPUT = {}


def _input(nch):
    # (computed once per channel count and left unchanged)
    if nch not in _INPUT:
        _INPUT[nch] = make_input(nch, N_IN, 61)
        _INPUT[nch].setflags(write=False)
    return _INPUT[nch]


def _blocks_after(make, x, n):
    """convolver blocks a fresh object has computed (its counter conv_blocks) after ONE call of the stream's first n samples"""
    b = make(2)
    b.process_host(x[:, :n])
    return b.stat("conv_blocks")


def _cuts(make, x):
    """two cuts of N_IN samples into calls of at most MAXIN: whole calls; and a call that ends one sample short of a block
    boundary, a one-sample call behind it, whole calls for the rest.  The boundary is the object's own: where the launch puts
    its blocks follows from the fused form's blocking (stride, offset, the filter's delay), not from in_len alone, so it is
    found by asking -- the smallest first call that completes the last block a call of MAXIN completes (bisection over
    fresh objects; the count of completed blocks grows with the call's length).  Returns the cuts and that length."""
    a = [MAXIN] * (N_IN // MAXIN) + ([N_IN % MAXIN] if N_IN % MAXIN else [])
    top = _blocks_after(make, x, MAXIN)
    assert top >= 1, top
    lo, hi = 1, MAXIN          # blocks(lo) < top <= blocks(hi)
    assert _blocks_after(make, x, lo) < top
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _blocks_after(make, x, mid) >= top:
            hi = mid
        else:
            lo = mid
    b = [hi - 1, 1]
    while sum(b) < N_IN:
        b.append(min(MAXIN, N_IN - sum(b)))
    assert sum(a) == N_IN and sum(b) == N_IN and b[0] >= 1
    return a, b, hi


def _stream(b, x, lens):
    """the outputs, the per-call counts and the first stage's symbols seen (stage_symbols() names a stage's LATEST launch: a
    short call that completes no block launches the history copy alone)"""
    ys, pos, seen = [], 0, set()
    for l in lens:
        ys.append(b.process_host(x[:, pos:pos + l]))
        seen.add(b.stage_symbols()[0])
        pos += l
    return np.concatenate(ys, axis=1), [y.shape[1] for y in ys], seen


def check_diet_case(lib, lib_kw, refwrap, case, nch, full_array):
    """`lib`: the bound library that carries the parity-test hook (the minimum-phase case runs on the reference's taps)"""
    from test_emul import reference_minphase_taps
    name, src, dst, tb, att, phase, symbol, in_len = case

    def make(half_fused):
        b = r8b.BatchResampler(src, dst, MAXIN, tb, att, nch=nch, phase=phase, **lib_kw)
        b.set_option("walk", 0)
        b.set_option("half_fused", half_fused)
        b.set_option("timing", 1)
        return b

    def run():
        x = _input(nch)
        b = make(2)
        conv = [l for l in b.describe().splitlines() if l.startswith("BlockConvolver")][0]
        assert int(re.search(r"in_len=(\d+)", conv).group(1)) == in_len, conv
        cut_a, cut_b, boundary = _cuts(make, x)
        ya, counts, seen = _stream(b, x, cut_a)
        assert symbol in seen and all(not v.startswith("k_conv") or v == symbol for v in seen), seen
        assert ya.shape[0] == nch and ya.shape[1] > 0 and np.isfinite(ya).all()
        # 1. the cut into calls does not show
        # (the second cut: its first call stops one sample short of a block's completion, the one-sample call completes it)
        b2 = make(2)
        b2.process_host(x[:, :boundary - 1])
        short = b2.stat("conv_blocks")
        b2.process_host(x[:, boundary - 1:boundary])
        assert b2.stat("conv_blocks") > short and b2.stage_symbols()[0] == symbol, (boundary, short, b2.stage_symbols())
        b2 = make(2)
        yb, _, seen = _stream(b2, x, cut_b)
        assert symbol in seen and all(not v.startswith("k_conv") or v == symbol for v in seen), seen
        assert ya.shape == yb.shape and np.array_equal(ya, yb), (name, nch, np.argwhere(ya != yb)[:4].tolist())
        # 2. every channel against the compiled reference, at the project's bound (full-scale noise: level 1)
        r, p = refwrap.batch_check(src, dst, MAXIN, cut_a, x, ya, counts, tb, att, phase=phase)
        print("convp diet: %s %s %d ch rms %.3g peak %.3g" % (name, symbol, nch, r.max(), p.max()))
        assert r.max() <= RMS_TOL and p.max() <= PEAK_TOL, (name, nch, r.tolist(), p.tolist())
        # 3. emulation: the half-array form is bitwise the full-array one
        if full_array:
            f = make(0)
            yf, _, seen = _stream(f, x, cut_a)
            assert FULL[name] in seen and all(not v.startswith("k_conv") or v == FULL[name] for v in seen), seen
            assert yf.shape == ya.shape and np.array_equal(yf, ya), (name, nch, np.argwhere(yf != ya)[:4].tolist())

    if phase:
        with reference_minphase_taps(lib, refwrap) as prov:
            run()
            assert prov.calls, "the provider was not consulted"
    else:
        run()


@pytest.mark.parametrize("case,nch", _PARAMS, ids=_IDS)
def test_emulated_convp_diet(emul, refwrap, case, nch):
    check_diet_case(emul, {"lib": emul}, refwrap, case, nch, full_array=True)


@pytest.mark.gpu
@pytest.mark.parametrize("case,nch", _PARAMS, ids=_IDS)
def test_hip_convp_diet(torch, refwrap, request, case, nch):
    """the same on the device; the minimum-phase case on the test build of the library (conftest.hip_hooks: the same device
    objects with the parity-test hook), every other one on the product library"""
    if case[5]:
        hooks = request.getfixturevalue("hip_hooks")
        check_diet_case(hooks, {"device": 0, "lib": hooks}, refwrap, case, nch, full_array=False)
    else:
        check_diet_case(None, {"device": 0}, refwrap, case, nch, full_array=False)
