"""Inf / NaN samples stay in their own channel of a pair (include/r8bsrc.h; r8b_convp.h cp_level_shift): the emulation
tier (CPU, tests/emul) and the GPU tier (-m gpu: the HIP library on the device) over every pair-kernel form
(tests/nonfinite_cases.py), and a full-size cfg2 batch on the GPU."""
import importlib
import os

import numpy as np
import pytest

import cases
from conftest import ROOT
from nonfinite_cases import NCH, NONFINITE_CASES, NONFINITE_MINPHASE_CASES, check_nonfinite

r8b = importlib.import_module("r8brain-free-src_amd")


@pytest.fixture(scope="module")
def emul():
    return cases.emul_lib(test_hooks=True)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "no ROCm device"
    assert os.path.exists(r8b.lib_path()), "libr8bsrc_hip.so missing: no CPU fallback exists"
    return t


def _maker(case, lib_kw, half, pair_conv, phase=0):
    src, dst, maxin, chunk, n, tb, att = case[:7]
    opts = dict(case[7]) if len(case) > 7 else {}

    def make():
        b = r8b.BatchResampler(src, dst, maxin, tb, att, nch=NCH, phase=phase, **lib_kw)
        b.set_option("half", half)
        b.set_option("pair_conv", pair_conv)
        for k, v in opts.items():
            b.set_option(k, v)
        return b
    return make


def _ids(cases):
    return ["%g-%g-%d%s" % (c[0], c[1], c[2], "-" + "-".join("%s%d" % kv for kv in c[7].items()) if len(c) > 7 else "")
            for c in cases]


@pytest.mark.parametrize("pair_conv", [1, 0])
@pytest.mark.parametrize("half", [0, 2])
@pytest.mark.parametrize("case", NONFINITE_CASES, ids=_ids(NONFINITE_CASES))
def test_emulated_nonfinite_stays_in_its_channel(emul, case, half, pair_conv):
    check_nonfinite(_maker(case, {"lib": emul}, half, pair_conv), case)


@pytest.mark.parametrize("half", [0, 2])
@pytest.mark.parametrize("case", NONFINITE_MINPHASE_CASES, ids=_ids(NONFINITE_MINPHASE_CASES))
def test_emulated_nonfinite_minimum_phase(emul, case, half):
    check_nonfinite(_maker(case, {"lib": emul}, half, 1, phase=1), case, phase=1)


@pytest.mark.gpu
@pytest.mark.parametrize("pair_conv", [1, 0])
@pytest.mark.parametrize("half", [0, 2])
@pytest.mark.parametrize("case", NONFINITE_CASES, ids=_ids(NONFINITE_CASES))
def test_hip_nonfinite_stays_in_its_channel(torch, case, half, pair_conv):
    check_nonfinite(_maker(case, {"device": 0}, half, pair_conv), case)


@pytest.mark.gpu
@pytest.mark.parametrize("half", [0, 2])
@pytest.mark.parametrize("case", NONFINITE_MINPHASE_CASES, ids=_ids(NONFINITE_MINPHASE_CASES))
def test_hip_nonfinite_minimum_phase(torch, case, half):
    check_nonfinite(_maker(case, {"device": 0}, half, 1, phase=1), case, phase=1)


@pytest.mark.gpu
def test_hip_nonfinite_full_size_cfg2(torch):
    """cfg2 at full size (1024 channels x 16384 samples per call, 44100 -> 96000): a handful of channels spread over the
    batch carry NaN / Inf; every other channel is bitwise what it is when those channels are zeros instead"""
    nch, L, calls = 1024, 16384, 3
    g = torch.Generator(device="cuda:0")
    g.manual_seed(5)
    x = torch.rand((nch, L * calls), dtype=torch.float64, device="cuda:0", generator=g) * 2.0 - 1.0
    faulty = [0, 1, 37, 510, 511, 777, 1022]
    x[faulty] = 0.0          # (zero apart from their non-finite samples: their partners' level shift stays as beside zeros)
    xz = x.clone()
    x[0, 20000] = float("nan")
    x[1, 30000] = float("inf")                      # (0 and 1: both channels of one pair)
    x[37, 9000:20000] = float("nan")                # (a run longer than a block)
    x[510, L - 1] = -float("inf")
    x[511, L] = float("nan")
    x[777, 2 * L + 100] = float("nan")
    x[1022, 40000] = float("nan")

    def run(inp):
        b = r8b.BatchResampler(44100.0, 96000.0, L, 2.0, 180.15, nch=nch, device=0)
        return torch.cat([b.process(inp[:, i * L:(i + 1) * L].contiguous()).clone() for i in range(calls)], dim=1)

    y, yz = run(x), run(xz)
    assert y.shape == yz.shape and y.shape[1] > 0
    ok = torch.ones(nch, dtype=torch.bool, device="cuda:0")
    ok[faulty] = False
    fin = torch.isfinite(y)
    assert bool(fin[ok].all())
    assert torch.equal(y[ok].view(torch.int64), yz[ok].view(torch.int64))
    for c in faulty:
        assert not bool(fin[c].all()), c
        assert bool(fin[c, :1000].all()), c          # (ahead of the first non-finite sample: untouched)
