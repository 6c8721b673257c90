"""Every kernel of the PCM twin -- the second build of r8b_kernels.hip, whose loads and stores decode and encode planar
S16 / S24 / S32 / F32 caller buffers in place -- by name, with every format on either side (tests/pcm_twin_cases.py).

The other modules reach the twin with S16 in and S24 out on seven default chains; the census modules run fp64 rows only.
Here every kernel of the twin's launcher list has entries of its own, one id per tier:

  test_pcm_twin_emulated / _gpu[id]       one entry with its six format pairs: the twin ran, its bytes are the encoded fp64
                                          path's, every byte outside the rows is untouched, the codes are the oracle's,
                                          another cut into calls gives the same bytes; formats that change from call to call
                                          and a checkpoint after a PCM call on one entry per kernel (pcm_twin_cases.check_entry)
  test_codec_edges_emulated / _gpu[id]    the in-kernel codec at its edges through the half-band up-sampler's copied
                                          samples, 1 and 14 taps: all 65536 S16 codes, the S24 / S32 / F32 edge codes, ties,
                                          saturation, denormals and overflow on the way out (check_codec_edges)
  test_twin_census_is_complete            the written-out kernel names against the launchers of r8b_kernels.hip
  test_twin_under_the_address_sanitizer   tests/cxx_pcm_twin.cpp: one stage per kernel with buffers sized to the byte, as a
                                          stand-alone host program under AddressSanitizer (slow)

Left out, with the reason: the codec edges through k_hbcascade.  A cascade exists only behind a chain's convolver
(r8b_batch_create_stage makes single stages), so no caller-chosen value reaches its copied samples; its loads never
decode, and what it encodes is held to the fp64 path byte for byte by its entries."""
import importlib
import os
import subprocess

import pytest

import cases
import pcm_twin_cases as T
import stage_census as S
from conftest import ROOT

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


def _reference():
    import refwrap as R
    return R if R.available() else None


_IDS = [e["id"] for e in T.ENTRIES]
_EDGES = [e for e in T.ENTRIES if e["id"] in ("k_hbup-t1", "k_hbup-t14")]


def _run(e, tier, lib_kw):
    tally = T.check_entry(r8b, tier, e, lib_kw, _reference())
    print("pcm twin census: %s (%s): %s" % (e["id"], "gpu" if tier.gpu else "emulated", tally))


@pytest.mark.parametrize("e", T.ENTRIES, ids=_IDS)
def test_pcm_twin_emulated(emul, e):
    """pcm_twin_cases.check_entry"""
    _run(e, S.HostTier(), {"lib": emul})


@pytest.mark.gpu
@pytest.mark.parametrize("e", T.ENTRIES, ids=_IDS)
def test_pcm_twin_gpu(torch, e):
    """pcm_twin_cases.check_entry"""
    _run(e, S.DeviceTier(torch), {"device": 0})


@pytest.mark.parametrize("e", _EDGES, ids=[e["id"] for e in _EDGES])
def test_codec_edges_emulated(emul, e):
    """pcm_twin_cases.check_codec_edges"""
    T.check_codec_edges(r8b, S.HostTier(), e, {"lib": emul})


@pytest.mark.gpu
@pytest.mark.parametrize("e", _EDGES, ids=[e["id"] for e in _EDGES])
def test_codec_edges_gpu(torch, e):
    """pcm_twin_cases.check_codec_edges: the first device run of the in-kernel codec at its edges -- a flushed F32
    denormal or a truncating conversion fails here"""
    T.check_codec_edges(r8b, S.DeviceTier(torch), e, {"device": 0})


def test_twin_census_is_complete():
    """the case module checks its lists when it is imported (pcm_twin_cases._complete): the kernel names written out there
    are the launch_symbol_note() names of the R8B_LAUNCH launchers of r8b_kernels.hip, ten of them, and every one but k_tail
    has entries; every entry runs the six pairs; one entry per kernel alternates its formats; the sanitizer program's table
    names every kernel"""
    T._complete()
    assert len(T.twin_launcher_symbols()) == 10 and len(_EDGES) == 2
    assert len(T.PAIRS) == 6 and len(T.ALTERNATING) == 9 and len(T.DUMPED + T.DUMPED_CHAINS) == 9
    assert all(e["level"] > 0 and e["kernel"] in (e["first"], e["last"]) for e in T.ENTRIES)


@pytest.mark.slow
def test_twin_under_the_address_sanitizer(tmp_path):
    """tests/cxx_pcm_twin.cpp: the emulation's sources and a stand-alone driver as one program built with
    -fsanitize=address,undefined (tests/emul/Makefile `pcm`, minutes of compilation): one stage per kernel, S24 -> S16 and
    F32 -> S24, every caller buffer a heap block of exactly the bytes its rows take -- a three-byte row read or written one
    byte past its end, which no device run can see, shows here.  Host code only."""
    table = tmp_path / "pcm_table.txt"
    with open(table, "w") as f:
        T.dump(f)
    d = os.path.join(ROOT, "tests", "emul")
    out = subprocess.run(["make", "-j8", "pcm", "PCM_TABLE=%s" % table], cwd=d, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and "runtime error" not in out.stdout and "AddressSanitizer" not in out.stdout and \
        out.stdout.strip().endswith("OK"), out.stdout[-3000:]
    assert "%d entries, 0 failed" % len(T.DUMPED + T.DUMPED_CHAINS) in out.stdout
