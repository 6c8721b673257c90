"""Every kernel of the PCM boundary by name (tests/pcm_boundary_cases.py): the 8 ingest and 40 egress kernels that
r8b_pcm_dispatch.h starts for r8b_batch_process_pcm and the r8b_batch_resample_clips entries.

  test_census_names_exactly_the_build   the boundary's host stubs in the product library and the names the emulator's
                                        backend notes (`nm -C`) equal the table's 48, both ways
  test_boundary_form_emulated[symbol]   one id per symbol on the host emulation: the form in all eight sample formats,
                                        alone (Src == Dst) and behind 44100 -> 88200 -- the symbols of both sides, every
                                        output byte against the numpy oracle, the sentinels around and between the
                                        buffers, the meters
  test_boundary_form_gpu[symbol]        the same on the device (-m gpu)
  test_meter_lanes_emulated / _gpu[symbol]  the 20 metering kernels: a lone event per channel on every lane and wave of
                                        the workgroup that converts it, then a whole chunk or tile of events
  test_boundary_refusals_emulated / _gpu  what the C ABI refuses in front of the launcher's own checks
  test_symbols_of_a_side_without_a_launch  "" before the first call, after a call without samples, and for a planar
                                        side that a stage converts itself

pcm_boundary_cases.check_plain / check_clip state what an id asserts."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import pcm_boundary_cases as B
from conftest import ROOT

r8b = importlib.import_module("r8brain-free-src_amd")


@pytest.fixture(scope="module")
def emul():
    return B.Tier(cases.emul_lib())


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "no ROCm device"
    assert os.path.exists(r8b.lib_path()), "libr8bsrc_hip.so missing: no CPU fallback exists"
    return B.Tier(None)


@pytest.fixture(scope="module")
def lib():
    # (as tests/test_abi_and_design.py gets the product library)
    if not os.path.exists(r8b.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return r8b.load()


# ---------------------------------------------------------------- a. the names
def built_names(path):
    """the boundary's symbols in a built library: the device library's host stubs (__device_stub__k_pcm_finish<true,
    false>), or the emulation's per-instance name strings (EmulPcm::pcm_finish<true, false>(...)::sym)"""
    out = subprocess.run(["nm", "-C", path], check=True, stdout=subprocess.PIPE, text=True).stdout
    found = set()
    for line in out.splitlines():
        m = re.search(r"__device_stub__(k_(?:pcm|clip)\w*)(?:<([\w, ]+)>)?\(", line)
        if m:
            args = [a.strip() for a in m.group(2).split(",")] if m.group(2) else []
            found.add(m.group(1) + ("<%s>" % ", ".join(args) if args else ""))
            continue
        m = re.search(r"\bEmulPcm::(\w+?)(?:<([\w:, ]+)>)?\(.*\)::sym\b", line)
        if m and " guard variable " not in line:
            found.add(B.emul_name(m.group(1), [a.strip() for a in m.group(2).split(",")] if m.group(2) else []))
    return found


def test_census_names_exactly_the_build(lib):
    cases.emul_lib()
    table = set(B.SYMBOLS)
    assert len(table) == 48 and B.NOT_REACHED == []
    for what, path in (("product library", r8b.lib_path()),
                       ("emulator", os.path.join(ROOT, "tests", "emul", "_build", "libr8bsrc_emul.so"))):
        built = built_names(path)
        assert built - table == set(), "%s: boundary kernels without a census entry: %s" % (what, sorted(built - table))
        assert table - built == set(), "%s: census entries for kernels that are gone: %s" % (what, sorted(table - built))
    # the bool arguments' spelling, as the demangler prints it, is the one the launcher notes
    assert "k_clip_sched_frames_out<false, true, true>" in table
    text = open(os.path.join(ROOT, "include", "r8bsrc.h")).read()
    assert "R8B_STAGE_PCM_IN = -1, R8B_STAGE_PCM_OUT = -2" in text
    assert (r8b.STAGE_PCM_IN, r8b.STAGE_PCM_OUT) == (-1, -2)


# ---------------------------------------------------------------- b. one id per symbol and tier
_IDS = [s.replace(" ", "") for s in B.SYMBOLS]


@pytest.mark.parametrize("form", B.FORMS, ids=_IDS)
def test_boundary_form_emulated(emul, form):
    B.check_form(emul, form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", B.FORMS, ids=_IDS)
def test_boundary_form_gpu(gpu, form):
    B.check_form(gpu, form)


# ---------------------------------------------------------------- c. the lone event
_METER_IDS = [f["symbol"].replace(" ", "") for f in B.METERED]


@pytest.mark.parametrize("form", B.METERED, ids=_METER_IDS)
def test_meter_lanes_emulated(emul, form):
    B.check_meter_lanes(emul, form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", B.METERED, ids=_METER_IDS)
def test_meter_lanes_gpu(gpu, form):
    B.check_meter_lanes(gpu, form)


# ---------------------------------------------------------------- d. refusals
def test_boundary_refusals_emulated(emul):
    B.check_refusals(emul)


@pytest.mark.gpu
def test_boundary_refusals_gpu(gpu):
    B.check_refusals(gpu)


# ---------------------------------------------------------------- the pseudo-stages themselves
def check_no_launch(tier):
    a = tier.make(2, 44100.0, 88200.0, 1024, att=B.ATT)
    assert a.boundary_symbols() == ("", "")
    x = tier.buf(np.zeros((2, 1024)))
    out = tier.buf(np.zeros((2, max(a.max_out_len, 1))))
    args = (tier.ptr(x), B.F64, False, 1024, 1024, tier.ptr(out), B.S16, True, 2)
    # without "timing" nothing is kept (two calls: the first ones end inside the chain's latency)
    assert a.process_pcm_ptr(*args) >= 0 and a.process_pcm_ptr(*args) > 0
    assert a.boundary_symbols() == ("", "")
    a.set_option("timing", 1)
    assert a.process_pcm_ptr(*args) > 0
    # (the planar fp64 input is the first stage's own: no ingest launch)
    assert a.boundary_symbols() == ("", "k_pcm_out")
    assert a.process_pcm_ptr(tier.ptr(x), B.F64, False, 1024, 0, tier.ptr(out), B.S16, True, 2) == 0
    assert a.boundary_symbols() == ("", "")
    # a stage number below the pseudo-stages is still refused
    buf = ctypes.create_string_buffer(96)
    assert a._lib.r8b_batch_stage_symbol(a._h, -3, buf, 96) == -1


def test_symbols_of_a_side_without_a_launch_emulated(emul):
    check_no_launch(emul)


@pytest.mark.gpu
def test_symbols_of_a_side_without_a_launch_gpu(gpu):
    check_no_launch(gpu)


# ---------------------------------------------------------------- under the sanitizers
@pytest.mark.slow
def test_boundary_under_the_address_sanitizer():
    """tests/cxx_pcm_boundary.cpp: the emulation's sources and a stand-alone driver as one program built with
    -fsanitize=address,undefined (tests/emul/Makefile `boundary`, minutes of compilation); each of the 48 forms in each of
    the eight formats through the launcher, every buffer sized to the byte.  Host code only."""
    d = os.path.join(ROOT, "tests", "emul")
    out = subprocess.run(["make", "-j8", "boundary"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and "runtime error" not in out.stdout and "AddressSanitizer" not in out.stdout and \
        out.stdout.strip().endswith("OK"), out.stdout[-3000:]
    assert "%d forms, 0 failed" % len(B.FORMS) in out.stdout
