"""The 4x-oversampled true-peak meter of the PCM egress (include/r8bsrc.h "true peak"; tests/true_peak_cases.py states what
each check asserts): every check on the host emulation, which runs the kernel's own body (csrc/r8b_truepeak.h), and on
the device (-m gpu).  Equality with the exact-arithmetic oracle is bitwise.

  spec_pass / spec_chain / phases   1. the specification, 2. chunk invariance
  lone_sample                       3. one sample at every lane and wave of a tile and across its edge
  nonfinite                         4. NaN skipped, Inf passes, Inf - Inf skipped
  clips_pass / _tile_edge / _chain  5. the five clip entries, the tail, the caller's order, zero history per call
  lifecycle / shards                6. read before enable, reset, clear(), disable, state_load, shards
  inert                             7. bytes, meters, symbols and counters with the meter on, off, never enabled
  test_build_links_the_kernel       the product library holds k_truepeak and its launcher's strong definition
  test_golden_taps_are_the_header   tests/golden/true_peak_taps.json and the literals of csrc/r8b_truepeak.h: the same bits
  test_true_peak_under_the_address_sanitizer   8. tests/cxx_true_peak.cpp (slow)"""
import importlib
import json
import os
import re
import subprocess

import pytest

import cases
import true_peak_cases as TP
from conftest import ROOT

r8b = importlib.import_module("r8brain-free-src_amd")

CHECKS = [TP.check_spec_pass, TP.check_spec_chain, TP.check_phases, TP.check_lone_sample, TP.check_nonfinite,
          TP.check_clips_pass, TP.check_clips_tile_edge, TP.check_clips_chain, TP.check_lifecycle, TP.check_shards,
          TP.check_inert]
_IDS = [f.__name__[len("check_"):] for f in CHECKS]


@pytest.fixture(scope="module")
def emul():
    return TP.Tier(cases.emul_lib())


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "no ROCm device"
    assert os.path.exists(r8b.lib_path()), "libr8bsrc_hip.so missing: no CPU fallback exists"
    return TP.Tier(None)


@pytest.mark.parametrize("check", CHECKS, ids=_IDS)
def test_true_peak_emulated(emul, check):
    check(emul)


@pytest.mark.gpu
@pytest.mark.parametrize("check", CHECKS, ids=_IDS)
def test_true_peak_gpu(gpu, check):
    check(gpu)


def test_golden_taps_are_the_header():
    text = open(os.path.join(ROOT, "r8brain-free-src_amd", "csrc", "r8b_truepeak.h")).read()
    block = re.search(r"#define R8B_TP_TAPS (.*?)\n// END GENERATED", text, re.S).group(1)
    lits = re.findall(r"-?0x1\.[0-9a-f]+p[+-]?\d+", block)
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "true_peak_taps.json")))["g"]
    assert [float.fromhex(v) for v in lits] == [float.fromhex(v) for row in gold for v in row] and len(lits) == 36
    g = [[float.fromhex(v) for v in row] for row in gold]
    # exactly symmetric, every tap non-zero, the smallest 2.6e-4 (include/r8bsrc.h)
    assert g[0] == g[2][::-1] and g[1] == g[1][::-1]
    assert 2.5e-4 < min(abs(v) for row in g for v in row) < 2.7e-4
    # a Nyquist filter's phases: unit gain at DC to the window's accuracy
    assert all(abs(sum(row) - 1.0) < 1e-4 for row in g)


def test_build_links_the_kernel():
    """the weak host form of launch_true_peak (r8b_capi.cpp) gives way to the device launcher in the product library,
    and the emulation, which has no other, keeps it"""
    if not os.path.exists(r8b.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    cases.emul_lib()

    def symbols(path):
        out = subprocess.run(["nm", "-C", path], check=True, stdout=subprocess.PIPE, text=True).stdout
        return [line.split(None, 2) for line in out.splitlines() if "true_peak" in line or "k_truepeak" in line]
    prod = symbols(r8b.lib_path())
    assert any("__device_stub__k_truepeak" in s[-1] for s in prod), prod
    # (one definition survives the link -- the strong one; that it is the device's shows on the GPU tier, where the host
    # form would read device pointers)
    assert len([s for s in prod if s[-1].startswith("r8bhip::launch_true_peak(")]) == 1, prod
    emul = symbols(os.path.join(ROOT, "tests", "emul", "_build", "libr8bsrc_emul.so"))
    assert len([s for s in emul if s[-1].startswith("r8bhip::launch_true_peak(")]) == 1, emul
    assert not any("k_truepeak" in s[-1] for s in emul)


@pytest.mark.slow
def test_true_peak_under_the_address_sanitizer(tmp_path):
    """tests/cxx_true_peak.cpp: the emulation's sources and a stand-alone driver as ONE program built with
    -fsanitize=address,undefined (no library, nothing preloaded; minutes of compilation): streams cut at the lengths of
    check 1 and the clip lengths of check 5 through the C ABI, every buffer a heap block sized to the byte, the values
    against the driver's own fma chain.  The sanitized objects of the emulation's sources are those of tests/emul/Makefile
    (`asan`: shared with the other sanitizer runs); the driver is compiled and the program linked here, with the same
    flags.  Host code only."""
    emul = os.path.join(ROOT, "tests", "emul")
    names = ["r8b_design", "r8b_plan", "r8b_engine", "r8b_capi", "emul_launch", "emul_pcm"]
    objs = [os.path.join("_build", "asan", n + ".o") for n in names]
    out = subprocess.run(["make", "-j8"] + objs, cwd=emul, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout[-3000:]
    flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize=shift",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas", "-DR8B_TEST_HOOKS",
             "-I" + os.path.join(ROOT, "r8brain-free-src_amd", "csrc")]
    exe = str(tmp_path / "cxx_true_peak")
    out = subprocess.run([os.environ.get("CXX", "g++")] + flags + [os.path.join(ROOT, "tests", "cxx_true_peak.cpp")] +
                         [os.path.join(emul, o) for o in objs] + ["-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True)
    assert out.returncode == 0, out.stdout[-3000:]
    run = subprocess.run([exe, str(TP.TF), os.path.join(ROOT, "tests", "golden", "true_peak_taps.json")], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "runtime error" not in run.stdout and "AddressSanitizer" not in run.stdout and \
        run.stdout.strip().endswith("OK"), run.stdout[-3000:]
