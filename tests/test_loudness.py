"""The BS.1770 K-weighted loudness meter of the PCM egress (include/r8bsrc.h "loudness"; tests/loudness_cases.py states what
each check asserts): every check on the host emulation, which runs the kernel's own body (csrc/r8b_loudness.h), and on the
device (-m gpu).  Equality with the exact-arithmetic oracle, and between two runs of the meter, is bitwise.

  design                            1. coefficients, hand-off matrix, sub-block, the refusal below 8000 Hz
  spec                              2. the specification on Src == Dst and on a chain
  cuts                              3. one call against the stream cut around segment, sub-block and tile edges
  lone_sample                       4. one sample at a tile's first and last lanes and across its edge
  nonfinite                         5. NaN and Inf enter as zeros
  clips_pass / clips_chain          6. the five clip entries, zero fill, the caller's order, empty state per call
  lifecycle                         7. read before enable, capacity, drain, clear(), disable, state_load, mid-stream
  inert                             8. bytes, meters, true peak, symbols and counters with the meter on, off, never enabled
  side_by_side                      8b. the three meters on one object through a stream's life, each against its alone-run
  gating / ebu_*                    9. r8b_loudness_integrated against numpy; EBU Tech 3341's synthetic signals
  test_build_links_the_kernel       10. the product library holds k_loudness and its launcher's strong definition
  test_loudness_under_the_address_sanitizer   11. tests/cxx_loudness.cpp (slow)"""
import importlib
import os
import subprocess

import pytest

import cases
import loudness_cases as LD
from conftest import ROOT

r8b = importlib.import_module("r8brain-free-src_amd")

CHECKS = [LD.check_design, LD.check_spec, LD.check_cuts, LD.check_lone_sample, LD.check_nonfinite, LD.check_clips_pass,
          LD.check_clips_chain, LD.check_lifecycle, LD.check_inert, LD.check_side_by_side, LD.check_gating] + LD.EBU_CHECKS
_IDS = [f.__name__[len("check_"):] for f in CHECKS]


@pytest.fixture(scope="module")
def emul():
    return LD.Tier(cases.emul_lib())


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "no ROCm device"
    assert os.path.exists(r8b.lib_path()), "libr8bsrc_hip.so missing: no CPU fallback exists"
    return LD.Tier(None)


@pytest.mark.parametrize("check", CHECKS, ids=_IDS)
def test_loudness_emulated(emul, check):
    check(emul)


@pytest.mark.gpu
@pytest.mark.parametrize("check", CHECKS, ids=_IDS)
def test_loudness_gpu(gpu, check):
    check(gpu)


def test_build_links_the_kernel():
    """the weak host form of launch_loudness (r8b_capi.cpp) gives way to the device launcher in the product library, and
    the emulation, which has no other, keeps it"""
    if not os.path.exists(r8b.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    cases.emul_lib()

    def symbols(path):
        out = subprocess.run(["nm", "-C", path], check=True, stdout=subprocess.PIPE, text=True).stdout
        return [line.split(None, 2) for line in out.splitlines() if "loudness" in line]
    prod = symbols(r8b.lib_path())
    assert any("__device_stub__k_loudness" in s[-1] for s in prod), prod
    assert len([s for s in prod if s[-1].startswith("r8bhip::launch_loudness(")]) == 1, prod
    emul = symbols(os.path.join(ROOT, "tests", "emul", "_build", "libr8bsrc_emul.so"))
    assert len([s for s in emul if s[-1].startswith("r8bhip::launch_loudness(")]) == 1, emul
    assert not any("k_loudness" in s[-1] for s in emul)


@pytest.mark.slow
def test_loudness_under_the_address_sanitizer(tmp_path):
    """tests/cxx_loudness.cpp: the emulation's sources and a stand-alone driver as ONE program built with
    -fsanitize=address,undefined (no library, nothing preloaded; minutes of compilation): streams cut at the lengths of
    check 3 and the clip lengths of check 6 through the C ABI, every buffer a heap block sized to the byte, the sums against
    the driver's own restatement.  The sanitized objects of the emulation's sources are those of tests/emul/Makefile
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
    exe = str(tmp_path / "cxx_loudness")
    out = subprocess.run([os.environ.get("CXX", "g++")] + flags + [os.path.join(ROOT, "tests", "cxx_loudness.cpp")] +
                         [os.path.join(emul, o) for o in objs] + ["-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True)
    assert out.returncode == 0, out.stdout[-3000:]
    run = subprocess.run([exe, str(LD.TILE)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "runtime error" not in run.stdout and "AddressSanitizer" not in run.stdout and \
        run.stdout.strip().endswith("OK"), run.stdout[-3000:]
