"""Every compiled instance of the compile-time-sized convolver kernels, by name, against the reference (tests/kernel_census.py).

The fast path is two templates compiled 267 times (k_convp<LN, UL, MODE, FLENP>, its walk form, k_convq,
k_convx<LOGN, UPLOG, MODE, FLENP>); the other modules pick their cases by ratio, so which instances they run depends on
what Engine::resolve_forms() and r8b_dispatch.h resolve a ratio to today.  Here the table has one entry per instance:

  test_census_names_exactly_the_build   the instances in the product library (host stubs, `nm -C`) and in the emulator's
                                        dispatch equal the table's symbols, both ways, and hold none of the 57 that no
                                        chain launches (kernel_census.NOT_BUILT)
  test_census_instance_emulated[symbol] one id per reachable instance on the host emulation (the real kernel bodies)
  test_census_instance_gpu[symbol]      the same on the device (-m gpu)
  test_census_under_the_address_sanitizer  tests/cxx_kernel_census.cpp: every reachable chain as a stand-alone host program
                                        under AddressSanitizer and UndefinedBehaviorSanitizer (slow)

kernel_census.check_instance() states what an id asserts."""
import importlib
import os
import subprocess

import pytest

import cases
import kernel_census as K
from conftest import ROOT

r8b = importlib.import_module("r8brain-free-src_amd")


def _tool():
    """tools/kernel_census.py (the case module has the same name: loaded by file)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_census_tool", os.path.join(ROOT, "tools", "kernel_census.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def emul():
    return cases.emul_lib(test_hooks=True)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "no ROCm device"
    assert os.path.exists(r8b.lib_path()), "libr8bsrc_hip.so missing: no CPU fallback exists"
    return t


@pytest.fixture(scope="module")
def lib():
    # (as tests/test_abi_and_design.py gets the product library)
    if not os.path.exists(r8b.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return r8b.load()


def _reference():
    import refwrap as R
    return R if R.available() else None


def test_census_names_exactly_the_build(lib, emul):
    tool = _tool()
    table = set(K.SYMBOLS)
    not_built = set(e["symbol"] for e in K.NOT_BUILT)
    assert len(not_built) == len(K.NOT_BUILT) == 57
    assert not_built & set(e["symbol"] for e in K.RUNS) == set()
    for what, path in (("product library", r8b.lib_path()),
                       ("emulator", os.path.join(ROOT, "tests", "emul", "_build", "libr8bsrc_emul.so"))):
        built = set(tool.list_instances(path))
        assert len(built) == len(K.SYMBOLS) == 267, (what, len(built))
        assert built - table == set(), "%s: instances without a census entry: %s" % (what, sorted(built - table))
        assert table - built == set(), "%s: census entries for instances that are gone: %s" % (what, sorted(table - built))
        assert built & not_built == set(), "%s: instances that no chain launches are back: %s" % (what, sorted(built & not_built))
    for e in K.NOT_BUILT:
        assert e["reason"] and e["cite"], e
    for e in K.RUNS:
        # an entry with options names an opt-in form; the pins are not options of the entry
        assert set(e["opt_in"]) <= {"walk", "walk_len", "quad", "half", "half_fused", "pair_two", "pair_conv", "pair_solo",
                                    "pair_split", "fuse", "fuse_hbconv", "fuse_hbd", "fuse_latency", "up3_poly"}, e


def _maker(e, lib_kw):
    def make():
        b = r8b.BatchResampler(e["src"], e["dst"], e["maxin"], e["tb"], e["att"], nch=K.NCH, phase=e["phase"], **lib_kw)
        for k, v in e["opts"].items():
            b.set_option(k, v)
        b.set_option("timing", 1)
        return b
    return make


def _check(e, tier, lib_kw, hooks):
    from test_emul import reference_minphase_taps
    ref = _reference()
    if e["phase"] and ref is not None:
        with reference_minphase_taps(hooks, ref) as prov:
            worst = K.check_instance(_maker(e, lib_kw), tier, e, ref, prov)
            assert prov.calls, "the provider was not consulted"
    else:
        worst = K.check_instance(_maker(e, lib_kw), tier, e, ref)
    print("census: %s worst own-level rms %s peak %s (over tol_scale)" % ((e["symbol"],) + (worst or ("-", "-"))))


_IDS = [e["symbol"].replace(" ", "") for e in K.RUNS]


@pytest.mark.parametrize("e", K.RUNS, ids=_IDS)
def test_census_instance_emulated(emul, e):
    _check(e, K.HostTier(), {"lib": emul}, emul)


@pytest.mark.gpu
@pytest.mark.parametrize("e", K.RUNS, ids=_IDS)
def test_census_instance_gpu(torch, request, e):
    """minimum-phase entries on the test build of the library (conftest.hip_hooks: the same device objects with the
    parity-test hook), every other one on the product library"""
    if e["phase"] and _reference() is not None:
        hooks = request.getfixturevalue("hip_hooks")
        _check(e, K.DeviceTier(torch), {"device": 0, "lib": hooks}, hooks)
    else:
        _check(e, K.DeviceTier(torch), {"device": 0}, None)


@pytest.mark.slow
def test_census_under_the_address_sanitizer(tmp_path):
    """tests/cxx_kernel_census.cpp: the emulation's sources and a stand-alone driver as one program built with
    -fsanitize=address,undefined (tests/emul/Makefile `census`, minutes of compilation); every reachable chain of the
    census, two calls of noise and two short ones, the symbol that ran checked.  Host code only."""
    table = tmp_path / "census_table.txt"
    with open(table, "w") as f:
        K.dump(f)
    d = os.path.join(ROOT, "tests", "emul")
    out = subprocess.run(["make", "-j8", "census", "TABLE=%s" % table], cwd=d, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and "runtime error" not in out.stdout and "AddressSanitizer" not in out.stdout and \
        out.stdout.strip().endswith("OK"), out.stdout[-3000:]
    assert "%d instances, 0 failed" % len(K.RUNS) in out.stdout
