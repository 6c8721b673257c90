"""Every row of the tables behind the table-driven stage kernels, by name, against the plain formulas and the reference
(tests/stage_census.py).

k_hbup, k_hbdown, k_hbcascade, k_hbdcascade, k_whole, k_poly and k_poly_tiled pick their filters at run time: 67 half-band
rows of 1 ... 14 taps, cascades of up to eight stages, 22 interpolator banks.  The other modules pick their cases by ratio
and reach the rows their ratios select; here every row, depth and bank has an id of its own, one per tier:

  test_hb_row_emulated / _gpu[id]         part A: every half-band row as a stand-alone up-sampler and decimator
  test_hb_columns_emulated / _gpu[id]     ... the store forms of hbup_compute, a row per tap count 1 / 4 / 5 / 8 / 9 / 14
  test_up_chain_emulated / _gpu[id]       part B: 44100 -> 44100 * 2^k, k = 3 ... 11 (cascade runs of 2 ... 8, 8 + 1, 8 + 2)
                                          and 48000 -> 48000 * 3 * 2^k at four (two) attenuations, two tile sizes
  test_chain_columns_emulated / _gpu[id]  ... the store forms of the cascade's last stage
  test_down_chain_emulated / _gpu[id]     the same ratios downwards through k_hbdcascade, two spans
  test_bank_emulated / _gpu[id]           part C: every bank length of both families at five ratios, on k_whole,
                                          k_poly_tiled (both fetch forms) and k_poly
  test_stages_under_the_address_sanitizer tests/cxx_stage_census.cpp: the chains of part B and a row of part A per tap
                                          count as a stand-alone host program under AddressSanitizer and
                                          UndefinedBehaviorSanitizer (slow)

stage_census.check_hb_row / check_up_chain / check_down_chain / check_bank state what an id asserts -- and the one stated
exception: output index 1 of the nine one-tap up-samplers against the reference, whose ring reads an element it never
wrote (check_hb_row).  Where oracle/_ref was not built the plain-formula half of an id still runs."""
import importlib
import os
import subprocess

import pytest

import cases
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


def _stage_maker(maxin, lib_kw):
    def make(desc, opts=None):
        b = r8b.BatchResampler(0, 0, maxin, nch=S.NCH, stage=desc, **lib_kw)
        for k, v in (opts or {}).items():
            b.set_option(k, v)
        b.set_option("timing", 1)
        return b
    return make


def _chain_maker(e, lib_kw):
    def make(opts):
        b = r8b.BatchResampler(e["src"], e["dst"], e["maxin"], S.TB, e["att"], nch=S.NCH, **lib_kw)
        for k, v in opts.items():
            b.set_option(k, v)
        b.set_option("timing", 1)
        return b
    return make


def _report(e, worst):
    print("stage census: %s worst own-level (over tol_scale): %s" % (e["id"], worst))


def _ids(es):
    return [e["id"] for e in es]


def _tiers(name, entries, run):
    """the emulated id and its gpu-marked twin of every entry"""
    @pytest.mark.parametrize("e", entries, ids=_ids(entries))
    def emulated(emul, e):
        run(e, S.HostTier(), {"lib": emul})

    @pytest.mark.gpu
    @pytest.mark.parametrize("e", entries, ids=_ids(entries))
    def gpu(torch, e):
        run(e, S.DeviceTier(torch), {"device": 0})

    emulated.__name__, gpu.__name__ = "test_%s_emulated" % name, "test_%s_gpu" % name
    emulated.__doc__ = gpu.__doc__ = run.__doc__
    return emulated, gpu


def _run_hb_row(e, tier, lib_kw):
    """stage_census.check_hb_row"""
    _report(e, S.check_hb_row(_stage_maker(S.A_MAXIN, lib_kw), tier, e, _reference()))


def _run_hb_columns(e, tier, lib_kw):
    """stage_census.check_hb_columns"""
    S.check_hb_columns(_stage_maker(S.A_MAXIN, lib_kw), tier, e)


def _run_up_chain(e, tier, lib_kw):
    """stage_census.check_up_chain"""
    _report(e, S.check_up_chain(_chain_maker(e, lib_kw), tier, e, _reference()))


def _run_chain_columns(e, tier, lib_kw):
    """stage_census.check_chain_columns"""
    S.check_chain_columns(_chain_maker(e, lib_kw), tier, e)


def _run_down_chain(e, tier, lib_kw):
    """stage_census.check_down_chain"""
    _report(e, S.check_down_chain(_chain_maker(e, lib_kw), tier, e, _reference()))


def _run_bank(e, tier, lib_kw):
    """stage_census.check_bank"""
    _report(e, S.check_bank(_stage_maker(S.C_MAXIN, lib_kw), tier, e, _reference()))


test_hb_row_emulated, test_hb_row_gpu = _tiers("hb_row", S.PART_A, _run_hb_row)
test_hb_columns_emulated, test_hb_columns_gpu = _tiers("hb_columns", S.A_COLUMNS, _run_hb_columns)
test_up_chain_emulated, test_up_chain_gpu = _tiers("up_chain", S.PART_B_UP, _run_up_chain)
test_chain_columns_emulated, test_chain_columns_gpu = _tiers("chain_columns", S.B_COLUMNS, _run_chain_columns)
test_down_chain_emulated, test_down_chain_gpu = _tiers("down_chain", S.PART_B_DOWN, _run_down_chain)
test_bank_emulated, test_bank_gpu = _tiers("bank", S.PART_C, _run_bank)


def test_census_is_complete():
    """the case module checks its lists against oracle/data/tables.json when it is imported (stage_census._complete):
    every half-band row, every depth 2 ... 8, 8 + 1, 8 + 2 in both directions, every bank length; the exception list is
    the nine one-tap up-sampler rows with one output index each.  The chains that are compared with the compiled
    reference chain are all that hold no one-tap up-sampler, and there are some of each kind"""
    S._complete()
    assert len(S.ONE_TAP_UP) == 9 and S.ONE_TAP_INDEX == 1
    for e in S.PART_B_UP:
        taps = [len(S.tables()["hb"]["third" if e["third"] else "half"][s][r]["taps"]) for s, r, _ in e["hb"]]
        assert e["one_tap"] == (1 in taps)
    compared = [e for e in S.PART_B_UP if not e["one_tap"]]
    assert len(compared) >= len(S.PART_B_UP) // 2 and {tuple(e["runs"]) for e in compared} >= {(2,), (8,), (8, 2)}


@pytest.mark.slow
def test_stages_under_the_address_sanitizer(tmp_path):
    """tests/cxx_stage_census.cpp: the emulation's sources and a stand-alone driver as one program built with
    -fsanitize=address,undefined (tests/emul/Makefile `stages`, minutes of compilation): the chains of part B and one
    row of part A per tap count, the symbols that ran checked.  The LDS arrays of emulated launches are heap blocks
    there: a cascade that writes past its buffers at depth 8 shows up.  Host code only."""
    table = tmp_path / "stage_table.txt"
    with open(table, "w") as f:
        S.dump(f)
    with open(table) as f:
        lines = sum(1 for l in f if l.strip())
    d = os.path.join(ROOT, "tests", "emul")
    out = subprocess.run(["make", "-j8", "stages", "STAGE_TABLE=%s" % table], cwd=d, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and "runtime error" not in out.stdout and "AddressSanitizer" not in out.stdout and \
        out.stdout.strip().endswith("OK"), out.stdout[-3000:]
    assert "%d entries, 0 failed" % lines in out.stdout
