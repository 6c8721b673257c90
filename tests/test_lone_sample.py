"""A lone sample swept across every lane of the pair kernels' cross-lane reductions (tests/lone_sample_cases.py): the
emulation tier (CPU, tests/emul -- its reductions are sequential, so it proves the inputs and the expectations: the
reference and the shared arithmetic of r8b_convp.h stay inside the own-level bounds for a lone sample beside a partner at
1e-12 and at 1e-9) and the GPU tier (-m gpu: ballot, DPP, readlane, lane exchanges and the per-wave words of
r8b_kernels.hip on the device).  Every id names its geometry, the kernel symbol that ran (asserted from stage_symbols()),
the pass of the sweep and the variant."""
import importlib
import os

import pytest

import cases
from conftest import ROOT
from lone_sample_cases import GEOMETRIES, GEOMETRY, DeviceRunner, HostRunner, check_lone_sample, passes

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
    """the compiled reference where oracle/_ref was built (assertion 1); the numpy oracle serves everywhere (assertion 2)"""
    import refwrap as R
    return R if R.available() else None


def _maker(g, lib_kw):
    def make(nch):
        b = r8b.BatchResampler(g["src"], g["dst"], g["maxin"], g["tb"], g["att"], nch=nch, **lib_kw)
        for k, v in g["opts"].items():
            b.set_option(k, v)
        return b
    return make


def _sweep(names, max_pairs=None):
    """(geometry, pass, variant) of every pass of the named geometries, and their ids"""
    params, ids = [], []
    for name in names:
        g = GEOMETRY[name]
        ps = passes(g, max_pairs)
        # no position skipped: the passes' positions add up to the first convolver's in_len
        assert sum(k for _, k, _ in ps) == g["in_len"] and [p for p, _, _ in ps] == [sum(k for _, k, _ in ps[:i]) for i in range(len(ps))]
        assert ps[-1][2] and not any(u for _, _, u in ps[:-1])
        for i, ps_i in enumerate(ps):
            for variant in ("A",) if g["solo"] else ("A", "B", "F"):
                params.append((name, ps_i, variant))
                ids.append("%s-%s-%dof%d-%s" % (name, g["symbol"].replace(" ", ""), i + 1, len(ps), variant))
    return params, ids


# the emulated twin: fft=32/64 (many blocks per wave), fft=1024/2048 (two blocks per workgroup) and cfg2, 256 pairs per object
_EMUL, _EMUL_IDS = _sweep(["fft32", "fft1024", "cfg2"], max_pairs=256)
_GPU, _GPU_IDS = _sweep([g["name"] for g in GEOMETRIES])


@pytest.mark.parametrize("name,sweep_pass,variant", _EMUL, ids=_EMUL_IDS)
def test_emulated_lone_sample_sweep(emul, name, sweep_pass, variant):
    g = GEOMETRY[name]
    p0, npairs, unpaired = sweep_pass
    check_lone_sample(_maker(g, {"lib": emul}), HostRunner(), g, variant, p0, npairs, unpaired, _reference())


@pytest.mark.gpu
@pytest.mark.parametrize("name,sweep_pass,variant", _GPU, ids=_GPU_IDS)
def test_hip_lone_sample_sweep(torch, name, sweep_pass, variant):
    """every pair-kernel form of lone_sample_cases.GEOMETRIES on the device; the one-channel form (modes 10 / 11 / 18, id
    `solo`) has no partner, but r8b_convp.h applies the silence decision to it (cp_silence on the workgroup's
    collect_bits), so variant A's silence and reference assertions run on its lone-sample channels.
    R8B_LONE_SAMPLE_RECORD=<file>: appends the pass's figures (profiles/lone_sample_sweep.txt is made from them)."""
    g = GEOMETRY[name]
    p0, npairs, unpaired = sweep_pass
    rec = check_lone_sample(_maker(g, {"device": 0}), DeviceRunner(torch), g, variant, p0, npairs, unpaired, _reference())
    print("lone sample sweep: %s %s %s pairs %d ref %s oracle %s" % (name, g["symbol"], variant, rec["pairs"], rec["ref"],
                                                                  rec["oracle"]))
    path = os.environ.get("R8B_LONE_SAMPLE_RECORD")
    if path:
        with open(path, "a") as f:
            f.write("%s\t%s\t%s\t%d\t%r\t%r\n" % (name, g["symbol"], variant, rec["pairs"], rec["ref"], rec["oracle"]))
