"""The convolver's table unit on its own (csrc/r8b_conv_tables.h; CPU tier): tests/cxx_conv_tables.cpp states what it
asserts -- the layouts of the pair kernel's constants with an index-coded spectrum, the real builders against the complex
ones, the twiddle table, the radix plans, the whole-step rows and the two-phase tables with their cache."""
import os
import subprocess

from conftest import ROOT


def test_conv_tables_stand_alone():
    """`make tables` of tests/emul/Makefile: ONE program from r8b_conv_tables.cpp, r8b_design.cpp, r8b_plan.cpp and the
    driver, built with that Makefile's SAN flags (-fsanitize=address,undefined; the three sanitized objects are shared with
    its other sanitizer runs), nothing preloaded.  No engine and no launcher object is linked: that the program links at all
    is the check that the table unit is host-only.  Host code only."""
    run = subprocess.run(["make", "-j3", "tables"], cwd=os.path.join(ROOT, "tests", "emul"), stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0 and "runtime error" not in run.stdout and "AddressSanitizer" not in run.stdout and \
        run.stdout.strip().endswith("OK"), run.stdout[-3000:]
