# tests/emul/finish.mk -- TEST INFRASTRUCTURE ONLY: the host emulation library of tests/emul/Makefile once more, with
# the finishing PCM egress (dither, meters) added by emul_pcm_finish.cpp.  emul_launch.cpp is compiled unchanged but
# for one name: its launch_pcm_out becomes launch_pcm_out_plain, which emul_pcm_finish.cpp's launch_pcm_out calls when
# neither feature is on.  Output: tests/emul/_build/libr8bsrc_emul_finish.so (tests/test_pcm_finish.py).
CSRC := ../../r8brain-free-src_amd/csrc
OUT := _build
CXX ?= g++
FLAGS := -std=c++17 -O2 -g -ffp-contract=off -fPIC -fvisibility=hidden -Wall -Wextra -Wno-unknown-pragmas -DR8B_TEST_HOOKS -I$(CSRC)

SRCS := $(CSRC)/r8b_design.cpp $(CSRC)/r8b_plan.cpp $(CSRC)/r8b_engine.cpp $(CSRC)/r8b_capi.cpp emul_pcm_finish.cpp
HDRS := $(wildcard $(CSRC)/*.h) $(CSRC)/r8b_tables.inc ../../include/r8bsrc.h

$(OUT)/libr8bsrc_emul_finish.so: $(SRCS) emul_launch.cpp $(HDRS)
	mkdir -p $(OUT)/finish
	$(CXX) $(FLAGS) -Dlaunch_pcm_out=launch_pcm_out_plain -c emul_launch.cpp -o $(OUT)/finish/emul_launch.o
	$(CXX) $(FLAGS) -shared $(SRCS) $(OUT)/finish/emul_launch.o -o $@
