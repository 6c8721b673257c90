# tests/emul/clips.mk -- TEST INFRASTRUCTURE ONLY: the host emulation library of finish.mk once more, with the masked
# row kernels of clips of unequal length (r8b_clip.h) added by emul_clips.cpp.  emul_launch.cpp and emul_pcm_finish.cpp
# are compiled unchanged but for names: emul_launch.cpp's launch_pcm_in / launch_pcm_out become launch_pcm_in_base /
# launch_pcm_out_plain, emul_pcm_finish.cpp's launch_pcm_out (the plain or the finishing egress) becomes
# launch_pcm_out_base; emul_clips.cpp's launch_pcm_in / launch_pcm_out run the clip phases when a launch carries
# lengths and forward to the *_base ones otherwise.  Output: tests/emul/_build/libr8bsrc_emul_clips.so
# (tests/test_clips.py).
CSRC := ../../r8brain-free-src_amd/csrc
OUT := _build
CXX ?= g++
FLAGS := -std=c++17 -O2 -g -ffp-contract=off -fPIC -fvisibility=hidden -Wall -Wextra -Wno-unknown-pragmas -DR8B_TEST_HOOKS -I$(CSRC)

SRCS := $(CSRC)/r8b_design.cpp $(CSRC)/r8b_plan.cpp $(CSRC)/r8b_engine.cpp $(CSRC)/r8b_capi.cpp emul_clips.cpp
HDRS := $(wildcard $(CSRC)/*.h) $(CSRC)/r8b_tables.inc ../../include/r8bsrc.h

$(OUT)/libr8bsrc_emul_clips.so: $(SRCS) emul_launch.cpp emul_pcm_finish.cpp $(HDRS)
	mkdir -p $(OUT)/clips
	$(CXX) $(FLAGS) -Dlaunch_pcm_in=launch_pcm_in_base -Dlaunch_pcm_out=launch_pcm_out_plain -c emul_launch.cpp -o $(OUT)/clips/emul_launch.o
	$(CXX) $(FLAGS) -Dlaunch_pcm_out=launch_pcm_out_base -c emul_pcm_finish.cpp -o $(OUT)/clips/emul_pcm_finish.o
	$(CXX) $(FLAGS) -shared $(SRCS) $(OUT)/clips/emul_launch.o $(OUT)/clips/emul_pcm_finish.o -o $@
