# tests/emul/clip_frames.mk -- TEST INFRASTRUCTURE ONLY: the host emulation library of clips.mk once more, with the tile
# kernels of interleaved clips (r8b_clip_frames.h) added by emul_clip_frames.cpp.  emul_launch.cpp, emul_pcm_finish.cpp
# and emul_clips.cpp are compiled unchanged but for names: the first two as clips.mk has them, emul_clips.cpp's
# launch_pcm_in / launch_pcm_out become launch_pcm_in_clips / launch_pcm_out_clips (the names it calls itself,
# launch_pcm_in_base / launch_pcm_out_base, are other tokens and stay); emul_clip_frames.cpp's launch_pcm_in /
# launch_pcm_out run the tile phases when a launch carries lengths and an interleaved layout and forward to the
# *_clips ones otherwise.  Output: tests/emul/_build/libr8bsrc_emul_clip_frames.so (tests/test_clip_frames.py).
CSRC := ../../r8brain-free-src_amd/csrc
OUT := _build
CXX ?= g++
FLAGS := -std=c++17 -O2 -g -ffp-contract=off -fPIC -fvisibility=hidden -Wall -Wextra -Wno-unknown-pragmas -DR8B_TEST_HOOKS -I$(CSRC)

SRCS := $(CSRC)/r8b_design.cpp $(CSRC)/r8b_plan.cpp $(CSRC)/r8b_engine.cpp $(CSRC)/r8b_capi.cpp emul_clip_frames.cpp
HDRS := $(wildcard $(CSRC)/*.h) $(CSRC)/r8b_tables.inc ../../include/r8bsrc.h

$(OUT)/libr8bsrc_emul_clip_frames.so: $(SRCS) emul_launch.cpp emul_pcm_finish.cpp emul_clips.cpp $(HDRS)
	mkdir -p $(OUT)/clip_frames
	$(CXX) $(FLAGS) -Dlaunch_pcm_in=launch_pcm_in_base -Dlaunch_pcm_out=launch_pcm_out_plain -c emul_launch.cpp -o $(OUT)/clip_frames/emul_launch.o
	$(CXX) $(FLAGS) -Dlaunch_pcm_out=launch_pcm_out_base -c emul_pcm_finish.cpp -o $(OUT)/clip_frames/emul_pcm_finish.o
	$(CXX) $(FLAGS) -Dlaunch_pcm_in=launch_pcm_in_clips -Dlaunch_pcm_out=launch_pcm_out_clips -c emul_clips.cpp -o $(OUT)/clip_frames/emul_clips.o
	$(CXX) $(FLAGS) -shared $(SRCS) $(OUT)/clip_frames/emul_launch.o $(OUT)/clip_frames/emul_pcm_finish.o $(OUT)/clip_frames/emul_clips.o -o $@
