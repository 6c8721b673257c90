# tests/emul/clip_mix.mk -- TEST INFRASTRUCTURE ONLY: the host emulation library of clip_frames.mk once more, with the
# mixing ingest of r8b_clip_mix.h added by emul_clip_mix.cpp.  The four stand-ins below it are compiled unchanged but for
# names: emul_launch.cpp, emul_pcm_finish.cpp and emul_clips.cpp as clip_frames.mk has them, emul_clip_frames.cpp's
# launch_pcm_in / launch_pcm_out become launch_pcm_in_frames / launch_pcm_out_frames (the names it calls itself,
# launch_pcm_in_clips / launch_pcm_out_clips, are other tokens and stay); emul_clip_mix.cpp's launch_pcm_in runs the mix
# phases when a launch carries mix_channels and forwards to the *_frames ones otherwise, its launch_pcm_out forwards.
# Output: tests/emul/_build/libr8bsrc_emul_clip_mix.so (tests/test_clip_mix.py).
CSRC := ../../r8brain-free-src_amd/csrc
OUT := _build
CXX ?= g++
FLAGS := -std=c++17 -O2 -g -ffp-contract=off -fPIC -fvisibility=hidden -Wall -Wextra -Wno-unknown-pragmas -DR8B_TEST_HOOKS -I$(CSRC)

SRCS := $(CSRC)/r8b_design.cpp $(CSRC)/r8b_plan.cpp $(CSRC)/r8b_engine.cpp $(CSRC)/r8b_capi.cpp emul_clip_mix.cpp
HDRS := $(wildcard $(CSRC)/*.h) $(CSRC)/r8b_tables.inc ../../include/r8bsrc.h

$(OUT)/libr8bsrc_emul_clip_mix.so: $(SRCS) emul_launch.cpp emul_pcm_finish.cpp emul_clips.cpp emul_clip_frames.cpp $(HDRS)
	mkdir -p $(OUT)/clip_mix
	$(CXX) $(FLAGS) -Dlaunch_pcm_in=launch_pcm_in_base -Dlaunch_pcm_out=launch_pcm_out_plain -c emul_launch.cpp -o $(OUT)/clip_mix/emul_launch.o
	$(CXX) $(FLAGS) -Dlaunch_pcm_out=launch_pcm_out_base -c emul_pcm_finish.cpp -o $(OUT)/clip_mix/emul_pcm_finish.o
	$(CXX) $(FLAGS) -Dlaunch_pcm_in=launch_pcm_in_clips -Dlaunch_pcm_out=launch_pcm_out_clips -c emul_clips.cpp -o $(OUT)/clip_mix/emul_clips.o
	$(CXX) $(FLAGS) -Dlaunch_pcm_in=launch_pcm_in_frames -Dlaunch_pcm_out=launch_pcm_out_frames -c emul_clip_frames.cpp -o $(OUT)/clip_mix/emul_clip_frames.o
	$(CXX) $(FLAGS) -shared $(SRCS) $(OUT)/clip_mix/emul_launch.o $(OUT)/clip_mix/emul_pcm_finish.o $(OUT)/clip_mix/emul_clips.o $(OUT)/clip_mix/emul_clip_frames.o -o $@
