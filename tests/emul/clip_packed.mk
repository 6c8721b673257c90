# tests/emul/clip_packed.mk -- TEST INFRASTRUCTURE ONLY: the host emulation library of clip_mix.mk once more, with the
# packed forms of r8b_clip_packed.h added by emul_clip_packed.cpp.  The five stand-ins below it are compiled unchanged but
# for names: emul_launch.cpp, emul_pcm_finish.cpp, emul_clips.cpp and emul_clip_frames.cpp as clip_mix.mk has them,
# emul_clip_mix.cpp's launch_pcm_in / launch_pcm_out become launch_pcm_in_mix / launch_pcm_out_mix (the names it calls
# itself, launch_pcm_in_frames / launch_pcm_out_frames, are other tokens and stay); emul_clip_packed.cpp's launch_pcm_in /
# launch_pcm_out run the packed phases when a launch carries clip_base and forward to the *_mix ones otherwise.
# Output: tests/emul/_build/libr8bsrc_emul_clip_packed.so (tests/test_clip_packed.py).
CSRC := ../../r8brain-free-src_amd/csrc
OUT := _build
CXX ?= g++
FLAGS := -std=c++17 -O2 -g -ffp-contract=off -fPIC -fvisibility=hidden -Wall -Wextra -Wno-unknown-pragmas -DR8B_TEST_HOOKS -I$(CSRC)

SRCS := $(CSRC)/r8b_design.cpp $(CSRC)/r8b_plan.cpp $(CSRC)/r8b_engine.cpp $(CSRC)/r8b_capi.cpp emul_clip_packed.cpp
HDRS := $(wildcard $(CSRC)/*.h) $(CSRC)/r8b_tables.inc ../../include/r8bsrc.h
OBJS := $(OUT)/clip_packed/emul_launch.o $(OUT)/clip_packed/emul_pcm_finish.o $(OUT)/clip_packed/emul_clips.o \
	$(OUT)/clip_packed/emul_clip_frames.o $(OUT)/clip_packed/emul_clip_mix.o

$(OUT)/libr8bsrc_emul_clip_packed.so: $(SRCS) emul_launch.cpp emul_pcm_finish.cpp emul_clips.cpp emul_clip_frames.cpp emul_clip_mix.cpp $(HDRS)
	mkdir -p $(OUT)/clip_packed
	$(CXX) $(FLAGS) -Dlaunch_pcm_in=launch_pcm_in_base -Dlaunch_pcm_out=launch_pcm_out_plain -c emul_launch.cpp -o $(OUT)/clip_packed/emul_launch.o
	$(CXX) $(FLAGS) -Dlaunch_pcm_out=launch_pcm_out_base -c emul_pcm_finish.cpp -o $(OUT)/clip_packed/emul_pcm_finish.o
	$(CXX) $(FLAGS) -Dlaunch_pcm_in=launch_pcm_in_clips -Dlaunch_pcm_out=launch_pcm_out_clips -c emul_clips.cpp -o $(OUT)/clip_packed/emul_clips.o
	$(CXX) $(FLAGS) -Dlaunch_pcm_in=launch_pcm_in_frames -Dlaunch_pcm_out=launch_pcm_out_frames -c emul_clip_frames.cpp -o $(OUT)/clip_packed/emul_clip_frames.o
	$(CXX) $(FLAGS) -Dlaunch_pcm_in=launch_pcm_in_mix -Dlaunch_pcm_out=launch_pcm_out_mix -c emul_clip_mix.cpp -o $(OUT)/clip_packed/emul_clip_mix.o
	$(CXX) $(FLAGS) -shared $(SRCS) $(OBJS) -o $@

# AddressSanitizer + UndefinedBehaviorSanitizer run of the packed phases on the host: the same sources and
# ../cxx_clip_packed.cpp as ONE program (no library, nothing preloaded), built and run by `make -f clip_packed.mk asan`
# (-fno-sanitize=shift: the 24-bit decoder of r8b_pcm_codec.h sign-extends by shifting a negative int left, which every
# compiler this builds with defines as C++20 does)
SAN := -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize=shift -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wno-unknown-pragmas -DR8B_TEST_HOOKS -I$(CSRC)
asan: $(OUT)/asan/cxx_clip_packed
	$(OUT)/asan/cxx_clip_packed
$(OUT)/asan/cxx_clip_packed: $(SRCS) emul_launch.cpp emul_pcm_finish.cpp emul_clips.cpp emul_clip_frames.cpp emul_clip_mix.cpp ../cxx_clip_packed.cpp $(HDRS)
	mkdir -p $(OUT)/asan
	$(CXX) $(SAN) -Dlaunch_pcm_in=launch_pcm_in_base -Dlaunch_pcm_out=launch_pcm_out_plain -c emul_launch.cpp -o $(OUT)/asan/emul_launch.o
	$(CXX) $(SAN) -Dlaunch_pcm_out=launch_pcm_out_base -c emul_pcm_finish.cpp -o $(OUT)/asan/emul_pcm_finish.o
	$(CXX) $(SAN) -Dlaunch_pcm_in=launch_pcm_in_clips -Dlaunch_pcm_out=launch_pcm_out_clips -c emul_clips.cpp -o $(OUT)/asan/emul_clips.o
	$(CXX) $(SAN) -Dlaunch_pcm_in=launch_pcm_in_frames -Dlaunch_pcm_out=launch_pcm_out_frames -c emul_clip_frames.cpp -o $(OUT)/asan/emul_clip_frames.o
	$(CXX) $(SAN) -Dlaunch_pcm_in=launch_pcm_in_mix -Dlaunch_pcm_out=launch_pcm_out_mix -c emul_clip_mix.cpp -o $(OUT)/asan/emul_clip_mix.o
	$(CXX) $(SAN) $(SRCS) ../cxx_clip_packed.cpp $(OUT)/asan/emul_launch.o $(OUT)/asan/emul_pcm_finish.o $(OUT)/asan/emul_clips.o $(OUT)/asan/emul_clip_frames.o $(OUT)/asan/emul_clip_mix.o -o $@
.PHONY: asan
