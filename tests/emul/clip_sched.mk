# tests/emul/clip_sched.mk -- TEST INFRASTRUCTURE ONLY: the host emulation library of clip_packed.mk once more, with the
# scheduled egress forms of r8b_clip_sched.h added by emul_clip_sched.cpp.  The six stand-ins below it are compiled
# unchanged but for names: emul_launch.cpp, emul_pcm_finish.cpp, emul_clips.cpp, emul_clip_frames.cpp and
# emul_clip_mix.cpp as clip_packed.mk has them, emul_clip_packed.cpp's launch_pcm_in / launch_pcm_out become
# launch_pcm_in_packed / launch_pcm_out_packed (the names it calls itself, launch_pcm_in_mix / launch_pcm_out_mix, are
# other tokens and stay); emul_clip_sched.cpp's launch_pcm_out runs the scheduled phases when a launch carries clip_chan
# or stores padding behind a base and forwards to the *_packed ones otherwise.
# Output: tests/emul/_build/libr8bsrc_emul_clip_sched.so (tests/test_clip_sched.py).
CSRC := ../../r8brain-free-src_amd/csrc
OUT := _build
CXX ?= g++
FLAGS := -std=c++17 -O2 -g -ffp-contract=off -fPIC -fvisibility=hidden -Wall -Wextra -Wno-unknown-pragmas -DR8B_TEST_HOOKS -I$(CSRC)

SRCS := $(CSRC)/r8b_design.cpp $(CSRC)/r8b_plan.cpp $(CSRC)/r8b_engine.cpp $(CSRC)/r8b_capi.cpp emul_clip_sched.cpp
HDRS := $(wildcard $(CSRC)/*.h) $(CSRC)/r8b_tables.inc ../../include/r8bsrc.h
STANDINS := emul_launch.cpp emul_pcm_finish.cpp emul_clips.cpp emul_clip_frames.cpp emul_clip_mix.cpp emul_clip_packed.cpp
NAMES := emul_launch.o emul_pcm_finish.o emul_clips.o emul_clip_frames.o emul_clip_mix.o emul_clip_packed.o

# the stand-ins under their names, into directory $(1) with the flags $(2)
define STANDIN_OBJS
	mkdir -p $(1)
	$(CXX) $(2) -Dlaunch_pcm_in=launch_pcm_in_base -Dlaunch_pcm_out=launch_pcm_out_plain -c emul_launch.cpp -o $(1)/emul_launch.o
	$(CXX) $(2) -Dlaunch_pcm_out=launch_pcm_out_base -c emul_pcm_finish.cpp -o $(1)/emul_pcm_finish.o
	$(CXX) $(2) -Dlaunch_pcm_in=launch_pcm_in_clips -Dlaunch_pcm_out=launch_pcm_out_clips -c emul_clips.cpp -o $(1)/emul_clips.o
	$(CXX) $(2) -Dlaunch_pcm_in=launch_pcm_in_frames -Dlaunch_pcm_out=launch_pcm_out_frames -c emul_clip_frames.cpp -o $(1)/emul_clip_frames.o
	$(CXX) $(2) -Dlaunch_pcm_in=launch_pcm_in_mix -Dlaunch_pcm_out=launch_pcm_out_mix -c emul_clip_mix.cpp -o $(1)/emul_clip_mix.o
	$(CXX) $(2) -Dlaunch_pcm_in=launch_pcm_in_packed -Dlaunch_pcm_out=launch_pcm_out_packed -c emul_clip_packed.cpp -o $(1)/emul_clip_packed.o
endef

$(OUT)/libr8bsrc_emul_clip_sched.so: $(SRCS) $(STANDINS) $(HDRS)
	$(call STANDIN_OBJS,$(OUT)/clip_sched,$(FLAGS))
	$(CXX) $(FLAGS) -shared $(SRCS) $(addprefix $(OUT)/clip_sched/,$(NAMES)) -o $@

# AddressSanitizer + UndefinedBehaviorSanitizer run of the scheduled forms on the host: the same sources and
# ../cxx_clip_sched.cpp as ONE program (no library, nothing preloaded), built and run by `make -f clip_sched.mk asan`
# (-fno-sanitize=shift: the 24-bit decoder of r8b_pcm_codec.h sign-extends by shifting a negative int left, which every
# compiler this builds with defines as C++20 does)
SAN := -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize=shift -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wno-unknown-pragmas -DR8B_TEST_HOOKS -I$(CSRC)
asan: $(OUT)/asan_sched/cxx_clip_sched
	$(OUT)/asan_sched/cxx_clip_sched
$(OUT)/asan_sched/cxx_clip_sched: $(SRCS) $(STANDINS) ../cxx_clip_sched.cpp $(HDRS)
	$(call STANDIN_OBJS,$(OUT)/asan_sched,$(SAN))
	$(CXX) $(SAN) $(SRCS) ../cxx_clip_sched.cpp $(addprefix $(OUT)/asan_sched/,$(NAMES)) -o $@
.PHONY: asan
