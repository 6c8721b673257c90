// tests/emul/emul_clips.cpp -- TEST INFRASTRUCTURE ONLY, an addition to emul_launch.cpp and emul_pcm_finish.cpp that
// leaves both as they are: the host stand-in of launch_pcm_in / launch_pcm_out as r8b_kernels.hip has them now -- the
// masked row kernels of r8b_clip.h when a launch carries clip lengths (PcmLaunch::clip_len), else what the two files
// provide (clips.mk compiles them with their launchers renamed to launch_pcm_in_base / launch_pcm_out_base).
// tests/test_clips.py loads the library clips.mk builds, _build/libr8bsrc_emul_clips.so.
// Like the emulator's other launchers it runs the very phases the kernels run for tid = 0 .. 255; the stand-in for the
// wave reduction and the atomics folds every thread's record into the channel's meters as it comes.
#include <stdexcept>

#define R8B_HD inline
#define R8B_LDS_WINDOW(N, v, p) { for (int i_ = 0; i_ < (N); i_++) (v)[i_] = (p)[i_]; }
#define R8B_LDS_ARRIVED(N, v, o)
#include "r8b_clip.h"

namespace r8bhip {

void launch_pcm_in_base(const PcmLaunch& L, void* stream);  // emul_launch.cpp's launch_pcm_in
void launch_pcm_out_base(const PcmLaunch& L, void* stream); // emul_pcm_finish.cpp's launch_pcm_out

template<bool DITHER, bool METER>
static void emul_clip_out(const PcmLaunch& L)
{
	auto commit = [&L](int ch, const PcmMeter& m)
	{
		if (m.peak > L.m_peak[ch]) L.m_peak[ch] = m.peak;
		L.m_clipped[ch] += m.clipped;
		L.m_nonfinite[ch] += m.nonfinite;
	};
	for (int c = 0; c < L.nch; c++)
		for (long long f0 = 0; f0 < L.n; f0 += kPcmRowChunk)
			for (int t = 0; t < 256; t++) clip_row_out<DITHER, METER>(L, f0, c, t, 256, commit);
}

void launch_pcm_in(const PcmLaunch& L, void* stream)
{
	if (L.clip_len == nullptr)
	{
		launch_pcm_in_base(L, stream);
		return;
	}
	if (L.interleaved) throw std::logic_error("launch_pcm: clip lengths go with planar buffers");
	for (int c = 0; c < L.nch; c++)
		for (long long f0 = 0; f0 < L.n; f0 += kPcmRowChunk)
			for (int t = 0; t < 256; t++) clip_row_in(L, f0, c, t, 256);
}

void launch_pcm_out(const PcmLaunch& L, void* stream)
{
	if (L.clip_len == nullptr)
	{
		launch_pcm_out_base(L, stream);
		return;
	}
	if (L.interleaved) throw std::logic_error("launch_pcm: clip lengths go with planar buffers");
	const bool meter = L.m_peak != nullptr;
	if (L.dither != 0 && meter) emul_clip_out<true, true>(L);
	else if (meter) emul_clip_out<false, true>(L);
	else if (L.dither != 0) emul_clip_out<true, false>(L);
	else emul_clip_out<false, false>(L);
}

} // namespace r8bhip
