// tests/emul/emul_pcm_finish.cpp -- TEST INFRASTRUCTURE ONLY, an addition to emul_launch.cpp that leaves that file as
// it is: the host stand-in of launch_pcm_out as r8b_kernels.hip has it now -- the plain egress when neither dither nor
// meters are on, else the finishing egress kernels (r8b_pcm.h).  finish.mk builds the emulation library once more as
// _build/libr8bsrc_emul_finish.so with emul_launch.cpp's own launch_pcm_out compiled under the name launch_pcm_out_plain
// and this file's in its place; tests/test_pcm_finish.py loads that library.  (libr8bsrc_emul.so, which the other
// tests load, knows the plain egress alone and ignores the dither and meter fields of a PcmLaunch.)
// Like the emulator's other launchers it runs the very phases the kernels run for tid = 0 .. 255, one loop per
// barrier-separated phase; the stand-in for the wave reduction and the atomics folds every thread's record into the
// channel's meters as it comes.
#include <limits>
#include <vector>

#define R8B_HD inline
#define R8B_LDS_WINDOW(N, v, p) { for (int i_ = 0; i_ < (N); i_++) (v)[i_] = (p)[i_]; }
#define R8B_LDS_ARRIVED(N, v, o)
#include "r8b_pcm.h"

namespace r8bhip {

void launch_pcm_out_plain(const PcmLaunch& L, void* stream); // emul_launch.cpp's launch_pcm_out (finish.mk)

template<bool DITHER, bool METER>
static void emul_pcm_finish(const PcmLaunch& L)
{
	auto commit = [&L](int ch, const PcmMeter& m)
	{
		if (m.peak > L.m_peak[ch]) L.m_peak[ch] = m.peak;
		L.m_clipped[ch] += m.clipped;
		L.m_nonfinite[ch] += m.nonfinite;
	};
	const int nthr = 256;
	if (!L.interleaved)
	{
		for (int c = 0; c < L.nch; c++)
			for (long long f0 = 0; f0 < L.n; f0 += kPcmRowChunk)
				for (int t = 0; t < nthr; t++) pcm_row_finish<DITHER, METER>(L, f0, c, t, nthr, commit);
		return;
	}
	std::vector<double> tile((size_t) kPcmTile * kPcmPitch);
	for (int c0 = 0; c0 < L.nch; c0 += kPcmTile)
		for (long long f0 = 0; f0 < L.n; f0 += kPcmTile)
		{
			// (poisoned: slots the gather leaves alone must never reach the buffer)
			for (double& v : tile) v = std::numeric_limits<double>::quiet_NaN();
			for (int t = 0; t < nthr; t++) pcm_finish_gather<DITHER, METER>(L, tile.data(), f0, c0, t, nthr, commit);
			for (int t = 0; t < nthr; t++) pcm_finish_scatter(L, tile.data(), f0, c0, t, nthr);
		}
}

void launch_pcm_out(const PcmLaunch& L, void* stream)
{
	const bool meter = L.m_peak != nullptr;
	if (L.dither == 0 && !meter)
	{
		launch_pcm_out_plain(L, stream);
		return;
	}
	if (L.n <= 0 || L.nch <= 0) return;
	if (L.dither != 0 && meter) emul_pcm_finish<true, true>(L);
	else if (meter) emul_pcm_finish<false, true>(L);
	else emul_pcm_finish<true, false>(L);
}

} // namespace r8bhip
