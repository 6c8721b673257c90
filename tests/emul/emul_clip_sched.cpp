// tests/emul/emul_clip_sched.cpp -- TEST INFRASTRUCTURE ONLY, an addition to emul_clip_packed.cpp that leaves it as it is:
// the host stand-in of launch_pcm_in / launch_pcm_out as r8b_kernels.hip has them now -- the egress forms of
// r8b_clip_sched.h when a launch carries clip_chan or stores padding behind a base (clip_sched_launch), else what
// emul_clip_packed.cpp provides (clip_sched.mk compiles it with its launchers renamed to launch_pcm_in_packed /
// launch_pcm_out_packed).  The ingest of an ordered call IS the packed ingest and is forwarded.
// tests/test_clip_sched.py loads the library clip_sched.mk builds, _build/libr8bsrc_emul_clip_sched.so.
// A workgroup is the kernels' very phases run for tid = 0 .. 255 one after the other, the barrier being the end of a
// loop over the threads; the stand-in for the wave reduction and the atomics folds every thread's record into the
// channel's meters as it comes.
#include <stdexcept>
#include <vector>

#define R8B_HD inline
#define R8B_LDS_WINDOW(N, v, p) { for (int i_ = 0; i_ < (N); i_++) (v)[i_] = (p)[i_]; }
#define R8B_LDS_ARRIVED(N, v, o)
#include "r8b_clip_sched.h"

namespace r8bhip {

void launch_pcm_in_packed(const PcmLaunch& L, void* stream);  // emul_clip_packed.cpp's launch_pcm_in
void launch_pcm_out_packed(const PcmLaunch& L, void* stream); // emul_clip_packed.cpp's launch_pcm_out

namespace {

template<bool DITHER, bool METER, bool PAD>
void emul_sched_out(const PcmLaunch& L)
{
	auto commit = [&L](int ch, const PcmMeter& m)
	{
		if (m.peak > L.m_peak[ch]) L.m_peak[ch] = m.peak;
		L.m_clipped[ch] += m.clipped;
		L.m_nonfinite[ch] += m.nonfinite;
	};
	if (!L.interleaved)
	{
		for (int c = 0; c < L.nch; c++)
			for (long long f0 = 0; f0 < L.n; f0 += kPcmRowChunk)
				for (int t = 0; t < 256; t++) clip_sched_row_out<DITHER, METER, PAD>(L, f0, c, t, 256, commit);
		return;
	}
	const int K = L.clip_channels, lg = clip_tile_log2(K), pitch = (1 << lg) + clip_tile_pad(K, kClipLanesOut);
	if ((long long) K * pitch > kClipTileDoubles) throw std::logic_error("launch_pcm_out: the tile exceeds kClipTileDoubles");
	const long long tiles = (L.n + (1LL << lg) - 1) >> lg;
	for (int i = 0; i < L.nch / K; i++)
		for (long long t = 0; t < tiles; t++)
		{
			if (!clip_sched_frames_out_live<PAD>(L, t << lg, i)) continue;
			// (NaN wherever a phase must not read before it has written)
			std::vector<double> tile(kClipTileDoubles, __builtin_nan(""));
			for (int tid = 0; tid < 256; tid++) clip_sched_frames_out_gather<DITHER, METER>(L, tile.data(), lg, pitch, t << lg, i, tid, 256, commit);
			for (int tid = 0; tid < 256; tid++) clip_sched_frames_out_store<PAD>(L, tile.data(), lg, pitch, t << lg, i, tid, 256);
		}
}

template<bool DITHER, bool METER>
void emul_sched_out_pad(const PcmLaunch& L)
{
	if (L.clip_pad != 0) emul_sched_out<DITHER, METER, true>(L);
	else emul_sched_out<DITHER, METER, false>(L);
}

} // namespace

void launch_pcm_in(const PcmLaunch& L, void* stream)
{
	launch_pcm_in_packed(L, stream);
}

void launch_pcm_out(const PcmLaunch& L, void* stream)
{
	if (!clip_sched_launch(L))
	{
		launch_pcm_out_packed(L, stream);
		return;
	}
	if (L.n <= 0 || L.nch <= 0) return;
	const int K = L.clip_channels;
	if (K < 1 || K > kClipChannelsMax || L.nch % K != 0)
		throw std::logic_error("launch_pcm: clip_channels must be 1 .. 64 and divide the channel count");
	const bool meter = L.m_peak != nullptr;
	if (meter && (L.m_clipped == nullptr || L.m_nonfinite == nullptr))
		throw std::logic_error("launch_pcm_out: meters need all three arrays");
	if (L.dither != 0 && meter) emul_sched_out_pad<true, true>(L);
	else if (meter) emul_sched_out_pad<false, true>(L);
	else if (L.dither != 0) emul_sched_out_pad<true, false>(L);
	else emul_sched_out_pad<false, false>(L);
}

} // namespace r8bhip
