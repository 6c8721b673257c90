// tests/emul/emul_clip_frames.cpp -- TEST INFRASTRUCTURE ONLY, an addition to emul_clips.cpp that leaves it as it is:
// the host stand-in of launch_pcm_in / launch_pcm_out as r8b_kernels.hip has them now -- the tile kernels of
// r8b_clip_frames.h when a launch carries clip lengths AND an interleaved layout, else what emul_clips.cpp provides
// (clip_frames.mk compiles it with its launchers renamed to launch_pcm_in_clips / launch_pcm_out_clips).
// tests/test_clip_frames.py loads the library clip_frames.mk builds, _build/libr8bsrc_emul_clip_frames.so.
// A workgroup is the kernels' very phases run for tid = 0 .. 255 one after the other, the barrier being the end of a
// loop over the threads; the stand-in for the wave reduction and the atomics folds every thread's record into the
// channel's meters as it comes.
#include <stdexcept>
#include <vector>

#define R8B_HD inline
#define R8B_LDS_WINDOW(N, v, p) { for (int i_ = 0; i_ < (N); i_++) (v)[i_] = (p)[i_]; }
#define R8B_LDS_ARRIVED(N, v, o)
#include "r8b_clip_frames.h"

namespace r8bhip {

void launch_pcm_in_clips(const PcmLaunch& L, void* stream);  // emul_clips.cpp's launch_pcm_in
void launch_pcm_out_clips(const PcmLaunch& L, void* stream); // emul_clips.cpp's launch_pcm_out

namespace {

// what the device launcher refuses, and the grid
void frames_grid(const PcmLaunch& L, long long* tiles, int* clips, int* lg)
{
	const int K = L.clip_channels;
	if (K < 1 || K > kClipChannelsMax || L.nch % K != 0)
		throw std::logic_error("launch_pcm: clip_channels must be 1 .. 64 and divide the channel count");
	*lg = clip_tile_log2(K);
	*tiles = (L.n + (1LL << *lg) - 1) >> *lg;
	*clips = L.nch / K;
}

// (NaN wherever a phase must not read before it has written)
std::vector<double> fresh_tile()
{
	return std::vector<double>(kClipTileDoubles, __builtin_nan(""));
}

template<bool DITHER, bool METER>
void emul_frames_out(const PcmLaunch& L)
{
	auto commit = [&L](int ch, const PcmMeter& m)
	{
		if (m.peak > L.m_peak[ch]) L.m_peak[ch] = m.peak;
		L.m_clipped[ch] += m.clipped;
		L.m_nonfinite[ch] += m.nonfinite;
	};
	long long tiles;
	int clips, lg;
	frames_grid(L, &tiles, &clips, &lg);
	const int pitch = (1 << lg) + clip_tile_pad(L.clip_channels, kClipLanesOut);
	for (int i = 0; i < clips; i++)
		for (long long t = 0; t < tiles; t++)
		{
			std::vector<double> tile = fresh_tile();
			for (int tid = 0; tid < 256; tid++) clip_frames_out_gather<DITHER, METER>(L, tile.data(), lg, pitch, t << lg, i, tid, 256, commit);
			for (int tid = 0; tid < 256; tid++) clip_frames_out_store(L, tile.data(), lg, pitch, t << lg, i, tid, 256);
		}
}

} // namespace

void launch_pcm_in(const PcmLaunch& L, void* stream)
{
	if (L.clip_len == nullptr || !L.interleaved)
	{
		launch_pcm_in_clips(L, stream);
		return;
	}
	if (L.n <= 0 || L.nch <= 0) return;
	long long tiles;
	int clips, lg;
	frames_grid(L, &tiles, &clips, &lg);
	const int pitch = (1 << lg) + clip_tile_pad(L.clip_channels, kClipLanesIn);
	for (int i = 0; i < clips; i++)
		for (long long t = 0; t < tiles; t++)
		{
			std::vector<double> tile = fresh_tile();
			for (int tid = 0; tid < 256; tid++) clip_frames_in_load(L, tile.data(), lg, pitch, t << lg, i, tid, 256);
			for (int tid = 0; tid < 256; tid++) clip_frames_in_store(L, tile.data(), lg, pitch, t << lg, i, tid, 256);
		}
}

void launch_pcm_out(const PcmLaunch& L, void* stream)
{
	if (L.clip_len == nullptr || !L.interleaved)
	{
		launch_pcm_out_clips(L, stream);
		return;
	}
	if (L.n <= 0 || L.nch <= 0) return;
	const bool meter = L.m_peak != nullptr;
	if (meter && (L.m_clipped == nullptr || L.m_nonfinite == nullptr))
		throw std::logic_error("launch_pcm_out: meters need all three arrays");
	if (L.dither != 0 && meter) emul_frames_out<true, true>(L);
	else if (meter) emul_frames_out<false, true>(L);
	else if (L.dither != 0) emul_frames_out<true, false>(L);
	else emul_frames_out<false, false>(L);
}

} // namespace r8bhip
