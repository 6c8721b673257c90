// tests/emul/emul_clip_packed.cpp -- TEST INFRASTRUCTURE ONLY, an addition to emul_clip_mix.cpp that leaves it as it is:
// the host stand-in of launch_pcm_in / launch_pcm_out as r8b_kernels.hip has them now -- the packed forms of
// r8b_clip_packed.h when a launch carries clip lengths AND clip_base, else what emul_clip_mix.cpp provides
// (clip_packed.mk compiles it with its launchers renamed to launch_pcm_in_mix / launch_pcm_out_mix).
// tests/test_clip_packed.py loads the library clip_packed.mk builds, _build/libr8bsrc_emul_clip_packed.so.
// A workgroup is the kernels' very phases run for tid = 0 .. 255 one after the other, the barrier being the end of a
// loop over the threads; the stand-in for the wave reduction and the atomics folds every thread's record into the
// channel's meters as it comes.
#include <stdexcept>
#include <vector>

#define R8B_HD inline
#define R8B_LDS_WINDOW(N, v, p) { for (int i_ = 0; i_ < (N); i_++) (v)[i_] = (p)[i_]; }
#define R8B_LDS_ARRIVED(N, v, o)
#include "r8b_clip_packed.h"

namespace r8bhip {

void launch_pcm_in_mix(const PcmLaunch& L, void* stream);  // emul_clip_mix.cpp's launch_pcm_in
void launch_pcm_out_mix(const PcmLaunch& L, void* stream); // emul_clip_mix.cpp's launch_pcm_out

namespace {

// what the device launcher refuses
void check_clips(const PcmLaunch& L)
{
	const int K = L.clip_channels;
	if (K < 1 || K > kClipChannelsMax || L.nch % K != 0)
		throw std::logic_error("launch_pcm: clip_channels must be 1 .. 64 and divide the channel count");
}

// (NaN wherever a phase must not read before it has written)
std::vector<double> fresh_tile()
{
	return std::vector<double>(kClipTileDoubles, __builtin_nan(""));
}

// the ingest's tile kernels: Kt channels of a clip in the PCM buffer (clip_channels, or mix_channels with a mix)
void emul_tiles_in(const PcmLaunch& L, int Kt, bool mixing)
{
	const int lg = clip_tile_log2(Kt), pitch = (1 << lg) + clip_tile_pad(Kt, kClipLanesIn);
	if ((long long) Kt * pitch > kClipTileDoubles) throw std::logic_error("launch_pcm_in: the tile exceeds kClipTileDoubles");
	const long long tiles = (L.n + (1LL << lg) - 1) >> lg;
	for (int i = 0; i < L.nch / L.clip_channels; i++)
		for (long long t = 0; t < tiles; t++)
		{
			std::vector<double> tile = fresh_tile();
			for (int tid = 0; tid < 256; tid++)
			{
				if (mixing) clip_packed_mix_load(L, tile.data(), lg, pitch, t << lg, i, tid, 256);
				else clip_packed_frames_in_load(L, tile.data(), lg, pitch, t << lg, i, tid, 256);
			}
			for (int tid = 0; tid < 256; tid++)
			{
				if (mixing) clip_mix_store(L, tile.data(), lg, pitch, t << lg, i, tid, 256);
				else clip_frames_in_store(L, tile.data(), lg, pitch, t << lg, i, tid, 256);
			}
		}
}

template<bool DITHER, bool METER>
void emul_packed_out(const PcmLaunch& L)
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
				for (int t = 0; t < 256; t++) clip_packed_row_out<DITHER, METER>(L, f0, c, t, 256, commit);
		return;
	}
	const int K = L.clip_channels, lg = clip_tile_log2(K), pitch = (1 << lg) + clip_tile_pad(K, kClipLanesOut);
	const long long tiles = (L.n + (1LL << lg) - 1) >> lg;
	for (int i = 0; i < L.nch / K; i++)
		for (long long t = 0; t < tiles; t++)
		{
			if (!clip_packed_frames_out_live(L, t << lg, i)) continue;
			std::vector<double> tile = fresh_tile();
			for (int tid = 0; tid < 256; tid++) clip_frames_out_gather<DITHER, METER>(L, tile.data(), lg, pitch, t << lg, i, tid, 256, commit);
			for (int tid = 0; tid < 256; tid++) clip_packed_frames_out_store(L, tile.data(), lg, pitch, t << lg, i, tid, 256);
		}
}

} // namespace

void launch_pcm_in(const PcmLaunch& L, void* stream)
{
	if (L.clip_len == nullptr || L.clip_base == nullptr)
	{
		launch_pcm_in_mix(L, stream);
		return;
	}
	if (L.n <= 0 || L.nch <= 0) return;
	check_clips(L);
	if (L.mix_channels != 0)
	{
		if (L.mix_channels < 1 || L.mix_channels > kClipChannelsMax || L.mix == nullptr)
			throw std::logic_error("launch_pcm_in: mix_channels must be 1 .. 64 and come with a matrix");
		emul_tiles_in(L, L.mix_channels, true);
	}
	else if (L.interleaved) emul_tiles_in(L, L.clip_channels, false);
	else
		for (int c = 0; c < L.nch; c++)
			for (long long f0 = 0; f0 < L.n; f0 += kPcmRowChunk)
				for (int t = 0; t < 256; t++) clip_packed_row_in(L, f0, c, t, 256);
}

void launch_pcm_out(const PcmLaunch& L, void* stream)
{
	if (L.clip_len == nullptr || L.clip_base == nullptr)
	{
		launch_pcm_out_mix(L, stream);
		return;
	}
	if (L.n <= 0 || L.nch <= 0) return;
	check_clips(L);
	const bool meter = L.m_peak != nullptr;
	if (meter && (L.m_clipped == nullptr || L.m_nonfinite == nullptr))
		throw std::logic_error("launch_pcm_out: meters need all three arrays");
	if (L.dither != 0 && meter) emul_packed_out<true, true>(L);
	else if (meter) emul_packed_out<false, true>(L);
	else if (L.dither != 0) emul_packed_out<true, false>(L);
	else emul_packed_out<false, false>(L);
}

} // namespace r8bhip
