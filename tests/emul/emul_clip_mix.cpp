// tests/emul/emul_clip_mix.cpp -- TEST INFRASTRUCTURE ONLY, an addition to emul_clip_frames.cpp that leaves it as it is:
// the host stand-in of launch_pcm_in / launch_pcm_out as r8b_kernels.hip has them now -- the mixing ingest of
// r8b_clip_mix.h when a launch carries clip lengths AND mix_channels, else what emul_clip_frames.cpp provides
// (clip_mix.mk compiles it with its launchers renamed to launch_pcm_in_frames / launch_pcm_out_frames).
// tests/test_clip_mix.py loads the library clip_mix.mk builds, _build/libr8bsrc_emul_clip_mix.so.
// A workgroup is the kernel's very phases run for tid = 0 .. 255 one after the other, the barrier being the end of a
// loop over the threads.
#include <stdexcept>
#include <vector>

#define R8B_HD inline
#define R8B_LDS_WINDOW(N, v, p) { for (int i_ = 0; i_ < (N); i_++) (v)[i_] = (p)[i_]; }
#define R8B_LDS_ARRIVED(N, v, o)
#include "r8b_clip_mix.h"

namespace r8bhip {

void launch_pcm_in_frames(const PcmLaunch& L, void* stream);  // emul_clip_frames.cpp's launch_pcm_in
void launch_pcm_out_frames(const PcmLaunch& L, void* stream); // emul_clip_frames.cpp's launch_pcm_out

void launch_pcm_in(const PcmLaunch& L, void* stream)
{
	if (L.clip_len == nullptr || L.mix_channels == 0)
	{
		launch_pcm_in_frames(L, stream);
		return;
	}
	if (L.n <= 0 || L.nch <= 0) return;
	// what the device launcher refuses, and the grid
	const int K = L.clip_channels, Kin = L.mix_channels;
	if (K < 1 || K > kClipChannelsMax || L.nch % K != 0)
		throw std::logic_error("launch_pcm: clip_channels must be 1 .. 64 and divide the channel count");
	if (Kin < 1 || Kin > kClipChannelsMax || L.mix == nullptr)
		throw std::logic_error("launch_pcm_in: mix_channels must be 1 .. 64 and come with a matrix");
	const int lg = clip_tile_log2(Kin), pitch = (1 << lg) + clip_tile_pad(Kin, kClipLanesIn);
	if ((long long) Kin * pitch > kClipTileDoubles) throw std::logic_error("launch_pcm_in: the tile exceeds kClipTileDoubles");
	const long long tiles = (L.n + (1LL << lg) - 1) >> lg;
	for (int i = 0; i < L.nch / K; i++)
		for (long long t = 0; t < tiles; t++)
		{
			// (NaN wherever a phase must not read before it has written)
			std::vector<double> tile(kClipTileDoubles, __builtin_nan(""));
			for (int tid = 0; tid < 256; tid++) clip_mix_load(L, tile.data(), lg, pitch, t << lg, i, tid, 256);
			for (int tid = 0; tid < 256; tid++) clip_mix_store(L, tile.data(), lg, pitch, t << lg, i, tid, 256);
		}
}

void launch_pcm_out(const PcmLaunch& L, void* stream)
{
	launch_pcm_out_frames(L, stream);
}

} // namespace r8bhip
