// r8b_clip_mix.h -- a channel mix in the ingest of the clip calls (r8b_batch_resample_clips_mix, include/r8bsrc.h): the
// caller's buffer holds clips of Kin = PcmLaunch::mix_channels channels, the object takes K = PcmLaunch::clip_channels
// channels per clip, and staging row i K + m receives  sum over k of mix[m Kin + k] x channel k  of clip i.  A mix is
// linear, so it commutes with the resampler: taken here, where every sample passes through a kernel anyway, it costs no
// pass over memory and everything behind the ingest runs on K / Kin of the channels.
// Lengths, windows and padding are r8b_clip.h's, the tile -- FT = 1 << clip_tile_log2(Kin) frames, Kin rows of FT + pad
// doubles, within kClipTileDoubles -- is r8b_clip_frames.h's with Kin in the place of its K.  Two phases:
//   load   an interleaved buffer by clip_frames_in_load_k (lanes on consecutive samples of the clip's valid frames), a
//          planar one row by row (lanes on the frames of row i Kin + k, masked by the clip's length).  Frames at or
//          past the clip's length are not loaded and their tile entries never read.
//   mix    element e = (m, f), m = e >> lg, f = e & (FT - 1): FT is a multiple of 64, so a wave holds ONE m per step --
//          the coefficients mix[m Kin + k] and the test for zero are wave-uniform, and the lanes read tile[k pitch + f]
//          on consecutive doubles, conflict free whatever the pad.  Frames of the window past the clip's end are +0.0.
// The sample is specified bit for bit (include/r8bsrc.h): over the k with a non-zero coefficient in ascending order,
// one multiply, then one fma per further k; clip_mix_sample below is that chain, compiled for the device and by the
// host emulation of tests/emul (emul_pcm.cpp, -ffp-contract=off) alike -- the fma is explicit, and the lone
// multiply has no addition next to it that a contracting compiler could fuse.
// Coefficients: the matrix can be 64 x 64 doubles, 32 KB, which no kernel argument carries; it lies in device memory
// (a block of the call's slot, r8b_capi.cpp) and is read through the SCALAR path: R8B_WAVE_UNIFORM makes m provably
// uniform, so the row's address is scalar, and R8B_MIX_ROW names the matrix as constant memory -- nothing writes it
// while the kernel runs, but the compiler cannot know that of a plain pointer behind whose loads the kernel stores, and
// would fetch every coefficient with a vector load of one address.  The coefficients then arrive by s_load through the
// constant cache, several per instruction, and live in scalar registers: no LDS beside the tile, no vector register
// per coefficient.  The chain is written without a branch (the zero test selects), so that the loads of a row do not
// wait for one another.  Loads only on the scalar side: every store of this kernel is a vector store.
#ifndef R8B_CLIP_MIX_H
#define R8B_CLIP_MIX_H

#include "r8b_clip_frames.h"

// an int that is the same in every lane of a wave, said so that the compiler can keep it in a scalar register
// (r8b_kernels.hip: readfirstlane; the host emulation has no lanes)
#ifndef R8B_WAVE_UNIFORM
#define R8B_WAVE_UNIFORM(x) (x)
#endif
// a row of the matrix: read-only for the kernel's lifetime (r8b_kernels.hip: a pointer into the constant address space)
#ifndef R8B_MIX_ROW
#define R8B_MIX_ROW const double*
#endif

namespace r8bhip {

// one staging sample: row = the Kin coefficients of the object channel, col = the frame's column of the tile
R8B_HD double clip_mix_sample(R8B_MIX_ROW row, int Kin, const double* col, int pitch)
{
	double acc = 0.0;
	bool any = false;
	for (int k = 0; k < Kin; k++)
	{
		const double g = row[k], x = col[k * pitch];
		const bool on = g != 0.0;
		const double t = any ? fma(g, x, acc) : g * x;
		acc = on ? t : acc;
		any = any || on;
	}
	return acc;
}

// ------------------------------------------------------------------ load
// planar PCM -> tile: lanes walk the frames of one row (base: where the clip's rows start, ClipStrided of r8b_clip.h)
template<int FMT, class Base>
R8B_HD void clip_mix_rows_load_t(const PcmLaunch& L, Base base, double* tile, int lg, int pitch, long long f0, int clip,
	int tid, int nthr)
{
	constexpr int B = pcm_io_bytes(FMT);
	const int Kin = L.mix_channels, FT = 1 << lg;
	int nf, nv;
	clip_tile_range(L, L.in_frame0, f0, FT, clip, &nf, &nv);
	const unsigned char* src = static_cast<const unsigned char*>(L.pcm) + (base.rows(L, clip) + L.in_frame0 + f0) * B;
	for (int e = tid; e < (Kin << lg); e += nthr)
	{
		const int k = e >> lg, f = e & (FT - 1);
		if (f < nv) tile[k * pitch + f] = pcm_io_decode(src + (base.row(L, clip, k) + f) * B, FMT);
	}
}

template<class Base>
R8B_HD void clip_mix_rows_load(const PcmLaunch& L, Base base, double* tile, int lg, int pitch, long long f0, int clip,
	int tid, int nthr)
{
	pcm_io_instance(L.fmt, [&](auto fmt) { clip_mix_rows_load_t<decltype(fmt)::value>(L, base, tile, lg, pitch, f0, clip, tid, nthr); });
}

R8B_HD void clip_mix_load(const PcmLaunch& L, double* tile, int lg, int pitch, long long f0, int clip, int tid, int nthr)
{
	if (L.interleaved) clip_frames_in_load_k(L, L.mix_channels, tile, lg, pitch, f0, clip, tid, nthr);
	else clip_mix_rows_load(L, ClipStrided(), tile, lg, pitch, f0, clip, tid, nthr);
}

// ------------------------------------------------------------------ mix and store
// tile -> staging rows: lanes walk the frames of one object channel; padding is +0.0
R8B_HD void clip_mix_store(const PcmLaunch& L, const double* tile, int lg, int pitch, long long f0, int clip, int tid,
	int nthr)
{
	const int K = L.clip_channels, Kin = L.mix_channels, FT = 1 << lg;
	int nf, nv;
	clip_tile_range(L, L.in_frame0, f0, FT, clip, &nf, &nv);
	double* dst = L.planar + (long long) clip * K * L.planar_stride + f0;
	for (int e = tid; e < (K << lg); e += nthr)
	{
		const int m = R8B_WAVE_UNIFORM(e >> lg), f = e & (FT - 1);
		if (f < nf)
			dst[(long long) m * L.planar_stride + f] = f < nv ? clip_mix_sample((R8B_MIX_ROW) L.mix + m * Kin, Kin, tile + f, pitch) : 0.0;
	}
}

} // namespace r8bhip

#endif
