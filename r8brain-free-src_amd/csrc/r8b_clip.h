// r8b_clip.h -- the PCM boundary for a batch of clips of unequal length (r8b_batch_resample_clips, include/r8bsrc.h):
// the planar row kernels of r8b_pcm.h once more, masked by a per-channel frame count (PcmLaunch::clip_len).
//
// The caller's buffers hold WHOLE clips, row c starting at frame 0 of clip c; the staging rows hold the window of one
// process() step.  The ingest decodes frames [in_frame0, in_frame0 + n) of every row into staging frames [0, n); a
// frame at or past the clip's length becomes +0.0 without a load -- the stream the reference's oneshot() feeds once a
// clip has ended (reference CDSPResampler.h:592-651) -- so whatever the caller's row holds there (another clip's
// samples, NaN, nothing at all past the allocation's end) never enters.  The egress encodes staging frames [0, n) to
// frames [frame0, frame0 + n) of every row; a frame at or past the clip's output length is written as the format's
// encoded zero without a load of the staging row, and is neither dithered nor metered.  Dither and meters go through
// the codec functions and the commit of pcm_row_finish_t: a frame's dither index is its frame number in the clip.
//
// Form: as pcm_row_in_t / pcm_row_finish_t -- a workgroup per kPcmRowChunk frames of the window of ONE channel, the
// format switch outside the loop, the channel's length one uniform load.  The frames of a chunk split at one point
// into the valid ones, converted by the very loop of the unmasked kernels, and the padding, which is stores alone.
// Phases are shared with the host emulation of tests/emul (emul_pcm.cpp).
#ifndef R8B_CLIP_H
#define R8B_CLIP_H

#include "r8b_pcm.h"

namespace r8bhip {

// the chunk [f0, f1) of the window and the frame fv in it at which the padding starts (window frames; w0: the window's
// first frame in the clip)
R8B_HD void clip_chunk(const PcmLaunch& L, long long w0, long long f0, int c, long long* f1, long long* fv)
{
	long long e = f0 + kPcmRowChunk;
	if (e > L.n) e = L.n;
	long long v = L.clip_len[c] - w0;
	if (v > e) v = e;
	if (v < f0) v = f0;
	*f1 = e;
	*fv = v;
}

// the first frame >= fv among f0 + tid, f0 + tid + nthr, ... (fv >= f0)
R8B_HD long long clip_first_pad(long long f0, long long fv, int tid, int nthr)
{
	long long f = f0 + tid;
	if (f < fv) f += (fv - f + nthr - 1) / nthr * nthr;
	return f;
}

// Where a row of a planar side -- or a clip of an interleaved one, r8b_clip_frames.h -- starts in the PCM buffer, in
// elements.  The phases take the rule as a parameter and apply it where they always worked the address out: the strided
// calls multiply by the common stride, the packed ones (r8b_clip_packed.h) read the row's or clip's own base.
struct ClipStrided
{
	R8B_HD long long operator()(const PcmLaunch& L, int r) const { return (long long) r * L.pcm_stride; }
	// the mixing ingest's planar clips (r8b_clip_mix.h): a clip's first row, and its row k from there
	R8B_HD long long rows(const PcmLaunch& L, int clip) const { return (long long) clip * L.mix_channels * L.pcm_stride; }
	R8B_HD long long row(const PcmLaunch& L, int, int k) const { return (long long) k * L.pcm_stride; }
	// the object channel of staging row r, for the egress's dither key and meters: the row itself, unless the clips ride
	// in another order (ClipSched, r8b_clip_sched.h)
	R8B_HD int chan(const PcmLaunch&, int r) const { return r; }
};

template<int FMT, class Base>
R8B_HD void clip_row_in_t(const PcmLaunch& L, Base base, long long f0, int c, int tid, int nthr)
{
	constexpr int B = pcm_io_bytes(FMT);
	const unsigned char* src = static_cast<const unsigned char*>(L.pcm) + (base(L, c) + L.in_frame0) * B;
	double* dst = L.planar + (long long) c * L.planar_stride;
	long long f1, fv;
	clip_chunk(L, L.in_frame0, f0, c, &f1, &fv);
	// (a one-byte format: the valid frames alone are the row the wide loads may touch)
	if constexpr (B == 1) pcm8_row_decode<FMT>(src, dst, f0, fv, tid, nthr);
	else
	{
#pragma unroll 8
		for (long long f = f0 + tid; f < fv; f += nthr) dst[f] = pcm_decode(src + f * B, FMT);
	}
	for (long long f = clip_first_pad(f0, fv, tid, nthr); f < f1; f += nthr) dst[f] = 0.0;
}

template<class Base>
R8B_HD void clip_row_in_at(const PcmLaunch& L, Base base, long long f0, int c, int tid, int nthr)
{
	pcm_io_instance(L.fmt, [&](auto fmt) { clip_row_in_t<decltype(fmt)::value>(L, base, f0, c, tid, nthr); });
}

R8B_HD void clip_row_in(const PcmLaunch& L, long long f0, int c, int tid, int nthr)
{
	clip_row_in_at(L, ClipStrided(), f0, c, tid, nthr);
}

// egress: the valid frames as pcm_row_finish_t has them (with neither dither nor meters: pcm_row_out_t's bytes), the
// thread commits once, after its frames.  PAD: the chunk's frames past the clip's end are
// stored as encoded zeros (the strided call; a packed clip has no room for them)
template<int FMT, bool DITHER, bool METER, bool PAD, class Base, class Commit>
R8B_HD void clip_row_out_t(const PcmLaunch& L, Base base, long long f0, int c, int tid, int nthr, Commit commit)
{
	constexpr int B = pcm_io_bytes(FMT);
	constexpr bool DITH = DITHER && pcm_io_dithers(FMT);
	unsigned char* dst = static_cast<unsigned char*>(L.pcm) + (base(L, c) + L.frame0) * B;
	const double* src = L.planar + (long long) c * L.planar_stride;
	long long f1, fv;
	clip_chunk(L, L.frame0, f0, c, &f1, &fv);
	const int ch = base.chan(L, c);
	const unsigned long long key = DITH ? pcm_dither_key(L.seed, (long long) L.first_channel + ch) : 0;
	PcmMeter m;
	if constexpr (B == 1)
	{
		// (the valid frames and the padding are rows of their own: a wide store never straddles the two, nor the chunk's end)
		pcm8_row_encode<FMT, DITH, METER>(dst, src, f0, fv, key, L.frame0, m, tid, nthr);
		if (PAD)
		{
			int clipped;
			pcm8_row_fill(dst, fv, f1, pcm8_encode(FMT, 0.0, 0.0, &clipped), tid, nthr);
		}
	}
	else
	{
#pragma unroll 8
		for (long long f = f0 + tid; f < fv; f += nthr)
		{
			const double v = src[f];
			const int clipped = pcm_encode_dithered(dst + f * B, FMT, v, DITH ? pcm_dither_keyed(key, L.frame0 + f) : 0.0);
			if (METER) pcm_meter_note(m, v, clipped);
		}
		if (PAD)
			for (long long f = clip_first_pad(f0, fv, tid, nthr); f < f1; f += nthr) pcm_encode(dst + f * B, FMT, 0.0);
	}
	if (METER) commit(ch, m);
}

template<bool DITHER, bool METER, bool PAD, class Base, class Commit>
R8B_HD void clip_row_out_at(const PcmLaunch& L, Base base, long long f0, int c, int tid, int nthr, Commit commit)
{
	pcm_io_instance(L.fmt, [&](auto fmt)
	{
		clip_row_out_t<decltype(fmt)::value, DITHER, METER, PAD>(L, base, f0, c, tid, nthr, commit);
	});
}

template<bool DITHER, bool METER, class Commit>
R8B_HD void clip_row_out(const PcmLaunch& L, long long f0, int c, int tid, int nthr, Commit commit)
{
	clip_row_out_at<DITHER, METER, true>(L, ClipStrided(), f0, c, tid, nthr, commit);
}

} // namespace r8bhip

#endif
