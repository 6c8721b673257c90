// r8b_clip_packed.h -- the PCM boundary of the clip calls for clips packed end to end
// (r8b_batch_resample_clips_packed, include/r8bsrc.h): every clip has a base of its own in the caller's buffer --
// PcmLaunch::clip_base, element offsets the host worked out, one per ROW of a planar side (the clip's offset plus k
// times the clip's own length) and one per CLIP of an interleaved one -- where the strided forms of r8b_clip.h,
// r8b_clip_frames.h and r8b_clip_mix.h multiply by pcm_stride.  Staging rows, windows, lengths, codec, dither key and
// meters are theirs: the phases below ARE their phases, given ClipPacked in the place of ClipStrided (the loops exist
// once), so a packed call's samples are the strided call's bit for bit.
//
// Form: as the strided siblings -- a workgroup per chunk of a row or per tile of a clip, the format switch outside the
// loop; the base is one more wave-uniform load beside the length's (blockIdx.y selects both), and no kernel multiplies
// by a per-clip length.  What differs:
//   ingest   the valid frames come from the clip's base; the staging frames past the clip's end are zeroed as ever, and
//            nothing else is loaded -- regions may overlap or coincide, and what lies between them is never read.
//   egress   a clip's region ends with its last valid frame, so the padding stores are gone: a workgroup whose chunk
//            or tile lies wholly at or past the clip's output length returns after the two uniform loads (before the
//            tile kernel's barrier: the test is the same in every thread), a partial one stores its valid frames
//            alone.  Meters commit as in the strided forms.
//   address  base + frame * channels is 64-bit arithmetic in elements, scaled to bytes last: a buffer may pass 2^32
//            bytes.  A base moves a row off the alignment a stride keeps (any element offset is allowed), which costs
//            partly filled cache lines at a region's two ends and nothing else; profiles/clip_packed_ab.txt.
// Phases are shared with the host emulation of tests/emul (emul_pcm.cpp).
#ifndef R8B_CLIP_PACKED_H
#define R8B_CLIP_PACKED_H

#include "r8b_clip_mix.h"

namespace r8bhip {

// a row's or a clip's own base in the place of ClipStrided's multiple of the stride (r8b_clip.h)
struct ClipPacked
{
	R8B_HD long long operator()(const PcmLaunch& L, int r) const { return L.clip_base[r]; }
	// the mixing ingest's planar clips: a base per row, read where the walk enters the row (FT is a multiple of 64: a wave
	// is in one row per step, so the load is uniform)
	R8B_HD long long rows(const PcmLaunch&, int) const { return 0; }
	R8B_HD long long row(const PcmLaunch& L, int clip, int k) const
	{
		return L.clip_base[(long long) clip * L.mix_channels + R8B_WAVE_UNIFORM(k)];
	}
	R8B_HD int chan(const PcmLaunch&, int r) const { return r; }
};

// whether the chunk or tile that starts at window frame f0 holds a frame below the length of row `row` (w0: the window's
// first frame in the clip)
R8B_HD bool clip_packed_live(const PcmLaunch& L, long long w0, long long f0, int row)
{
	return w0 + f0 < L.clip_len[row];
}

// ------------------------------------------------------------------ planar sides: rows (r8b_clip.h)
R8B_HD void clip_packed_row_in(const PcmLaunch& L, long long f0, int c, int tid, int nthr)
{
	clip_row_in_at(L, ClipPacked(), f0, c, tid, nthr);
}

template<bool DITHER, bool METER, class Commit>
R8B_HD void clip_packed_row_out(const PcmLaunch& L, long long f0, int c, int tid, int nthr, Commit commit)
{
	if (!clip_packed_live(L, L.frame0, f0, c)) return;
	clip_row_out_at<DITHER, METER, false>(L, ClipPacked(), f0, c, tid, nthr, commit);
}

// ------------------------------------------------------------------ interleaved sides: tiles (r8b_clip_frames.h)
// (tile -> staging rows is clip_frames_in_store, staging rows -> tile clip_frames_out_gather: neither touches the PCM side)
R8B_HD void clip_packed_frames_in_load(const PcmLaunch& L, double* tile, int lg, int pitch, long long f0, int clip, int tid,
	int nthr)
{
	clip_frames_in_load_at(L, L.clip_channels, ClipPacked(), tile, lg, pitch, f0, clip, tid, nthr);
}

R8B_HD bool clip_packed_frames_out_live(const PcmLaunch& L, long long f0, int clip)
{
	return clip_packed_live(L, L.frame0, f0, clip * L.clip_channels);
}

R8B_HD void clip_packed_frames_out_store(const PcmLaunch& L, const double* tile, int lg, int pitch, long long f0, int clip,
	int tid, int nthr)
{
	clip_frames_out_store_at<false>(L, ClipPacked(), tile, lg, pitch, f0, clip, tid, nthr);
}

// ------------------------------------------------------------------ the mixing ingest (r8b_clip_mix.h)
// (tile -> staging rows is clip_mix_store)
R8B_HD void clip_packed_mix_load(const PcmLaunch& L, double* tile, int lg, int pitch, long long f0, int clip, int tid,
	int nthr)
{
	if (L.interleaved) clip_frames_in_load_at(L, L.mix_channels, ClipPacked(), tile, lg, pitch, f0, clip, tid, nthr);
	else clip_mix_rows_load(L, ClipPacked(), tile, lg, pitch, f0, clip, tid, nthr);
}

} // namespace r8bhip

#endif
