// r8b_clip_sched.h -- the PCM egress of the clip calls for clips scheduled longest first
// (r8b_batch_resample_clips_sched with R8B_CLIPS_LONGEST_FIRST, include/r8bsrc.h): clip order[g] rides in slot g, i.e.
// in staging rows g K .. g K + K - 1, so a staging row is no longer the caller's object channel of the same number.
// What is per row or per clip and filled by the host -- the lengths (PcmLaunch::clip_len) and the bases
// (PcmLaunch::clip_base) -- comes permuted from there, and a STRIDED side of an ordered call gets bases as well (row or
// clip times the stride, worked out on the host): every ordered side addresses through clip_base.  The ingest therefore
// IS the packed ingest of r8b_clip_packed.h.  The egress needs two things the packed forms do not have:
//   clip_chan  the object channel of each staging row (PcmLaunch::clip_chan).  The dither key and the meter commit go by
//              it -- the caller's numbering: a clip's dither and its meters do not depend on the slot it rode in.  One
//              more wave-uniform load beside the length's and the base's: blockIdx.y selects the row kernel's, the tile
//              kernel reads it where its walk enters a row (FT is a multiple of 64: a wave is in one row per step).
//   clip_pad   an ordered strided output keeps its padding -- encoded zeros up to the call's longest output in every row
//              -- so these forms address by base AND store the padding: clip_row_out_at<..., PAD = true> and
//              clip_frames_out_store_at<true> with the base rule below.  Such a launch covers every row of the object,
//              also the rows a dropping call (R8B_CLIPS_DROP_FINISHED) no longer computes: their lengths lie at or
//              below the window's first frame, so they store padding and load nothing.
// The phases ARE r8b_clip.h's and r8b_clip_frames.h's, given ClipSched in the place of ClipStrided / ClipPacked (the
// loops exist once); no kernel multiplies by a per-clip length.  Without padding, a workgroup whose chunk or tile lies
// wholly at or past the row's length returns after the uniform loads, as in the packed forms.
// Phases are shared with the host emulation of tests/emul (emul_pcm.cpp); which launch runs these forms: r8b_pcm_dispatch.h.
#ifndef R8B_CLIP_SCHED_H
#define R8B_CLIP_SCHED_H

#include "r8b_clip_packed.h"

namespace r8bhip {

// ClipPacked's bases, and the row's object channel from clip_chan (null: the row itself)
struct ClipSched
{
	R8B_HD long long operator()(const PcmLaunch& L, int r) const { return L.clip_base[r]; }
	R8B_HD int chan(const PcmLaunch& L, int r) const
	{
		return L.clip_chan != nullptr ? (int) L.clip_chan[R8B_WAVE_UNIFORM(r)] : r;
	}
};

// does the launch need these forms?  (host side: asked by r8b_pcm_dispatch.h alone, for device launcher and emulator alike)
inline bool clip_sched_launch(const PcmLaunch& L)
{
	return L.clip_len != nullptr && L.clip_base != nullptr && (L.clip_chan != nullptr || L.clip_pad != 0);
}

// ------------------------------------------------------------------ planar sides: rows
template<bool DITHER, bool METER, bool PAD, class Commit>
R8B_HD void clip_sched_row_out(const PcmLaunch& L, long long f0, int c, int tid, int nthr, Commit commit)
{
	if (!PAD && !clip_packed_live(L, L.frame0, f0, c)) return;
	clip_row_out_at<DITHER, METER, PAD>(L, ClipSched(), f0, c, tid, nthr, commit);
}

// ------------------------------------------------------------------ interleaved sides: tiles
// (PAD: every tile of the window is stored; else as clip_packed_frames_out_live)
template<bool PAD>
R8B_HD bool clip_sched_frames_out_live(const PcmLaunch& L, long long f0, int clip)
{
	return PAD || clip_packed_live(L, L.frame0, f0, clip * L.clip_channels);
}

template<bool DITHER, bool METER, class Commit>
R8B_HD void clip_sched_frames_out_gather(const PcmLaunch& L, double* tile, int lg, int pitch, long long f0, int clip, int tid,
	int nthr, Commit commit)
{
	clip_frames_out_gather_at<DITHER, METER>(L, ClipSched(), tile, lg, pitch, f0, clip, tid, nthr, commit);
}

template<bool PAD>
R8B_HD void clip_sched_frames_out_store(const PcmLaunch& L, const double* tile, int lg, int pitch, long long f0, int clip,
	int tid, int nthr)
{
	clip_frames_out_store_at<PAD>(L, ClipSched(), tile, lg, pitch, f0, clip, tid, nthr);
}

} // namespace r8bhip

#endif
