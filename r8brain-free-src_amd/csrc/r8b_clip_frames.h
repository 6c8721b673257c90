// r8b_clip_frames.h -- the PCM boundary for a batch of INTERLEAVED clips of unequal length (r8b_batch_resample_clips_ex,
// include/r8bsrc.h): clip i holds K = PcmLaunch::clip_channels channels frame-major, sample (frame f, channel k) at element
// i * pcm_stride + f * K + k of the caller's buffer, and goes through rows i K .. i K + K - 1 of the staging window.
// Lengths, windows, padding, dither and meters are r8b_clip.h's: clip_len holds one frame count per ROW (the clip's,
// K times), a frame at or past it is neither loaded nor dithered nor metered.
//
// Form: a workgroup takes one tile of one clip, FT frames x K channels -- FT = 1 << clip_tile_log2(K), the largest power
// of two with FT * K <= kClipTileSamples (64 at the least) -- through an LDS array of K rows of FT + pad doubles.  The
// tile kernels of r8b_pcm.h reach coalesced accesses by letting lanes walk 64 channels of one frame; a clip has a few
// channels and a base of its own, so here the lanes of the PCM side walk CONSECUTIVE SAMPLES of the clip's frame range
// (sample s of the tile is frame s / K, channel s % K: a thread keeps the pair by adding, without a division in the
// loop), and the lanes of the staging side walk the frames of one row: FT is a multiple of 64, so the 64 lanes of a
// wave hold one channel per step -- what a wave's meter reduction needs (PcmMeterCommit).  A thread notes at most
// FT / 256 samples of a channel before it commits them (the packed counts).
// All egress arithmetic happens on the staging side; the PCM side of the egress is stores only.
// LDS banks: the staging side's lanes are on consecutive doubles of a row, whatever the pitch.  The PCM side's lanes
// sit at k * pitch + f with k fast and f slow, where kPcmPitch's pad of one double (lanes on 64 rows of one column)
// would put lanes (k, f + 1) and (k + 1, f) on one bank -- min(K, lanes / K)-way.  The pad is lanes / K doubles
// instead (clip_tile_pad: FT is a multiple of 32, so row k starts k * lanes / K banks on and the lanes of a service
// group -- 16 for the ingest's ds_write_b64, 32 for the egress's ds_read_b64 -- fall on banks of their own when K is
// a power of two, and all but one or two of them when it is not); one double from K = 16 / 32 on.
// Phases are shared with the host emulation of tests/emul (emul_pcm.cpp).
#ifndef R8B_CLIP_FRAMES_H
#define R8B_CLIP_FRAMES_H

#include "r8b_clip.h"

namespace r8bhip {

// samples of a tile the frame count is chosen for (a power of two; 8 per thread).  Measured on 1024 channels of S16 -> F32
// clips (profiles/clip_frames_ab.txt): 2048 samples -- 16 KB of LDS, nine workgroups per CU -- run within 2 % of
// the planar row kernels, 4096 and 512 samples 11 - 13 % behind them.  Clips of more than 32 channels take 64 frames
// whatever the product (a wave holds one channel per step), up to 64 x kPcmTile samples
#ifndef R8B_CLIP_TILE_SAMPLES
#define R8B_CLIP_TILE_SAMPLES 2048
#endif
static const int kClipTileSamples = R8B_CLIP_TILE_SAMPLES;
// K rows of FT + pad doubles, K <= kPcmTile: the largest tile a launch may ask for (K = 64: 64 rows of 65)
static const int kClipTileDoubles = (kClipTileSamples > 64 * kPcmTile ? kClipTileSamples : 64 * kPcmTile) + kPcmTile;
static_assert(kClipTileSamples >= 256 && (kClipTileSamples & (kClipTileSamples - 1)) == 0, "a power of two, a sample per thread");
static_assert(kClipChannelsMax == kPcmTile, "r8b_launch.h states the bound for the host side");

// log2 of the tile's frames FT for clips of K channels (constexpr: the kernels and the host launcher both call it)
constexpr int clip_tile_log2(int K)
{
	int lg = 6;
	while ((2 << lg) * K <= kClipTileSamples) lg++;
	return lg;
}

// doubles between the rows of the tile beyond FT, for the `lanes` lanes LDS serves together on the PCM side
// (R8B_CLIP_PITCH_ODD: kPcmPitch's single double, for the measurement in profiles/clip_frames_ab.txt)
constexpr int clip_tile_pad(int K, int lanes)
{
#ifdef R8B_CLIP_PITCH_ODD
	(void) K;
	(void) lanes;
	return 1;
#else
	return K >= lanes ? 1 : (lanes + K - 1) / K;
#endif
}
static const int kClipLanesIn = 16, kClipLanesOut = 32; // ds_write_b64 / ds_read_b64 service groups

// the tile's window frames [f0, f0 + *nf) and the number *nv of them below the clip's length (w0: the window's first
// frame in the clip)
R8B_HD void clip_tile_range(const PcmLaunch& L, long long w0, long long f0, int FT, int clip, int* nf, int* nv)
{
	long long e = f0 + FT;
	if (e > L.n) e = L.n;
	long long v = L.clip_len[clip * L.clip_channels] - w0;
	if (v > e) v = e;
	if (v < f0) v = f0;
	*nf = (int) (e - f0);
	*nv = (int) (v - f0);
}

// ------------------------------------------------------------------ ingest
// PCM -> tile: lanes walk consecutive samples of the clip's valid frames.  K: the channels of a clip in the PCM buffer
// -- L.clip_channels here, the mix's input channels in r8b_clip_mix.h (the clip's length is that of its first ROW
// either way: clip_tile_range); base -- where the clip starts in the PCM buffer (ClipStrided, r8b_clip.h)
template<int FMT, class Base>
R8B_HD void clip_frames_in_load_t(const PcmLaunch& L, int K, Base base, double* tile, int lg, int pitch, long long f0,
	int clip, int tid, int nthr)
{
	constexpr int B = pcm_io_bytes(FMT);
	const int FT = 1 << lg;
	int nf, nv;
	clip_tile_range(L, L.in_frame0, f0, FT, clip, &nf, &nv);
	const unsigned char* src = static_cast<const unsigned char*>(L.pcm) + (base(L, clip) + (L.in_frame0 + f0) * K) * B;
	const int ns = nv * K, df = nthr / K, dk = nthr - df * K;
	int f = tid / K, k = tid - f * K;
#pragma unroll 4
	for (int s = tid; s < ns; s += nthr)
	{
		tile[k * pitch + f] = pcm_io_decode(src + (long long) s * B, FMT);
		f += df;
		k += dk;
		if (k >= K)
		{
			k -= K;
			f++;
		}
	}
}

template<class Base>
R8B_HD void clip_frames_in_load_at(const PcmLaunch& L, int K, Base base, double* tile, int lg, int pitch,
	long long f0, int clip, int tid, int nthr)
{
	pcm_io_instance(L.fmt, [&](auto fmt) { clip_frames_in_load_t<decltype(fmt)::value>(L, K, base, tile, lg, pitch, f0, clip, tid, nthr); });
}

R8B_HD void clip_frames_in_load_k(const PcmLaunch& L, int K, double* tile, int lg, int pitch, long long f0, int clip,
	int tid, int nthr)
{
	clip_frames_in_load_at(L, K, ClipStrided(), tile, lg, pitch, f0, clip, tid, nthr);
}

R8B_HD void clip_frames_in_load(const PcmLaunch& L, double* tile, int lg, int pitch, long long f0, int clip, int tid,
	int nthr)
{
	clip_frames_in_load_k(L, L.clip_channels, tile, lg, pitch, f0, clip, tid, nthr);
}

// tile -> staging rows: lanes walk the frames of one row; padding is +0.0
R8B_HD void clip_frames_in_store(const PcmLaunch& L, const double* tile, int lg, int pitch, long long f0, int clip, int tid,
	int nthr)
{
	const int K = L.clip_channels, FT = 1 << lg;
	int nf, nv;
	clip_tile_range(L, L.in_frame0, f0, FT, clip, &nf, &nv);
	double* dst = L.planar + (long long) clip * K * L.planar_stride + f0;
	for (int e = tid; e < (K << lg); e += nthr)
	{
		const int c = e >> lg, f = e & (FT - 1);
		if (f < nf) dst[(long long) c * L.planar_stride + f] = f < nv ? tile[c * pitch + f] : 0.0;
	}
}

// ------------------------------------------------------------------ egress
// staging rows -> tile: lanes walk the frames of one row.  An integer format's samples go into the tile dithered, rounded
// and saturated (exact as doubles), a float format's as they are, padding as 0.0; a thread commits a channel's meter
// record when its walk leaves the channel (every lane of a wave at the same step: FT is a multiple of 64).  base: names
// the object channel of a staging row (ClipStrided::chan, r8b_clip.h), read where the walk enters the row
template<bool DITHER, bool METER, class Base, class Commit>
R8B_HD void clip_frames_out_gather_at(const PcmLaunch& L, Base base, double* tile, int lg, int pitch, long long f0, int clip,
	int tid, int nthr, Commit commit)
{
	const int K = L.clip_channels, FT = 1 << lg;
	int nf, nv;
	clip_tile_range(L, L.frame0, f0, FT, clip, &nf, &nv);
	const double scale = pcm_io_scale(L.fmt);
	const bool dith = DITHER && pcm_io_dithers(L.fmt); // (G.711 rounds at its scale undithered)
	const double* src = L.planar + (long long) clip * K * L.planar_stride + f0;
	const int ch0 = clip * K;
	PcmMeter m;
	unsigned long long key = 0;
	int cc = -1, och = 0;
	for (int e = tid; e < (K << lg); e += nthr)
	{
		const int c = e >> lg, f = e & (FT - 1);
		if (c != cc)
		{
			if (METER && cc >= 0) commit(och, m);
			m = PcmMeter();
			cc = c;
			if (METER || dith) och = base.chan(L, ch0 + c);
			if (dith) key = pcm_dither_key(L.seed, (long long) L.first_channel + och);
		}
		if (f < nv)
		{
			const double v = src[(long long) c * L.planar_stride + f];
			double t = v;
			int clipped = fabs(v) > 1.0;
			if (scale != 0.0)
				t = pcm_quantize_dithered(v, scale, dith ? pcm_dither_keyed(key, L.frame0 + f0 + f) : 0.0, &clipped);
			tile[c * pitch + f] = t;
			if (METER) pcm_meter_note(m, v, clipped);
		}
		else if (f < nf) tile[c * pitch + f] = 0.0;
	}
	if (METER && cc >= 0) commit(och, m);
}

template<bool DITHER, bool METER, class Commit>
R8B_HD void clip_frames_out_gather(const PcmLaunch& L, double* tile, int lg, int pitch, long long f0, int clip, int tid,
	int nthr, Commit commit)
{
	clip_frames_out_gather_at<DITHER, METER>(L, ClipStrided(), tile, lg, pitch, f0, clip, tid, nthr, commit);
}

// tile -> PCM: lanes walk consecutive samples of the clip's frame range; stores only.  PAD: the tile's frames
// past the clip's end are stored too, as the encoded zeros the gather left (the strided call; a packed clip has no room
// for them)
template<int FMT, bool PAD, class Base>
R8B_HD void clip_frames_out_store_t(const PcmLaunch& L, Base base, const double* tile, int lg, int pitch, long long f0,
	int clip, int tid, int nthr)
{
	constexpr int B = pcm_io_bytes(FMT);
	constexpr bool QUANTIZED = pcm_io_dithers(FMT) || B == 1; // (the gather rounded at pcm_io_scale: the integer formats and G.711)
	const int K = L.clip_channels, FT = 1 << lg;
	int nf, nv;
	clip_tile_range(L, L.frame0, f0, FT, clip, &nf, &nv);
	unsigned char* dst = static_cast<unsigned char*>(L.pcm) + (base(L, clip) + (L.frame0 + f0) * K) * B;
	const int ns = (PAD ? nf : nv) * K, df = nthr / K, dk = nthr - df * K;
	int f = tid / K, k = tid - f * K;
#pragma unroll 4
	for (int s = tid; s < ns; s += nthr)
	{
		const double t = tile[k * pitch + f];
		if (QUANTIZED) pcm_io_store_quantized(dst + (long long) s * B, FMT, t);
		else pcm_encode(dst + (long long) s * B, FMT, t);
		f += df;
		k += dk;
		if (k >= K)
		{
			k -= K;
			f++;
		}
	}
}

template<bool PAD, class Base>
R8B_HD void clip_frames_out_store_at(const PcmLaunch& L, Base base, const double* tile, int lg, int pitch,
	long long f0, int clip, int tid, int nthr)
{
	pcm_io_instance(L.fmt, [&](auto fmt) { clip_frames_out_store_t<decltype(fmt)::value, PAD>(L, base, tile, lg, pitch, f0, clip, tid, nthr); });
}

R8B_HD void clip_frames_out_store(const PcmLaunch& L, const double* tile, int lg, int pitch, long long f0, int clip,
	int tid, int nthr)
{
	clip_frames_out_store_at<true>(L, ClipStrided(), tile, lg, pitch, f0, clip, tid, nthr);
}

} // namespace r8bhip

#endif
