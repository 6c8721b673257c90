// r8b_pcm.h -- PCM ingest/egress next to the hot path: interleaved or planar
// int16 / packed int24 / int32 / float32 / float64 samples <-> the planar fp64 rows the resampler
// works on, so that 2-4 bytes per sample cross PCIe and the HBM edge instead of 8.
//
// The reference has no such code in-tree: its command-line tool converts through CWaveFile (the
// external "libvox", absent from the repository; call sites bench/r8bfreesrc.cpp:103,134), and
// oneshot<Tin,Tout> (CDSPResampler.h:592-651) only casts.  The conventions here are the usual PCM
// ones and are part of this library's interface (include/r8bsrc.h):
//   decode: integer / 2^(bits-1); float32 widened exactly
//   encode: v * 2^(bits-1), round to nearest even, saturate to [-2^(bits-1), 2^(bits-1)-1]
//           (plain by default; with TPDF dither added before the rounding in the finishing egress
//           kernels at the end of this file); float32 by round-to-nearest conversion; NaN encodes
//           as 0 in the integer formats
// The one-byte formats -- unsigned 8-bit PCM, G.711 mu-law and A-law (include/r8bsrc.h) -- exist at this
// boundary only: the kernels here decode and encode them, a stage kernel never sees them.
// The sample codec itself lives in r8b_pcm_codec.h (the stage kernels use its five formats too, for planar
// PCM buffers read and written in place; the "boundary codec" on top of them is for this file and r8b_clip*.h).  Phases are shared with the host emulation of tests/emul
// like every other kernel.
#ifndef R8B_PCM_H
#define R8B_PCM_H

#include "r8b_kernel_phases.h"

namespace r8bhip {

// byte offset of (frame f, channel c) in the PCM buffer
R8B_HD long long pcm_offset(const PcmLaunch& L, long long f, int c)
{
	const long long e = L.interleaved ? f * L.pcm_stride + c : (long long) c * L.pcm_stride + f;
	return e * pcm_io_bytes(L.fmt);
}

// A workgroup converts a tile of kPcmTile frames x kPcmTile channels.  Interleaved buffers are
// frame-major, the planar rows channel-major: the tile goes through LDS (pitch kPcmTile + 1) so
// that both sides are accessed with the fastest index on consecutive lanes.
static const int kPcmTile = 64;
static const int kPcmPitch = kPcmTile + 1;

// PCM -> tile (interleaved) : lanes walk channels
R8B_HD void pcm_in_gather(const PcmLaunch& L, double* tile, long long f0, int c0, int tid, int nthr)
{
	const unsigned char* src = static_cast<const unsigned char*>(L.pcm);
	for (int e = tid; e < kPcmTile * kPcmTile; e += nthr)
	{
		const int c = e & (kPcmTile - 1), f = e >> 6;
		if (f0 + f < L.n && c0 + c < L.nch)
			tile[c * kPcmPitch + f] = pcm_io_decode(src + pcm_offset(L, f0 + f, c0 + c), L.fmt);
	}
}

// tile -> planar rows : lanes walk frames
R8B_HD void pcm_in_scatter(const PcmLaunch& L, const double* tile, long long f0, int c0, int tid,
	int nthr)
{
	for (int e = tid; e < kPcmTile * kPcmTile; e += nthr)
	{
		const int f = e & (kPcmTile - 1), c = e >> 6;
		if (f0 + f < L.n && c0 + c < L.nch)
			L.planar[(long long) (c0 + c) * L.planar_stride + f0 + f] = tile[c * kPcmPitch + f];
	}
}

// planar PCM -> planar rows, no transposition
R8B_HD void pcm_in_direct(const PcmLaunch& L, long long f0, int c0, int tid, int nthr)
{
	const unsigned char* src = static_cast<const unsigned char*>(L.pcm);
	for (int e = tid; e < kPcmTile * kPcmTile; e += nthr)
	{
		const int f = e & (kPcmTile - 1), c = e >> 6;
		if (f0 + f < L.n && c0 + c < L.nch)
			L.planar[(long long) (c0 + c) * L.planar_stride + f0 + f] =
				pcm_io_decode(src + pcm_offset(L, f0 + f, c0 + c), L.fmt);
	}
}

R8B_HD void pcm_out_gather(const PcmLaunch& L, double* tile, long long f0, int c0, int tid, int nthr)
{
	for (int e = tid; e < kPcmTile * kPcmTile; e += nthr)
	{
		const int f = e & (kPcmTile - 1), c = e >> 6;
		if (f0 + f < L.n && c0 + c < L.nch)
			tile[c * kPcmPitch + f] = L.planar[(long long) (c0 + c) * L.planar_stride + f0 + f];
	}
}

R8B_HD void pcm_out_scatter(const PcmLaunch& L, const double* tile, long long f0, int c0, int tid,
	int nthr)
{
	unsigned char* dst = static_cast<unsigned char*>(L.pcm);
	for (int e = tid; e < kPcmTile * kPcmTile; e += nthr)
	{
		const int c = e & (kPcmTile - 1), f = e >> 6;
		if (f0 + f < L.n && c0 + c < L.nch)
			pcm_io_encode(dst + pcm_offset(L, f0 + f, c0 + c), L.fmt, tile[c * kPcmPitch + f]);
	}
}

R8B_HD void pcm_out_direct(const PcmLaunch& L, long long f0, int c0, int tid, int nthr)
{
	unsigned char* dst = static_cast<unsigned char*>(L.pcm);
	for (int e = tid; e < kPcmTile * kPcmTile; e += nthr)
	{
		const int f = e & (kPcmTile - 1), c = e >> 6;
		if (f0 + f < L.n && c0 + c < L.nch)
			pcm_io_encode(dst + pcm_offset(L, f0 + f, c0 + c), L.fmt,
				L.planar[(long long) (c0 + c) * L.planar_stride + f0 + f]);
	}
}

// Planar PCM <-> planar rows, row by row (no transposition): a workgroup converts kPcmRowChunk consecutive frames
// of ONE channel, thread tid the frames tid, tid + nthr, ... of the chunk -- consecutive lanes on consecutive
// samples, eight independent loads in flight per thread, the format switch outside the loop.  (The tile form
// above moves 64 frames of a row per instruction and decides the format per sample: 2.2 TB/s on the staging
// passes in front of / behind a fast-path convolver, where this streams.)
static const int kPcmRowChunk = 2048;

// ------------------------------------------------------------------ the one-byte row form
// A row of a one-byte format (kPcmU8, kPcmUlaw, kPcmAlaw) with a lane per sample is a byte load or store per lane, 64
// bytes per wave instruction.  Here a lane takes kPcm8Lane = 4 CONSECUTIVE samples with one dword access.  A row starts
// at any byte (a packed clip's base is any element offset, and base + frame0 moves from step to step), and no byte
// outside the frames [fa, fb) it is given may be read or written (a packed region's neighbours; the page behind an
// input's last sample), so the frames split by the ADDRESS: a head of up to three frames that reach the next multiple of
// four bytes, whole aligned groups, a tail -- head and tail a byte per lane, lanes 0 .. of the workgroup.  Which lane
// converts a sample changes nothing of its value, its dither index (the frame's) or its channel's meters (maxima and
// sums).  Measured against a lane per sample and against eight samples per lane (profiles/pcm8_ab.txt): four is the
// fastest of the three on the ingest and on calls with both sides in one byte, the egress alone does not tell them apart.
static const int kPcm8Lane = 4;
typedef unsigned Pcm8Word;
static_assert(sizeof(Pcm8Word) == kPcm8Lane, "one access of a lane");

// one(f): frame f alone; group(f): frames f .. f + kPcm8Lane - 1, p + f a multiple of kPcm8Lane bytes.  nthr >= kPcm8Lane - 1
template<class One, class Group>
R8B_HD void pcm8_walk(const unsigned char* p, long long fa, long long fb, int tid, int nthr, One one, Group group)
{
	long long fh = fa + (long long) ((0 - (size_t) (p + fa)) & (size_t) (kPcm8Lane - 1));
	if (fh > fb) fh = fb;
	const long long ng = (fb - fh) / kPcm8Lane, ft = fh + ng * kPcm8Lane;
	if (fa + tid < fh) one(fa + tid);
	for (long long g = tid; g < ng; g += nthr) group(fh + g * kPcm8Lane);
	if (ft + tid < fb) one(ft + tid);
}

// frames [fa, fb) of the byte row src -> dst[fa .. fb)
template<int FMT>
R8B_HD void pcm8_row_decode(const unsigned char* src, double* dst, long long fa, long long fb, int tid, int nthr)
{
	typedef Pcm8Word W;
	pcm8_walk(src, fa, fb, tid, nthr,
		[&](long long f) { dst[f] = pcm8_decode(src[f], FMT); },
		[&](long long f)
		{
			W w;
			__builtin_memcpy(&w, __builtin_assume_aligned(src + f, sizeof(W)), sizeof(W));
#pragma unroll
			for (int j = 0; j < (int) sizeof(W); j++) dst[f + j] = pcm8_decode((unsigned) (w >> (8 * j)) & 255u, FMT);
		});
}

// src[fa .. fb) -> frames [fa, fb) of the byte row dst; a frame's dither index is frame0 + f
template<int FMT, bool DITH, bool METER>
R8B_HD void pcm8_row_encode(unsigned char* dst, const double* src, long long fa, long long fb, unsigned long long key,
	long long frame0, PcmMeter& m, int tid, int nthr)
{
	typedef Pcm8Word W;
	auto byte = [&](long long f)
	{
		const double v = src[f];
		int clipped;
		const unsigned b = pcm8_encode(FMT, v, DITH ? pcm_dither_keyed(key, frame0 + f) : 0.0, &clipped);
		if (METER) pcm_meter_note(m, v, clipped);
		return b;
	};
	pcm8_walk(dst, fa, fb, tid, nthr,
		[&](long long f) { dst[f] = (unsigned char) byte(f); },
		[&](long long f)
		{
			W w = 0;
#pragma unroll
			for (int j = 0; j < (int) sizeof(W); j++) w |= (W) byte(f + j) << (8 * j);
			__builtin_memcpy(__builtin_assume_aligned(dst + f, sizeof(W)), &w, sizeof(W));
		});
}

// frames [fa, fb) of the byte row dst = b (a clip's padding: the format's encoded zero)
R8B_HD void pcm8_row_fill(unsigned char* dst, long long fa, long long fb, unsigned b, int tid, int nthr)
{
	typedef Pcm8Word W;
	pcm8_walk(dst, fa, fb, tid, nthr,
		[&](long long f) { dst[f] = (unsigned char) b; },
		[&](long long f)
		{
			const W w = (W) b * (W) 0x01010101u;
			__builtin_memcpy(__builtin_assume_aligned(dst + f, sizeof(W)), &w, sizeof(W));
		});
}

template<int FMT>
R8B_HD void pcm_row_in_t(const PcmLaunch& L, long long f0, int c, int tid, int nthr)
{
	constexpr int B = pcm_io_bytes(FMT);
	const unsigned char* src = static_cast<const unsigned char*>(L.pcm) + (long long) c * L.pcm_stride * B;
	double* dst = L.planar + (long long) c * L.planar_stride;
	long long f1 = f0 + kPcmRowChunk;
	if (f1 > L.n) f1 = L.n;
	if constexpr (B == 1) pcm8_row_decode<FMT>(src, dst, f0, f1, tid, nthr);
	else
	{
#pragma unroll 8
		for (long long f = f0 + tid; f < f1; f += nthr) dst[f] = pcm_decode(src + f * B, FMT);
	}
}

template<int FMT>
R8B_HD void pcm_row_out_t(const PcmLaunch& L, long long f0, int c, int tid, int nthr)
{
	constexpr int B = pcm_io_bytes(FMT);
	unsigned char* dst = static_cast<unsigned char*>(L.pcm) + (long long) c * L.pcm_stride * B;
	const double* src = L.planar + (long long) c * L.planar_stride;
	long long f1 = f0 + kPcmRowChunk;
	if (f1 > L.n) f1 = L.n;
	if constexpr (B == 1)
	{
		PcmMeter m;
		pcm8_row_encode<FMT, false, false>(dst, src, f0, f1, 0, 0, m, tid, nthr);
	}
	else
	{
#pragma unroll 8
		for (long long f = f0 + tid; f < f1; f += nthr) pcm_encode(dst + f * B, FMT, src[f]);
	}
}

R8B_HD void pcm_row_in(const PcmLaunch& L, long long f0, int c, int tid, int nthr)
{
	pcm_io_instance(L.fmt, [&](auto fmt) { pcm_row_in_t<decltype(fmt)::value>(L, f0, c, tid, nthr); });
}

R8B_HD void pcm_row_out(const PcmLaunch& L, long long f0, int c, int tid, int nthr)
{
	pcm_io_instance(L.fmt, [&](auto fmt) { pcm_row_out_t<decltype(fmt)::value>(L, f0, c, tid, nthr); });
}

// ------------------------------------------------------------------ finishing egress: TPDF dither and / or meters
// The two egress forms once more, as kernels of their own (k_pcm_finish<DITHER, METER>, k_pcm_rows_finish<DITHER, METER>),
// so that the plain ones above stay as they are.  Dither (r8b_pcm_codec.h) is a function of the sample's channel number
// and absolute output frame, L.frame0 + its frame in the launch: nothing is carried from call to call.
// Meters: a thread keeps a PcmMeter over the samples of ONE channel it converts and hands it to `commit(channel, m)`,
// which every thread of a wave calls at the same place with the same channel -- the kernel's reduces over the wave and
// issues one atomic per meter (max / add on 64-bit integers: the order of arrival does not matter, the meters are
// deterministic); the host emulation's folds each thread's record into the arrays directly.

// rows: as pcm_row_out_t; the workgroup's channel is one, so a thread commits once, after its frames
template<int FMT, bool DITHER, bool METER, class Commit>
R8B_HD void pcm_row_finish_t(const PcmLaunch& L, long long f0, int c, int tid, int nthr, Commit commit)
{
	constexpr int B = pcm_io_bytes(FMT);
	constexpr bool DITH = DITHER && pcm_io_dithers(FMT);
	unsigned char* dst = static_cast<unsigned char*>(L.pcm) + (long long) c * L.pcm_stride * B;
	const double* src = L.planar + (long long) c * L.planar_stride;
	long long f1 = f0 + kPcmRowChunk;
	if (f1 > L.n) f1 = L.n;
	const unsigned long long key = DITH ? pcm_dither_key(L.seed, (long long) L.first_channel + c) : 0;
	PcmMeter m;
	if constexpr (B == 1) pcm8_row_encode<FMT, DITH, METER>(dst, src, f0, f1, key, L.frame0, m, tid, nthr);
	else
	{
#pragma unroll 8
		for (long long f = f0 + tid; f < f1; f += nthr)
		{
			const double v = src[f];
			const int clipped = pcm_encode_dithered(dst + f * B, FMT, v, DITH ? pcm_dither_keyed(key, L.frame0 + f) : 0.0);
			if (METER) pcm_meter_note(m, v, clipped);
		}
	}
	if (METER) commit(c, m);
}

template<bool DITHER, bool METER, class Commit>
R8B_HD void pcm_row_finish(const PcmLaunch& L, long long f0, int c, int tid, int nthr, Commit commit)
{
	pcm_io_instance(L.fmt, [&](auto fmt) { pcm_row_finish_t<decltype(fmt)::value, DITHER, METER>(L, f0, c, tid, nthr, commit); });
}

// tile, rows -> LDS (lanes walk frames of one channel: nthr is a multiple of the tile's 64 frames, so the 64 lanes of a
// wave hold one channel per step).  All the arithmetic happens here, where a wave can reduce its meters: an integer
// format's samples go into the tile dithered, rounded and saturated (exact as doubles), a float format's as they are.
template<bool DITHER, bool METER, class Commit>
R8B_HD void pcm_finish_gather(const PcmLaunch& L, double* tile, long long f0, int c0, int tid, int nthr, Commit commit)
{
	const double scale = pcm_io_scale(L.fmt);
	const bool dith = DITHER && pcm_io_dithers(L.fmt); // (G.711 rounds at its scale undithered)
	for (int e = tid; e < kPcmTile * kPcmTile; e += nthr)
	{
		const int f = e & (kPcmTile - 1), c = e >> 6;
		PcmMeter m;
		if (f0 + f < L.n && c0 + c < L.nch)
		{
			const double v = L.planar[(long long) (c0 + c) * L.planar_stride + f0 + f];
			double t = v;
			int clipped = fabs(v) > 1.0;
			if (scale != 0.0)
				t = pcm_quantize_dithered(v, scale, dith ? pcm_dither(L.seed, (long long) L.first_channel + c0 + c,
					L.frame0 + f0 + f) : 0.0, &clipped);
			tile[c * kPcmPitch + f] = t;
			if (METER) pcm_meter_note(m, v, clipped);
		}
		if (METER && c0 + c < L.nch) commit(c0 + c, m);
	}
}

// tile -> PCM (lanes walk channels): stores only
R8B_HD void pcm_finish_scatter(const PcmLaunch& L, const double* tile, long long f0, int c0, int tid, int nthr)
{
	unsigned char* dst = static_cast<unsigned char*>(L.pcm);
	const bool quantized = pcm_io_scale(L.fmt) != 0.0;
	for (int e = tid; e < kPcmTile * kPcmTile; e += nthr)
	{
		const int c = e & (kPcmTile - 1), f = e >> 6;
		if (f0 + f < L.n && c0 + c < L.nch)
		{
			unsigned char* const p = dst + pcm_offset(L, f0 + f, c0 + c);
			if (quantized) pcm_io_store_quantized(p, L.fmt, tile[c * kPcmPitch + f]);
			else pcm_encode(p, L.fmt, tile[c * kPcmPitch + f]);
		}
	}
}

} // namespace r8bhip

#endif
