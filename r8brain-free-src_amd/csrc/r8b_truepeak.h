// r8b_truepeak.h -- the 4x-oversampled true-peak meter of the PCM egress (include/r8bsrc.h "true peak"): table and body of
// k_truepeak (r8b_kernels.hip) and of the serial host form of launch_true_peak (r8b_capi.cpp), which runs the phases
// below with tid = 0, nthr = 1.
//
// y[4 j] = x[j - 6]; y[4 j + p] = g[p] x[j], then fma(g[4 t + p], x[j - t], .) for t = 1 .. 11, p = 1, 2, 3; the meter is
// max |y|, NaN skipped.  x is a row of the fp64 staging rows, the values the egress launch beside this one encodes.
//
// Work: a workgroup per (row, tile of kTpTile frames).  The tile lies in LDS behind its 11-frame halo -- the history array
// for a launch's first tile, the row itself for the others -- and in front of 11 + 16 zeros, where the tail of a clip
// that ends in the tile is computed (TruePeakLaunch::clip_len).  A thread takes kTpRun consecutive frames at a time: 19
// LDS reads into a register window feed their 8 x 36 multiply-adds.  Lanes are kTpRun doubles apart, so the tile is laid
// out with one pad double per eight (tp_at): 9 doubles from lane to lane, 32 lanes on 32 different bank pairs.
// History: the workgroup of a row's last tile copies the launch's last 11 frames out of its LDS into hist_out, the OTHER
// of the two arrays the host takes in turn -- hist_in is still being read by the first tile's workgroup.
#ifndef R8B_TRUEPEAK_H
#define R8B_TRUEPEAK_H

#include <cmath>

#include "r8b_launch.h"

// (the host compiler of r8b_capi.cpp does not know the pragma, and its loops run once per frame anyway)
#ifdef __HIPCC__
#define R8B_TP_UNROLL _Pragma("unroll")
#else
#define R8B_TP_UNROLL
#endif

namespace r8bhip {

static const int kTpTaps = 12;            // per phase
static const int kTpHist = kTpTaps - 1;   // frames a y reaches back: the halo, the history, the tail of a clip
static const int kTpRun = 8;              // consecutive frames of a thread
static const int kTpTile = 2048;          // frames of a workgroup: kTpRun for each of 256 threads
// logical doubles of the tile: halo, frames, the tail's zeros, up to the end of the last run's window
static const int kTpSpan = kTpHist + kTpTile + 2 * kTpRun;
static const int kTpLdsDoubles = kTpSpan + (kTpSpan >> 3) + 1;
static_assert(kTpTile % kTpRun == 0 && kTpHist <= 2 * kTpRun && kTpHistStride >= kTpHist, "tile geometry");

R8B_HD int tp_at(int i) { return i + (i >> 3); }

// phase p = 1, 2, 3 is row p - 1: g[4 t + p], t = 0 .. 11 (tools/gen_true_peak.py writes the lines between the markers;
// the committed literals are the definition, tests/golden/true_peak_taps.json holds the same bits)
// BEGIN GENERATED (tools/gen_true_peak.py)
#define R8B_TP_TAPS { \
	{ -0x1.0cae97e5c8338p-12, 0x1.65f2a9f08d31fp-9, -0x1.82ea978435647p-7, 0x1.24cd6e78a45f6p-5, -0x1.7cb7fd56d1fedp-4, 0x1.21cc5555c39f6p-2, 0x1.c9fa05c436cbcp-1, -0x1.38fa93588e7e6p-3, 0x1.db6bf2922add3p-5, -0x1.5af24ccc02b01p-6, 0x1.8be8b3f660813p-8, -0x1.0a4cb91b2e261p-10 }, \
	{ -0x1.96ede21153186p-11, 0x1.7f8f158b8b5ddp-8, -0x1.71b3a399ad34cp-6, 0x1.08bba9867f03bp-4, -0x1.56ca85a59a9c5p-3, 0x1.3d93c82a9a7c9p-1, 0x1.3d93c82a9a7c9p-1, -0x1.56ca85a59a9c5p-3, 0x1.08bba9867f03bp-4, -0x1.71b3a399ad34cp-6, 0x1.7f8f158b8b5ddp-8, -0x1.96ede21153186p-11 }, \
	{ -0x1.0a4cb91b2e261p-10, 0x1.8be8b3f660813p-8, -0x1.5af24ccc02b01p-6, 0x1.db6bf2922add3p-5, -0x1.38fa93588e7e6p-3, 0x1.c9fa05c436cbcp-1, 0x1.21cc5555c39f6p-2, -0x1.7cb7fd56d1fedp-4, 0x1.24cd6e78a45f6p-5, -0x1.82ea978435647p-7, 0x1.65f2a9f08d31fp-9, -0x1.0cae97e5c8338p-12 } }
// END GENERATED

// What a workgroup meters of its tile: the y of local frames [lo, hi) -- past the tile's end by up to 11 where a clip's
// last frame lies in it -- for object channel `chan`
struct TpTile
{
	int lo, hi, chan;
};

// t0: the tile's first frame in the launch
R8B_HD TpTile tp_tile(const TruePeakLaunch& L, int row, long long t0)
{
	TpTile T;
	T.chan = L.clip_chan != nullptr ? (int) L.clip_chan[row] : row;
	const long long left = L.n - t0;
	const int frames = left < kTpTile ? (int) left : kTpTile;
	T.lo = L.skip > t0 ? (L.skip - t0 < frames ? (int) (L.skip - t0) : frames) : 0;
	T.hi = frames;
	if (L.clip_len != nullptr)
	{
		// the clip's last frame, tile-local: before the tile -- the clip has ended, its tail is another workgroup's; in
		// it -- the tail is this one's; behind it -- the whole tile
		const long long last = L.clip_len[row] - 1 - L.frame0 - t0;
		if (last < 0) T.hi = 0;
		else if (last < frames) T.hi = (int) last + 1 + kTpHist;
	}
	return T;
}

// load phase: logical index e is local frame e - 11.  Every load is unconditional, at an index clamped into what exists,
// and what lies outside is zeroed by a select behind it: nine loads of a thread are in flight together, where a branch
// around each would serialise their latencies (measured: profiles/true_peak_ab.txt)
static const int kTpHaloLanes = 256; // the halo's loop runs this far, so that the kernel's 256 threads all take one turn
static_assert(9 * (kTpHaloLanes - 1) + 8 < kTpLdsDoubles, "a pad slot (tp_at never yields 8 mod 9) for every turn");
R8B_HD void tp_load(const TruePeakLaunch& L, double* xs, int row, long long t0, int tid, int nthr)
{
	const double* src = L.rows + (long long) row * L.stride;
	const long long end = L.clip_len != nullptr && L.clip_len[row] - L.frame0 < L.n ? L.clip_len[row] - L.frame0 : L.n;
	// the halo: the history in front of the launch (none: zeros), the row in front of a later tile
	const bool first = t0 == 0, none = first && L.hist_in == nullptr;
	const double* halo = !first ? src + (t0 - kTpHist) : none ? src : L.hist_in + (long long) row * kTpHistStride;
	for (int e = tid; e < kTpHaloLanes; e += nthr)
	{
		const int h = e < kTpHist ? e : kTpHist - 1;
		const double v = halo[none ? 0 : h];
		// (the turns past the halo store into pad slots, which nobody reads: a store under a branch would take the load
		// with it, and its latency would come on top of the tile's)
		xs[e < kTpHist ? tp_at(e) : 9 * e + 8] = none || (!first && t0 - kTpHist + h >= end) ? 0.0 : v;
	}
	// the tile's frames, zeros past the end ...
R8B_TP_UNROLL
	for (int e = tid; e < kTpTile; e += nthr)
	{
		const long long f = t0 + e;
		const double v = src[f < L.n ? f : L.n - 1];
		xs[tp_at(e + kTpHist)] = f < end ? v : 0.0;
	}
	// ... and behind the tile, where only the tail of a clip that ends in it reads
	for (int e = kTpHist + kTpTile + tid; e < kTpSpan; e += nthr) xs[tp_at(e)] = 0.0;
}

// the launch's last 11 frames (or fewer, behind what is left of the old ones) into the other history array; the
// workgroup of the row's last tile, after the load phase
R8B_HD void tp_history(const TruePeakLaunch& L, const double* xs, int row, long long t0, int tid, int nthr)
{
	const int e0 = (int) (L.n - t0); // logical index of frame n - 11
	for (int k = tid; k < kTpHist; k += nthr) L.hist_out[(long long) row * kTpHistStride + k] = xs[tp_at(e0 + k)];
}

// frame i of a run: w[i + 11 - t] is x[j - t]
R8B_HD double tp_frame(const double* w, int i, double m)
{
	constexpr double g[3][kTpTaps] = R8B_TP_TAPS;
	// (fmax returns the other operand for a NaN: skipped)
	m = fmax(m, fabs(w[i + kTpHist - kTpTaps / 2]));
R8B_TP_UNROLL
	for (int p = 0; p < 3; p++)
	{
		double acc = g[p][0] * w[i + kTpHist];
R8B_TP_UNROLL
		for (int t = 1; t < kTpTaps; t++) acc = fma(g[p][t], w[i + kTpHist - t], acc);
		m = fmax(m, fabs(acc));
	}
	return m;
}

// compute phase.  commit(channel, bit pattern of the thread's max |y|): every thread calls it once, at the same place
template<class Commit>
R8B_HD void tp_compute(const TpTile& T, const double* xs, int tid, int nthr, Commit commit)
{
	double m = 0.0;
	for (int r = tid; r * kTpRun < T.hi; r += nthr)
	{
		const int f0 = r * kTpRun;
		if (f0 + kTpRun <= T.lo) continue;
		double w[kTpRun + kTpHist];
R8B_TP_UNROLL
		for (int k = 0; k < kTpRun + kTpHist; k++) w[k] = xs[tp_at(f0 + k)];
		if (f0 >= T.lo && f0 + kTpRun <= T.hi)
		{
R8B_TP_UNROLL
			for (int i = 0; i < kTpRun; i++) m = tp_frame(w, i, m);
		}
		else
		{
R8B_TP_UNROLL
			for (int i = 0; i < kTpRun; i++)
				if (f0 + i >= T.lo && f0 + i < T.hi) m = tp_frame(w, i, m);
		}
	}
	unsigned long long b;
	__builtin_memcpy(&b, &m, 8);
	commit(T.chan, b);
}

} // namespace r8bhip

#endif
