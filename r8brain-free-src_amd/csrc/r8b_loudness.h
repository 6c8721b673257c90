// r8b_loudness.h -- the BS.1770 K-weighted loudness meter of the PCM egress (include/r8bsrc.h "loudness"): body of
// k_loudness (r8b_kernels.hip) and of the serial host form of launch_loudness (r8b_capi.cpp), which runs ld_row below
// with tid = 0, NTHR = 1 and a sync that does nothing.
//
// K-weighting is two biquads, a recurrence; the definition cuts the meter frames into segments of 64 whose start state
// follows a linear hand-off S_{k+1} = Phi S_k + Z_k (Z_k: the segment's final state from zero state), evaluated as a
// stated chain of fmas.  That makes the segments independent but for the hand-off:
//   pass 1   a lane per segment: Z_k, the 64 frames from zero state;
//   walk     one lane: the tile's hand-offs in order, S_k into Z_k's place;
//   pass 2   a lane per segment: z from S_k, and the segment's one or two pieces e = fma(z, z, e) of the sub-blocks it
//            overlaps;
//   add      one lane: the pieces in ascending order into the open sum, which is stored when its sub-block's last frame
//            is in.
// Work: a workgroup of one wave per row walks the row's tiles of 64 segments in order -- the tiles depend on each other
// through S -- so a row is read once.  A tile lies in LDS at a pitch of 65 doubles per segment: lanes are 65 doubles
// apart, 32 lanes on 32 different bank pairs.  The frames a launch runs are the `pending` ones the last launch left
// over (fewer than 64, in `state`) and then the row's; whole segments only, the rest goes back to `state`.
#ifndef R8B_LOUDNESS_H
#define R8B_LOUDNESS_H

#include <cmath>

#include "r8b_launch.h"

// (the host compiler of r8b_capi.cpp does not know the pragma)
#ifdef __HIPCC__
#define R8B_LD_UNROLL(n) _Pragma(#n)
#else
#define R8B_LD_UNROLL(n)
#endif

namespace r8bhip {

static const int kLdSeg = 64;                       // M, frames of a segment
static const int kLdTileSegs = 64;                  // segments of a tile: one per lane
static const int kLdTile = 4096;                    // frames of a tile
static const int kLdPitch = kLdSeg + 1;
static const int kLdPend = 8;                       // where the pending frames begin in a row's state
// the tile, Z_k / S_k of its segments, their two pieces
static const int kLdLdsDoubles = kLdTileSegs * kLdPitch + 4 * kLdTileSegs + 2 * kLdTileSegs;
static_assert(kLdTile == kLdSeg * kLdTileSegs && kLdPend + kLdSeg <= kLdStateStride, "tile geometry");

R8B_HD int ld_at(int e) { return (e >> 6) * kLdPitch + (e & 63); }

// one frame: the shelf on x, the high-pass on the shelf's y (c: LoudnessLaunch::coef); s: p1 q1 p2 q2
R8B_HD double ld_frame(const double* c, double x, double* s)
{
	const double y = fma(c[0], x, s[0]);
	s[0] = fma(-c[3], y, fma(c[1], x, s[1]));
	s[1] = fma(-c[4], y, c[2] * x);
	const double z = fma(c[5], y, s[2]);
	s[2] = fma(-c[8], z, fma(c[6], y, s[3]));
	s[3] = fma(-c[9], z, c[7] * y);
	return z;
}

// S_{k+1} from S_k and Z_k
R8B_HD void ld_handoff(const double* phi, double* s, const double* z)
{
	double n[4];
	for (int i = 0; i < 4; i++)
		n[i] = fma(phi[4 * i + 3], s[3], fma(phi[4 * i + 2], s[2], fma(phi[4 * i + 1], s[1], fma(phi[4 * i], s[0], z[i]))));
	for (int i = 0; i < 4; i++) s[i] = n[i];
}

// a sample whose exponent field is 2047 enters as +0.0
R8B_HD double ld_finite(double x)
{
	unsigned long long b;
	__builtin_memcpy(&b, &x, 8);
	return ((b >> 52) & 0x7ff) == 0x7ff ? 0.0 : x;
}

// one row of a launch.  lds: kLdLdsDoubles doubles of the workgroup; sync(): a barrier of its NTHR threads.  A tile is
// fetched into registers (kLdTile / NTHR doubles of a thread) while the tile before it is computed
template<int NTHR, class Sync>
R8B_HD void ld_row(const LoudnessLaunch& L, double* lds, int row, int tid, Sync sync)
{
	static_assert(kLdTile % NTHR == 0, "every thread fetches the same number of frames");
	const int nthr = NTHR;
	double* const xs = lds;
	double* const zs = lds + kLdTileSegs * kLdPitch;
	double* const es = zs + 4 * kLdTileSegs;
	const double* const src = L.rows + (long long) row * L.stride;
	double* const st = L.state + (long long) row * kLdStateStride;
	const int chan = L.clip_chan != nullptr ? (int) L.clip_chan[row] : row;
	const int p = L.pending, hop = (int) L.hop;
	long long total = p + L.n, nbmax = 0x7fffffffffffffffLL;
	bool finishing = false;
	if (L.clip_len != nullptr)
	{
		// the clip ended before this launch: nothing; its last frame is in it: the last segment filled with zeros
		const long long len = L.clip_len[row];
		if (len <= L.frame0) return;
		nbmax = len / L.hop;
		if (len <= L.frame0 + L.n)
		{
			finishing = true;
			total = len - L.m0;
		}
	}
	const long long segs = finishing ? (total + kLdSeg - 1) / kLdSeg : total / kLdSeg;
	const int rem = finishing ? 0 : (int) (total % kLdSeg);
	const long long tiles = (total + kLdTile - 1) / kLdTile;
	// the walking lane's: S, the open sum and its sub-block, the frames that sub-block still lacks
	double S[4] = { 0.0, 0.0, 0.0, 0.0 }, A = 0.0;
	if (tid == 0 && !L.fresh)
	{
		for (int i = 0; i < 4; i++) S[i] = st[i];
		A = st[4];
	}
	long long b = L.m0 / L.hop;
	int left = (int) ((b + 1) * L.hop - L.m0);
	double* const store = L.sums + (long long) chan * L.capacity;
	// fetch: every load unconditional -- a pending frame from the state, a frame of the row at an index clamped into it --
	// so that all of a thread's loads are in flight together; what does not exist is zeroed when the tile is put into LDS
	double nx[kLdTile / NTHR];
	auto fetch = [&](long long t0)
	{
R8B_LD_UNROLL(unroll)
		for (int u = 0; u < kLdTile / NTHR; u++)
		{
			const long long v = t0 + u * NTHR + tid, i = v - p;
			nx[u] = *(v < p ? st + kLdPend + v : src + (i < L.n ? i : L.n - 1));
		}
	};
	fetch(0);
	for (long long t = 0; t < tiles; t++)
	{
		const long long t0 = t * kLdTile;
R8B_LD_UNROLL(unroll)
		for (int u = 0; u < kLdTile / NTHR; u++)
		{
			const long long v = t0 + u * NTHR + tid;
			xs[ld_at(u * NTHR + tid)] = v < total ? ld_finite(nx[u]) : 0.0;
		}
		sync();
		if (t + 1 < tiles) fetch(t0 + kLdTile);
		// the frames behind the last whole segment: they lie in the last tile
		if (t + 1 == tiles)
			for (int j = tid; j < rem; j += nthr) st[kLdPend + j] = xs[ld_at((int) (segs * kLdSeg - t0) + j)];
		const long long lack = segs - t * kLdTileSegs;
		const int ns = lack < 0 ? 0 : lack < kLdTileSegs ? (int) lack : kLdTileSegs;
		// pass 1
		for (int k = tid; k < ns; k += nthr)
		{
			double s[4] = { 0.0, 0.0, 0.0, 0.0 };
R8B_LD_UNROLL(unroll 8)
			for (int j = 0; j < kLdSeg; j++) ld_frame(L.coef, xs[k * kLdPitch + j], s);
			for (int i = 0; i < 4; i++) zs[4 * k + i] = s[i];
		}
		sync();
		// walk
		if (tid == 0)
			for (int k = 0; k < ns; k++)
			{
				double z[4];
				for (int i = 0; i < 4; i++)
				{
					z[i] = zs[4 * k + i];
					zs[4 * k + i] = S[i];
				}
				ld_handoff(L.phi, S, z);
			}
		sync();
		// pass 2: frames [0, split) of a segment lie in the sub-block its first frame is in, the others in the next
		const int r0 = (int) ((L.m0 + t0) % L.hop);
		for (int k = tid; k < ns; k += nthr)
		{
			double s[4];
			for (int i = 0; i < 4; i++) s[i] = zs[4 * k + i];
			const int r = r0 + k * kLdSeg, split = (r / hop + 1) * hop - r;
			double e = 0.0, e0 = 0.0;
R8B_LD_UNROLL(unroll 8)
			for (int j = 0; j < kLdSeg; j++)
			{
				const double z = ld_frame(L.coef, xs[k * kLdPitch + j], s);
				// (the second piece starts from 0.0 at the sub-block's first frame)
				e0 = j == split ? e : e0;
				e = fma(z, z, j == split ? 0.0 : e);
			}
			es[2 * k] = split < kLdSeg ? e0 : e;
			es[2 * k + 1] = split < kLdSeg ? e : 0.0;
		}
		sync();
		// add
		if (tid == 0)
			for (int k = 0; k < ns; k++)
			{
				A += es[2 * k];
				if (left <= kLdSeg)
				{
					const long long slot = b - L.store0;
					if (b < nbmax && slot >= 0 && slot < L.capacity) store[slot] = A;
					A = 0.0;
					if (left < kLdSeg) A += es[2 * k + 1];
					b++;
					left += hop;
				}
				left -= kLdSeg;
			}
		sync();
	}
	if (tid == 0 && !finishing)
	{
		for (int i = 0; i < 4; i++) st[i] = S[i];
		st[4] = A;
	}
}

} // namespace r8bhip

#endif
