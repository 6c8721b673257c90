// tests/emul/emul_pcm.cpp -- TEST INFRASTRUCTURE ONLY, the PCM boundary of the host emulation (emul_launch.cpp, whose
// opening comment holds for this file too; an object of its own for the build's sake): the stand-in of launch_pcm_in /
// launch_pcm_out as r8b_kernels.hip has them.  Which form a PcmLaunch runs -- plain, finishing or clip; rows or tiles;
// strided, packed or scheduled; dither and meters -- it decides with the launcher's own r8b_pcm_dispatch.h.
#include <limits>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#define R8B_HD inline
#define R8B_LDS_WINDOW(N, v, p) { for (int i_ = 0; i_ < (N); i_++) (v)[i_] = (p)[i_]; }
#define R8B_LDS_ARRIVED(N, v, o)
#include "r8b_clip_sched.h"
#include "r8b_pcm_dispatch.h"

namespace r8bhip {

// The emulator backend of r8b_pcm_dispatch.h: every form of the PCM boundary (r8b_pcm.h, r8b_clip*.h).  A workgroup is
// the kernel's very phases run for tid = 0 .. 255 one after the other, the barrier being the end of a loop over the
// threads.
struct EmulPcm
{
	// the stand-in for the wave reduction and the atomics of the kernels' PcmMeterCommit: every thread's record is folded
	// into the channel's meters as it comes
	struct Commit
	{
		const PcmLaunch& L;
		void operator()(int ch, const PcmMeter& m) const
		{
			if (m.peak > L.m_peak[ch]) L.m_peak[ch] = m.peak;
			L.m_clipped[ch] += m.clipped;
			L.m_nonfinite[ch] += m.nonfinite;
		}
	};

	// the device symbol of the form a member stands in for, as DevPcm::start notes it (r8b_kernels.hip)
	static void note(const std::string& sym) { launch_symbol_note(sym.c_str()); }
#define R8B_EMUL_NOTE(...) \
	{ \
		static const std::string sym = pcm_symbol(__VA_ARGS__); \
		note(sym); \
	}

	// a row kernel: phase(f0, row, tid), a workgroup per chunk of a row
	template<class F>
	static void rows(const PcmGrid& g, F phase)
	{
		for (unsigned y = 0; y < g.y; y++)
			for (unsigned x = 0; x < g.x; x++)
				for (int t = 0; t < 256; t++) phase((long long) x * kPcmRowChunk, (int) y, t);
	}

	// a two-phase tile kernel, a workgroup per tile of 1 << lg frames: where live(f0, y) holds (the kernels' test in front
	// of their barrier), first(tile, f0, y, tid), the barrier, second(tile, f0, y, tid) -- on a tile of `doubles` that is
	// NaN wherever a phase must not read before it has written
	template<class Live, class F1, class F2>
	static void tiles(const PcmGrid& g, int lg, size_t doubles, Live live, F1 first, F2 second)
	{
		for (unsigned y = 0; y < g.y; y++)
			for (unsigned x = 0; x < g.x; x++)
			{
				const long long f0 = (long long) x << lg;
				if (!live(f0, (int) y)) continue;
				std::vector<double> tile(doubles, std::numeric_limits<double>::quiet_NaN());
				for (int t = 0; t < 256; t++) first(tile.data(), f0, (int) y, t);
				for (int t = 0; t < 256; t++) second(tile.data(), f0, (int) y, t);
			}
	}
	static bool all_live(long long, int) { return true; }

	// the plain and the finishing tiles: kPcmTile frames by kPcmTile channels
	template<class F1, class F2>
	static void pcm_tiles(const PcmGrid& g, F1 first, F2 second)
	{
		static_assert(kPcmTile == 1 << 6, "the tile's frames as a shift");
		tiles(g, 6, (size_t) kPcmTile * kPcmPitch, all_live,
			[&](double* tile, long long f0, int y, int t) { first(tile, f0, y * kPcmTile, t); },
			[&](double* tile, long long f0, int y, int t) { second(tile, f0, y * kPcmTile, t); });
	}

	// the clip tiles: Kt rows of (1 << lg) + pad doubles, as the kernels work them out; the phases get lg and pitch too
	template<class Live, class F1, class F2>
	static void clip_tiles(const PcmGrid& g, int Kt, int lanes, Live live, F1 first, F2 second)
	{
		const int lg = clip_tile_log2(Kt), pitch = (1 << lg) + clip_tile_pad(Kt, lanes);
		// (this backend's own buffer, the largest tile's: the device launcher asks for g.lds bytes of LDS)
		if (g.lds > kClipTileDoubles * sizeof(double)) throw std::logic_error("emul launch_pcm: the tile exceeds kClipTileDoubles");
		tiles(g, lg, kClipTileDoubles, live,
			[&](double* tile, long long f0, int y, int t) { first(tile, lg, pitch, f0, y, t); },
			[&](double* tile, long long f0, int y, int t) { second(tile, lg, pitch, f0, y, t); });
	}

	void pcm_rows_in(const PcmLaunch& L, const PcmGrid& g)
	{
		R8B_EMUL_NOTE("k_pcm_rows_in")
		rows(g, [&](long long f0, int c, int t) { pcm_row_in(L, f0, c, t, 256); });
	}
	void pcm_rows_out(const PcmLaunch& L, const PcmGrid& g)
	{
		R8B_EMUL_NOTE("k_pcm_rows_out")
		rows(g, [&](long long f0, int c, int t) { pcm_row_out(L, f0, c, t, 256); });
	}
	void pcm_in(const PcmLaunch& L, const PcmGrid& g)
	{
		R8B_EMUL_NOTE("k_pcm_in")
		pcm_tiles(g, [&](double* tile, long long f0, int c0, int t) { pcm_in_gather(L, tile, f0, c0, t, 256); },
			[&](double* tile, long long f0, int c0, int t) { pcm_in_scatter(L, tile, f0, c0, t, 256); });
	}
	void pcm_out(const PcmLaunch& L, const PcmGrid& g)
	{
		R8B_EMUL_NOTE("k_pcm_out")
		pcm_tiles(g, [&](double* tile, long long f0, int c0, int t) { pcm_out_gather(L, tile, f0, c0, t, 256); },
			[&](double* tile, long long f0, int c0, int t) { pcm_out_scatter(L, tile, f0, c0, t, 256); });
	}
	template<bool DITHER, bool METER>
	void pcm_rows_finish(const PcmLaunch& L, const PcmGrid& g)
	{
		R8B_EMUL_NOTE("k_pcm_rows_finish", {DITHER, METER})
		rows(g, [&](long long f0, int c, int t) { pcm_row_finish<DITHER, METER>(L, f0, c, t, 256, Commit{L}); });
	}
	template<bool DITHER, bool METER>
	void pcm_finish(const PcmLaunch& L, const PcmGrid& g)
	{
		R8B_EMUL_NOTE("k_pcm_finish", {DITHER, METER})
		pcm_tiles(g,
			[&](double* tile, long long f0, int c0, int t) { pcm_finish_gather<DITHER, METER>(L, tile, f0, c0, t, 256, Commit{L}); },
			[&](double* tile, long long f0, int c0, int t) { pcm_finish_scatter(L, tile, f0, c0, t, 256); });
	}

	template<class Base>
	void clip_rows_in(const PcmLaunch& L, const PcmGrid& g)
	{
		if constexpr (std::is_same<Base, ClipPacked>::value) R8B_EMUL_NOTE("k_clip_packed_rows_in")
		else R8B_EMUL_NOTE("k_clip_rows_in")
		rows(g, [&](long long f0, int c, int t)
		{
			if constexpr (std::is_same<Base, ClipPacked>::value) clip_packed_row_in(L, f0, c, t, 256);
			else clip_row_in(L, f0, c, t, 256);
		});
	}
	template<class Base>
	void clip_frames_in(const PcmLaunch& L, const PcmGrid& g)
	{
		if constexpr (std::is_same<Base, ClipPacked>::value) R8B_EMUL_NOTE("k_clip_packed_frames_in")
		else R8B_EMUL_NOTE("k_clip_frames_in")
		clip_tiles(g, L.clip_channels, kClipLanesIn, all_live,
			[&](double* tile, int lg, int pitch, long long f0, int clip, int t)
			{
				if constexpr (std::is_same<Base, ClipPacked>::value) clip_packed_frames_in_load(L, tile, lg, pitch, f0, clip, t, 256);
				else clip_frames_in_load(L, tile, lg, pitch, f0, clip, t, 256);
			},
			[&](double* tile, int lg, int pitch, long long f0, int clip, int t) { clip_frames_in_store(L, tile, lg, pitch, f0, clip, t, 256); });
	}
	template<class Base>
	void clip_mix_in(const PcmLaunch& L, const PcmGrid& g)
	{
		if constexpr (std::is_same<Base, ClipPacked>::value) R8B_EMUL_NOTE("k_clip_packed_mix_in")
		else R8B_EMUL_NOTE("k_clip_mix_in")
		clip_tiles(g, L.mix_channels, kClipLanesIn, all_live,
			[&](double* tile, int lg, int pitch, long long f0, int clip, int t)
			{
				if constexpr (std::is_same<Base, ClipPacked>::value) clip_packed_mix_load(L, tile, lg, pitch, f0, clip, t, 256);
				else clip_mix_load(L, tile, lg, pitch, f0, clip, t, 256);
			},
			[&](double* tile, int lg, int pitch, long long f0, int clip, int t) { clip_mix_store(L, tile, lg, pitch, f0, clip, t, 256); });
	}
	template<class Base, bool PAD, bool DITHER, bool METER>
	void clip_rows_out(const PcmLaunch& L, const PcmGrid& g)
	{
		if constexpr (std::is_same<Base, ClipSched>::value) R8B_EMUL_NOTE("k_clip_sched_rows_out", {DITHER, METER, PAD})
		else if constexpr (std::is_same<Base, ClipPacked>::value) R8B_EMUL_NOTE("k_clip_packed_rows_out", {DITHER, METER})
		else R8B_EMUL_NOTE("k_clip_rows_out", {DITHER, METER})
		rows(g, [&](long long f0, int c, int t)
		{
			if constexpr (std::is_same<Base, ClipSched>::value) clip_sched_row_out<DITHER, METER, PAD>(L, f0, c, t, 256, Commit{L});
			else if constexpr (std::is_same<Base, ClipPacked>::value) clip_packed_row_out<DITHER, METER>(L, f0, c, t, 256, Commit{L});
			else clip_row_out<DITHER, METER>(L, f0, c, t, 256, Commit{L});
		});
	}
	template<class Base, bool PAD, bool DITHER, bool METER>
	void clip_frames_out(const PcmLaunch& L, const PcmGrid& g)
	{
		if constexpr (std::is_same<Base, ClipSched>::value) R8B_EMUL_NOTE("k_clip_sched_frames_out", {DITHER, METER, PAD})
		else if constexpr (std::is_same<Base, ClipPacked>::value) R8B_EMUL_NOTE("k_clip_packed_frames_out", {DITHER, METER})
		else R8B_EMUL_NOTE("k_clip_frames_out", {DITHER, METER})
		clip_tiles(g, L.clip_channels, kClipLanesOut,
			[&](long long f0, int clip)
			{
				if constexpr (std::is_same<Base, ClipSched>::value) return clip_sched_frames_out_live<PAD>(L, f0, clip);
				else if constexpr (std::is_same<Base, ClipPacked>::value) return clip_packed_frames_out_live(L, f0, clip);
				else return true;
			},
			[&](double* tile, int lg, int pitch, long long f0, int clip, int t)
			{
				if constexpr (std::is_same<Base, ClipSched>::value)
					clip_sched_frames_out_gather<DITHER, METER>(L, tile, lg, pitch, f0, clip, t, 256, Commit{L});
				else clip_frames_out_gather<DITHER, METER>(L, tile, lg, pitch, f0, clip, t, 256, Commit{L});
			},
			[&](double* tile, int lg, int pitch, long long f0, int clip, int t)
			{
				if constexpr (std::is_same<Base, ClipSched>::value) clip_sched_frames_out_store<PAD>(L, tile, lg, pitch, f0, clip, t, 256);
				else if constexpr (std::is_same<Base, ClipPacked>::value) clip_packed_frames_out_store(L, tile, lg, pitch, f0, clip, t, 256);
				else clip_frames_out_store(L, tile, lg, pitch, f0, clip, t, 256);
			});
	}
};
#undef R8B_EMUL_NOTE

void launch_pcm_in(const PcmLaunch& L, void*)
{
	EmulPcm b;
	pcm_in_dispatch(L, b);
}

void launch_pcm_out(const PcmLaunch& L, void*)
{
	EmulPcm b;
	pcm_out_dispatch(L, b);
}

} // namespace r8bhip
