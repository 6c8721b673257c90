// r8b_dispatch.h -- which kernel a fast-path launch runs (launch_convp, launch_convx).  Engine mode and geometry pick the
// instance <LN, UL, MODE, FLENP>; the launch's options promote it to a half-array form, to the eight-elements-per-thread
// form (k_convq) or to the walk form (k_convp_walk); the descriptor is completed (convp_prepare, the workgroup map), grid
// and LDS size are set, and the kernel's symbol is noted for the engine (launch_symbol_note).
// One copy for the device launcher (r8b_kernels.hip) and the CPU emulator (tests/emul/emul_launch.cpp), which include it
// after the kernel headers and differ only in the backend B that runs what was decided:
//   template<int LN, int UL, int MODE, int FLENP, bool WALK> void convp(const ConvxLaunch& X, const LaunchGrid& g);
//   void convq(const ConvxLaunch& X, const LaunchGrid& g);
//   template<int LOGN, int UPLOG, int MODE, int FLENP> void convx(const ConvxLaunch& X, const LaunchGrid& g);
// The geometry lists R8B_CONVP_GEOMS* / R8B_CONVX_GEOMS* (r8b_launch.h, or the compiler's command line) expand here: a
// part object of the device build holds its share of them, and the dispatchers return false for any other geometry.
#ifndef R8B_DISPATCH_H
#define R8B_DISPATCH_H

#include <algorithm>
#include <stdexcept>
#include <string>

namespace r8bhip {

struct LaunchGrid
{
	unsigned grid;  // workgroups
	unsigned npair; // channel pairs of a pair-kernel launch (channels in the one-channel forms)
	size_t lds;     // dynamic LDS bytes
};

// ---- which instances are built ----
// The dispatchers below name one instance per geometry of the lists and mode of their mode lists (Modes*).  The planner
// and the engine ask for fewer: an instance that no chain can launch is not built -- convp_run / convx_run compile no
// kernel for it and refuse it by its symbol.  One rule per line, with what keeps every chain away from it
// (tests/kernel_census.py NOT_BUILT has the same rules at length, instance by instance).
constexpr bool convp_instance_built(int ln, int ul, int mode, int flenp)
{
	const int back = convp_mode(mode).back;
	const int n = 1 << (ul > 0 ? ln + ul : ln); // points of the block's larger transform
	// decimation by 4 exists in the ratio 3/4 alone, behind the 3x zero stuffing, which the kBackEdge3 forms take
	// (Engine::conv_path(): pair_edge3, the kTabSoloDown case's up3 and convx_edge3 come before the plain paths)
	if (ul == -2 && back == kBackConv) return false;
	// ... and not on 64 -> 16 points: a 64-point block takes 32 taps, the shortest quarter-band filter has 35
	// (convp_geometry_ok: decimating by 4 from 128 points)
	if (ul == -2 && ln == 6) return false;
	// a 1:1 convolver in front of an interpolator: In / Out >= 2, a phase pair's windows start 2 or 3 samples apart, which
	// is the 27-tap form (Engine::resolve_forms() kFusedPair2: taps2 == 27 ? kBackWhole2W : kBackWhole2)
	if (ul == 0 && back == kBackWhole2) return false;
	// 64-point blocks have 34 new samples at least: the interpolator's run does not fit the block's part of the array
	// (Engine::fused_form(): pair && g.in_len + 32 > g.n_out)
	if (n == 64 && (back == kBackWhole1 || convp_back_two_phase(back))) return false;
	// 128-point blocks have 96 new samples at most, windows of more than 24 taps ask for 100 (fused_form(): g.in_len < 4 * w.flen)
	if (n == 128 && flenp > 24) return false;
	// ... and 64 at least: the two-phase form's run does not fit (fused_form(): run_fits)
	if (n == 128 && convp_back_two_phase(back)) return false;
	return true;
}
// (the one-channel kernel's MODE is the back end itself)
constexpr bool convx_instance_built(int /*logn*/, int uplog, int mode, int /*flenp*/)
{
	// decimation by 4: the ratio 3/4 alone, as above
	return !(uplog == -2 && mode == kBackConv);
}

// the modes the dispatchers name on a geometry, each with 24-tap windows -- the whole-step modes 1 and 18 beside them,
// with 24-tap or 32-tap windows by the interpolator's length
template<int... MS> struct ModeList {};
using ModesPair = ModeList<0, 3, 6, 7, 4, 5, 16, 17>;           // 1:1 and 2x up-sampling geometries
using ModesLong = ModeList<8, 9, 10, 11, 18, 12, 13, 14, 15>;   // <13, 0>: the split and one-channel forms
using ModesDown = ModeList<0, 3, 6, 7>;                         // decimating geometries
using ModesSoloDown2 = ModeList<10, 11, 14, 15>;                // <13, -1>: the one-channel form
using ModesSoloDown4 = ModeList<10, 11>;                        // <13, -2>: ... real spectra only

#ifndef R8B_DEV_GEOMS
// the rules against the whole lists: they leave out the 57 instances of tests/kernel_census.py NOT_BUILT and no other
// (the polyphase, half-band-front, half-array and walk forms exist only where they run: none of them is left out)
template<int... MS> constexpr int convp_left_out(int ln, int ul, ModeList<MS...>)
{
	return (0 + ... + (convp_instance_built(ln, ul, MS, 24) ? 0 : 1));
}
constexpr int convp_left_out_all()
{
	int n = 0;
#define R8B_COUNT(LN, UL) \
	n += convp_left_out(LN, UL, ModesPair()) + !convp_instance_built(LN, UL, 1, 24) + !convp_instance_built(LN, UL, 1, 32);
	R8B_CONVP_GEOMS(R8B_COUNT) R8B_CONVP_GEOMS_BIG(R8B_COUNT)
#undef R8B_COUNT
	n += convp_left_out(13, 0, ModesLong()) + !convp_instance_built(13, 0, 18, 32);
#define R8B_COUNT(LN, DL) n += convp_left_out(LN, -DL, ModesDown());
	R8B_CONVP_GEOMS_DOWN(R8B_COUNT) R8B_COUNT(6, 2) // (<6, -2>: off the list for good, with its rule)
#undef R8B_COUNT
	return n + convp_left_out(13, -1, ModesSoloDown2()) + convp_left_out(13, -2, ModesSoloDown4());
}
constexpr int convx_left_out_all()
{
	int n = 0;
#define R8B_COUNT(LN, UL) \
	n += !convx_instance_built(LN, UL, kBackConv, 24) + !convx_instance_built(LN, UL, kBackEdge3, 24) + \
		!convx_instance_built(LN, UL, kBackWhole1, 24) + !convx_instance_built(LN, UL, kBackWhole1, 32);
	R8B_CONVX_GEOMS(R8B_COUNT)
#undef R8B_COUNT
#define R8B_COUNT(LN, DL) n += !convx_instance_built(LN, -DL, kBackConv, 24) + !convx_instance_built(LN, -DL, kBackEdge3, 24);
	R8B_CONVX_GEOMS_DOWN(R8B_COUNT)
#undef R8B_COUNT
	return n;
}
static_assert(convp_left_out_all() == 53 && convx_left_out_all() == 4,
	"convp_instance_built / convx_instance_built: a rule is too wide or too narrow");
#endif

// (an unnamed namespace: the bodies below depend on the geometry lists, which differ between the device build's parts)
namespace {

// "k_convp_walk<11, 1, 4, 24>": a kernel template's instance as rocprofv3 names it
inline std::string symbol4(const char* base, int a, int b, int c, int d)
{
	return std::string(base) + "<" + std::to_string(a) + ", " + std::to_string(b) + ", " + std::to_string(c) + ", " +
		std::to_string(d) + ">";
}

// a mode that a geometry's dispatcher does not name: refused (never run as another mode)
inline std::runtime_error mode_not_listed(const char* who, int mode, int ln, int ul)
{
	return std::runtime_error(std::string(who) + ": mode " + std::to_string(mode) + " is not among the modes of geometry <" +
		std::to_string(ln) + ", " + std::to_string(ul) + ">");
}

// the half-array form that stands in for <LN, UL, MODE> (r8b_convp.h cp_ha_*, table: r8b_convp_mode.h), kConvpModeNone: none
template<int LN, int UL, int MODE> constexpr int convp_ha_form()
{
	constexpr bool conv = convp_back_conv(convp_mode(MODE).back), two = convp_back_two_phase(convp_mode(MODE).back);
	// the geometries the form is built for (convp_ha_ok), and the back ends there:
	constexpr bool built =
		// 2048 -> 4096 points -- with the whole-step interpolator fused in: 49 KB, three workgroups per CU, in place of the
		// full-array modes and of their walk form; convolver only: 32 KB, four workgroups per CU
		(LN == 11 && UL == 1 && (conv || two)) ||
		// 4096 -> 8192 points, convolver only: 64 KB, two workgroups of 512 threads
		(LN == 12 && UL == 1 && conv) ||
		// 4096 -> 4096 points, interpolator fused in: both transforms' exchanges by parts (BASELINE's cfg3)
		(LN == 12 && UL == 0 && two) ||
		// 4096 -> 2048 points, convolver only: the FORWARD transform's exchanges by parts
		(LN == 12 && UL == -1 && conv);
	return built ? convp_mode_half_form(MODE, convp_half_of_geometry(UL)) : kConvpModeNone;
}

template<int LN, int UL, int MODE, int FLENP, class B>
void convp_run(const ConvxLaunch& X0, B& b)
{
	if constexpr (!convp_instance_built(LN, UL, MODE, FLENP))
		throw std::runtime_error("launch_convp: " + symbol4("k_convp", LN, UL, MODE, FLENP) + " is not built");
	else
	{
		constexpr int HA = convp_ha_form<LN, UL, MODE>();
		if constexpr (HA != kConvpModeNone)
		{
			// options half_fused (where the interpolator's run fits the half array) and half; with option quad set, the
			// convolver-only forms of the 2x up-sampling geometries with a real kernel spectrum are not taken (k_convq stands in
			// for the full-array convolver of <11, 1>)
			if (convp_mode_ha_fused(HA) ? X0.half_fused != 0 && convp_ha_fused_fits(X0.run_off, X0.c.in_len, X0.in_step) :
				X0.half != 0 && (X0.quad == 0 || UL != 1 || convp_mode(HA).cx))
			{
				convp_run<LN, UL, HA, FLENP>(X0, b);
				return;
			}
		}
		ConvxLaunch X = X0;
		constexpr bool SOLO = convp_mode_solo(MODE);
		constexpr unsigned SUB = ConvpGeom<LN, UL>::SUB;
		const unsigned nbg = ((unsigned) X.c.nblk + SUB - 1u) / SUB;
		LaunchGrid g;
		g.npair = SOLO ? (unsigned) X.c.nch : ((unsigned) X.c.nch + 1u) >> 1;
		g.grid = nbg * g.npair;
		// (one block group: floor(2^32 / 1) + 1 does not fit; 0 makes convp_div return 0, handled by the kernel)
		X.nblk_magic = nbg > 1 ? (unsigned) (0x100000000ull / nbg) + 1u : 0u;
		{
			// convp_div(i, magic) is floor(i / nbg) only while i * nbg < 2^32; i runs up to the grid size (an eighth of it in
			// the XCD-interleaved mapping).  Far out of reach of audio batches -- tens of millions of input samples per call
			// and channel pair --, refused rather than mapped wrongly
			const unsigned long long np = g.npair, imax = (np & 7ull) == 0 ? (np >> 3) * nbg : np * nbg;
			if (nbg > 1 && imax * nbg >= 0x100000000ull)
				throw std::runtime_error("launch_convp: too many blocks per call for the workgroup map (split the call)");
		}
		convp_prepare<LN, UL>(X, convp_mode(MODE).back != kBackWhole1, convp_mode_sp(MODE), SOLO, convp_mode_p3(MODE));
		// (the half-band front stages its raw samples over the array and what lies behind it)
		if constexpr (convp_mode_ha(MODE)) g.lds = (size_t) convp_ha_lds_bytes<LN, UL, MODE>();
		else g.lds = (size_t) std::max(convp_lds_bytes<LN, UL>(), convp_mode_hbf(MODE) ? kHbfLdsBytes : 0);
		if constexpr (LN == 11 && UL == 1 && MODE == convp_mode_find(kLayPair, kBackConv, false))
		{
			// eight elements per thread (r8b_convq.h, option quad): the same work on 512 threads per block pair
			if (X.quad != 0)
			{
				g.lds = (size_t) convq_lds_bytes();
				b.convq(X, g);
				launch_symbol_note("k_convq");
				return;
			}
		}
		if constexpr (convp_walk_ok<LN, UL, MODE>())
		{
			// (X.walk: the engine allows the walk form, at most that many blocks per workgroup; the launch's interior blocks
			// decide whether it is taken: a workgroup per channel pair and slice of them, then one per edge block)
			int i0 = 0, i1 = 0;
			if (X.walk > 0 && convp_walk_range<LN, UL>(X, &i0, &i1) && i1 - i0 >= 2)
			{
				X.walk_i0 = i0;
				X.walk_i1 = i1;
				X.walk_len = std::min(X.walk, i1 - i0);
				const unsigned nwi = (unsigned) (i1 - i0), nslice = (nwi + (unsigned) X.walk_len - 1u) / (unsigned) X.walk_len;
				g.grid = (nslice + (unsigned) X.c.nblk - nwi) * g.npair;
				b.template convp<LN, UL, MODE, FLENP, true>(X, g);
				static const std::string sym = symbol4("k_convp_walk", LN, UL, MODE, FLENP);
				launch_symbol_note(sym.c_str());
				launch_walk_blocks_add((long long) nwi);
				return;
			}
		}
		b.template convp<LN, UL, MODE, FLENP, false>(X, g);
		static const std::string sym = symbol4("k_convp", LN, UL, MODE, FLENP);
		launch_symbol_note(sym.c_str());
	}
}

// runs the first of modes M, MS... that is `mode`; false: none is
template<int LN, int UL, int M, int... MS, class B>
bool convp_mode_in(ModeList<M, MS...>, const ConvxLaunch& X, int mode, B& b)
{
	if (mode == M)
	{
		convp_run<LN, UL, M, 24>(X, b);
		return true;
	}
	if constexpr (sizeof...(MS) > 0) return convp_mode_in<LN, UL>(ModeList<MS...>(), X, mode, b);
	else return false;
}

// a 1:1 or up-sampling geometry: ModesPair, and the mode with one phase per thread (32-tap windows where needed)
template<int LN, int UL, class B>
void convp_modes(const ConvxLaunch& X, int mode, B& b)
{
	if (convp_mode_in<LN, UL>(ModesPair(), X, mode, b)) return;
	if (mode != 1) throw mode_not_listed("launch_convp", mode, LN, UL);
	if (X.flen > 24) convp_run<LN, UL, 1, 32>(X, b);
	else convp_run<LN, UL, 1, 24>(X, b);
}

template<int LN, int UL, class B>
bool convp_geom(const ConvxLaunch& X, int ln, int up, int mode, B& b)
{
	if (ln != LN || up != (1 << UL)) return false;
#ifdef R8B_DEV_ONLY_MODE
	// development build (tools/variant.sh): one mode of the listed geometries only
	if (mode != R8B_DEV_ONLY_MODE) return false;
	convp_run<LN, UL, R8B_DEV_ONLY_MODE, 24>(X, b);
#else
	if (convp_mode_p3(mode))
	{
		// the polyphase 3x form: 1:1 geometries of 1024 ... 4096 points
		if constexpr (UL == 0 && LN >= 10 && LN <= 12) convp_run<LN, UL, 19, 24>(X, b);
		else throw std::runtime_error("launch_convp: polyphase 3x form on a geometry it is not built for");
	}
	else convp_modes<LN, UL>(X, mode, b);
#endif
	return true;
}

// 8192-point blocks (512-thread workgroups).  The 1:1 geometry also carries the split 2x up-sampling form (modes 8 / 9 /
// 12 / 13, r8b_convp.h cp_sp_*) and the one-channel form (modes 10 / 11 / 14 / 15 / 18, cp_solo_*: 16384-point blocks)
template<int LN, int UL, class B>
bool convp_big(const ConvxLaunch& X, int ln, int up, int mode, B& b)
{
	if constexpr (LN == 13 && UL == 0)
	{
		if ((ln == 13 && convp_mode_sp(mode)) || (ln == 14 && convp_mode_solo(mode)))
		{
			if (convp_mode(mode).back == kBackWhole1 && X.flen > 24) convp_run<LN, UL, 18, 32>(X, b);
			else if (!convp_mode_in<LN, UL>(ModesLong(), X, mode, b)) throw mode_not_listed("launch_convp", mode, LN, UL);
			return true;
		}
	}
	if (ln != LN || up != (1 << UL) || !convp_mode_pair_full(mode)) return false;
	convp_modes<LN, UL>(X, mode, b);
	return true;
}

// the decimating form <LN, -DL>; behind <13, -DL> also the one-channel form decimating by 2 / 4 (16384-point blocks)
template<int LN, int DL, class B>
bool convp_down(const ConvxLaunch& X, int ln, int mode, B& b)
{
	if (X.c.down != (1 << DL)) return false;
	if constexpr (LN == 13 && DL == 1)
	{
		if (ln == 14 && convp_mode_solo(mode))
		{
			if (!convp_mode_in<LN, -DL>(ModesSoloDown2(), X, mode, b)) throw mode_not_listed("launch_convp", mode, LN, -DL);
			return true;
		}
	}
	// (decimating by 4: real spectra only)
	if constexpr (LN == 13 && DL == 2)
	{
		if (ln == 14 && convp_mode_solo(mode))
		{
			if (!convp_mode_in<LN, -DL>(ModesSoloDown4(), X, mode, b)) throw mode_not_listed("launch_convp", mode, LN, -DL);
			return true;
		}
	}
	if (ln != LN) return false;
	if (convp_mode_hbf(mode))
	{
		// the half-band front: the 4096 -> 2048-point geometry
		if constexpr (LN == 12 && DL == 1) convp_run<LN, -DL, 20, 24>(X, b);
		else throw std::runtime_error("launch_convp: half-band front on a geometry it is not built for");
		return true;
	}
	if (!convp_mode_pair_full(mode) || !convp_back_conv(convp_mode(mode).back)) return false;
	if (!convp_mode_in<LN, -DL>(ModesDown(), X, mode, b)) throw mode_not_listed("launch_convp", mode, LN, -DL);
	return true;
}

// launch_convp over the geometries of the lists; false: none of them is the launch's
template<class B>
bool convp_dispatch(const ConvxLaunch& X, int mode, B& b)
{
	int ln = 0;
	while ((1 << ln) < X.c.n_in) ln++;
	[[maybe_unused]] const int up = X.c.up_pow2 ? X.c.up : 1; // (mode 3: a 3x zero-stuffed input is 1:1 for the transforms)
	if (X.c.down_pow2 && X.c.down > 1)
	{
#define R8B_CONVP_TRY(LN, DL) if (convp_down<LN, DL>(X, ln, mode, b)) return true;
		R8B_CONVP_GEOMS_DOWN(R8B_CONVP_TRY)
#undef R8B_CONVP_TRY
		return false;
	}
#define R8B_CONVP_TRY(LN, UL) if (convp_big<LN, UL>(X, ln, up, mode, b)) return true;
	R8B_CONVP_GEOMS_BIG(R8B_CONVP_TRY)
#undef R8B_CONVP_TRY
#define R8B_CONVP_TRY(LN, UL) if (convp_geom<LN, UL>(X, ln, up, mode, b)) return true;
	R8B_CONVP_GEOMS(R8B_CONVP_TRY)
#undef R8B_CONVP_TRY
	return false;
}

// ... where every geometry is at hand (the one-object build, the emulator): `who` names the launcher in the message
template<class B>
void convp_dispatch_all(const ConvxLaunch& X, int mode, B& b, const char* who)
{
	if (convp_dispatch(X, mode, b)) return;
	if (X.c.down_pow2 && X.c.down > 1) throw std::runtime_error("launch_convp: decimating geometry not instantiated");
	throw std::runtime_error(std::string(who) + ": geometry not instantiated");
}

template<int LOGN, int UPLOG, int MODE, int FLENP, class B>
void convx_run(const ConvxLaunch& X, B& b)
{
	if constexpr (!convx_instance_built(LOGN, UPLOG, MODE, FLENP))
		throw std::runtime_error("launch_convx: " + symbol4("k_convx", LOGN, UPLOG, MODE, FLENP) + " is not built");
	else
	{
		LaunchGrid g;
		g.npair = 0;
		g.grid = (unsigned) X.c.nblk * (unsigned) X.c.nch;
		// work array; the linear output run (in_len + kConvxRunPad doubles) aliases its start
		g.lds = (size_t) convx_lds_need(UPLOG > 0 ? LOGN + UPLOG : LOGN, X.c.in_len, MODE) * sizeof(double);
		b.template convx<LOGN, UPLOG, MODE, FLENP>(X, g);
		static const std::string sym = symbol4("k_convx", LOGN, UPLOG, MODE, FLENP);
		launch_symbol_note(sym.c_str());
	}
}

// launch_convx over the geometries of the lists; false: none of them is the launch's
template<class B>
bool convx_dispatch(const ConvxLaunch& X, int mode, B& b)
{
	int logn = 0;
	while ((2 << logn) < X.c.n_in) logn++;
	// mode 3: a 3x zero-stuffed input / 3x strided output is 1:1 as far as the transforms go
	[[maybe_unused]] const int up = X.c.up_pow2 ? X.c.up : 1;
#define R8B_CONVX_TRY(LN, DL) \
	if (logn == LN && X.c.down == (1 << DL)) \
	{ \
		if (mode == kBackEdge3) convx_run<LN, -DL, kBackEdge3, 24>(X, b); \
		else if (mode == kBackConv) convx_run<LN, -DL, kBackConv, 24>(X, b); \
		else throw mode_not_listed("launch_convx", mode, LN, -DL); \
		return true; \
	}
	if (X.c.down_pow2 && X.c.down > 1)
	{
		R8B_CONVX_GEOMS_DOWN(R8B_CONVX_TRY)
	}
#undef R8B_CONVX_TRY
#define R8B_CONVX_TRY(LN, UL) \
	if (logn == LN && up == (1 << UL)) \
	{ \
		if (mode == kBackConv) convx_run<LN, UL, kBackConv, 24>(X, b); \
		else if (mode == kBackEdge3) convx_run<LN, UL, kBackEdge3, 24>(X, b); \
		else if (mode != kBackWhole1) throw mode_not_listed("launch_convx", mode, LN, UL); \
		else if (X.flen > 24) convx_run<LN, UL, kBackWhole1, 32>(X, b); \
		else convx_run<LN, UL, kBackWhole1, 24>(X, b); \
		return true; \
	}
	R8B_CONVX_GEOMS(R8B_CONVX_TRY)
#undef R8B_CONVX_TRY
	return false;
}

} // namespace
} // namespace r8bhip

#endif
