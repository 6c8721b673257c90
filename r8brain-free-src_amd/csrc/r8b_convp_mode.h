// r8b_convp_mode.h -- what the pair kernel's template parameter MODE means (k_convp, k_convp_walk, convp_body: r8b_convp.h).
// MODE is a plain number -- it is part of every kernel symbol, "k_convp<11, 1, 23, 24>" -- that stands for five
// independent choices.  The table below is the ONLY place where they are tied to numbers: kernels, launcher, engine and
// emulator read it (at compile time wherever MODE is a template argument) and name what they mean.  A new form is one
// line here plus its code.  Plain constexpr C++: included by host and device translation units alike.
#ifndef R8B_CONVP_MODE_H
#define R8B_CONVP_MODE_H

namespace r8bhip {

// layout: what a workgroup's block is
constexpr int kLayPair = 0;  // two channels in one complex transform (every geometry)
constexpr int kLaySplit = 1; // split 2x up-sampling form (cp_sp_*; 8192 -> 16384 points on geometry <13, 0>)
constexpr int kLaySolo = 2;  // one-channel form (cp_solo_*; 16384-point blocks on geometries <13, 0>, <13, -1>, <13, -2>)
constexpr int kLayP3 = 3;    // polyphase 3x form (cp_p3_*; geometries <10, 0> ... <12, 0>)
constexpr int kLayHbf = 4;   // pair behind a half-band decimator taken in the load (cp_hbf_*; geometry <12, -1>)

// back end: what the block does behind its backward transform (k_convx's MODE takes the first three)
constexpr int kBackConv = 0;    // convolver only: from the registers to the destination
constexpr int kBackWhole1 = 1;  // whole-step interpolator fused in, one phase per thread
constexpr int kBackEdge3 = 3;   // convolver only, behind a 3x zero-stuffing load and / or in front of a 3x strided store
constexpr int kBackWhole2 = 4;  // whole-step interpolator fused in, two phases per thread, 25-tap windows
constexpr int kBackWhole2W = 5; // ... adjacent windows up to three samples apart (In > Out): 27-tap windows
constexpr bool convp_back_conv(int back) { return back == kBackConv || back == kBackEdge3; }
constexpr bool convp_back_two_phase(int back) { return back == kBackWhole2 || back == kBackWhole2W; }

// half-array form (cp_ha_*): which transform's exchanges go by parts through an array of doubles.  The geometry decides
// (convp_half_of_geometry): the side with more points than the other, both where they are equal
constexpr int kHalfNone = 0, kHalfBack = 1, kHalfFwd = 2, kHalfBoth = 3;
constexpr int convp_half_of_geometry(int ul) { return ul > 0 ? kHalfBack : (ul < 0 ? kHalfFwd : kHalfBoth); }

constexpr int kConvpModeNone = -1, kConvpModeEnd = 34;

struct ConvpMode
{
	int layout;
	int back;
	bool cx;  // complex kernel spectrum (minimum phase, or an alignment moved by inherited latency)
	int half;
	int full; // a half-array form: the full-array mode it stands in for (same layout, back end and spectrum)
};

constexpr ConvpMode convp_mode(int m)
{
	constexpr int none = kConvpModeNone;
	switch (m)
	{
	case 0: return {kLayPair, kBackConv, false, kHalfNone, none};
	case 1: return {kLayPair, kBackWhole1, false, kHalfNone, none};
	case 3: return {kLayPair, kBackEdge3, false, kHalfNone, none};
	case 4: return {kLayPair, kBackWhole2, false, kHalfNone, none};
	case 5: return {kLayPair, kBackWhole2W, false, kHalfNone, none};
	case 6: return {kLayPair, kBackConv, true, kHalfNone, none};
	case 7: return {kLayPair, kBackEdge3, true, kHalfNone, none};
	case 8: return {kLaySplit, kBackConv, false, kHalfNone, none};
	case 9: return {kLaySplit, kBackEdge3, false, kHalfNone, none};
	case 10: return {kLaySolo, kBackConv, false, kHalfNone, none};
	case 11: return {kLaySolo, kBackEdge3, false, kHalfNone, none};
	case 12: return {kLaySplit, kBackConv, true, kHalfNone, none};
	case 13: return {kLaySplit, kBackEdge3, true, kHalfNone, none};
	case 14: return {kLaySolo, kBackConv, true, kHalfNone, none};
	case 15: return {kLaySolo, kBackEdge3, true, kHalfNone, none};
	case 16: return {kLayPair, kBackWhole2, true, kHalfNone, none};
	case 17: return {kLayPair, kBackWhole2W, true, kHalfNone, none};
	case 18: return {kLaySolo, kBackWhole1, false, kHalfNone, none};  // (cp_solo_final_store / cp_whole_compute_solo)
	case 19: return {kLayP3, kBackConv, false, kHalfNone, none};
	case 20: return {kLayHbf, kBackConv, false, kHalfNone, none};
	// half-array forms.  Convolver only -- 2048 / 4096 -> 2x points: 32 KB, four workgroups per CU (8192 points: 64 KB, two
	// of 512 threads):
	case 21: return {kLayPair, kBackConv, false, kHalfBack, 0};
	case 22: return {kLayPair, kBackEdge3, false, kHalfBack, 3};
	// ... the interpolator fused in -- 2048 -> 4096 points: the array is what the interpolator's run of (A, B) pairs needs
	// (kHaFusedElems), its first 32 KB carry the transforms; three workgroups per CU:
	case 23: return {kLayPair, kBackWhole2, false, kHalfBack, 4};
	case 25: return {kLayPair, kBackWhole2W, false, kHalfBack, 5};
	// ... the 4096 -> 2048-point DECIMATING geometry: the forward transform's two exchanges go by parts through 4096
	// doubles, the backward side's 2048 complex values fit as they are; three workgroups per CU:
	case 27: return {kLayPair, kBackConv, false, kHalfFwd, 0};
	case 28: return {kLayPair, kBackEdge3, false, kHalfFwd, 3};
	// ... 23 / 25 / 21 / 22 with a complex kernel spectrum (minimum-phase chains):
	case 29: return {kLayPair, kBackWhole2, true, kHalfBack, 16};
	case 30: return {kLayPair, kBackWhole2W, true, kHalfBack, 17};
	case 31: return {kLayPair, kBackConv, true, kHalfBack, 6};
	case 32: return {kLayPair, kBackEdge3, true, kHalfBack, 7};
	// ... the 4096 -> 4096-point 1:1 geometry (BASELINE's cfg3): all four exchanges by parts, two of them across the
	// workgroup; the array is the interpolator's run as in mode 25:
	case 33: return {kLayPair, kBackWhole2W, false, kHalfBoth, 5};
	default: return {none, none, false, kHalfNone, none}; // (2, 24, 26: unused)
	}
}
constexpr bool convp_mode_exists(int m) { return convp_mode(m).layout != kConvpModeNone; }

// the inverse; kConvpModeNone: no such mode
constexpr int convp_mode_find(int layout, int back, bool cx, int half = kHalfNone)
{
	for (int m = 0; m < kConvpModeEnd; m++)
	{
		const ConvpMode d = convp_mode(m);
		if (d.layout == layout && d.back == back && d.cx == cx && d.half == half) return m;
	}
	return kConvpModeNone;
}

// the half-array form whose exchanges go by parts on side `half` and that stands in for full-array mode m
constexpr int convp_mode_half_form(int m, int half)
{
	for (int h = 0; h < kConvpModeEnd; h++)
		if (convp_mode(h).half == half && convp_mode(h).full == m) return h;
	return kConvpModeNone;
}

// one-line readers
// (the pair layout on its full array: what the engine asks for on any geometry)
constexpr bool convp_mode_pair_full(int m) { return convp_mode(m).layout == kLayPair && convp_mode(m).half == kHalfNone; }
constexpr bool convp_mode_p3(int m) { return convp_mode(m).layout == kLayP3; }
constexpr bool convp_mode_sp(int m) { return convp_mode(m).layout == kLaySplit; }
constexpr bool convp_mode_solo(int m) { return convp_mode(m).layout == kLaySolo; }
constexpr bool convp_mode_hbf(int m) { return convp_mode(m).layout == kLayHbf; }
constexpr bool convp_mode_ha(int m) { return convp_mode(m).half != kHalfNone; }
constexpr bool convp_mode_ha_down(int m) { return convp_mode(m).half == kHalfFwd; }
constexpr bool convp_mode_ha_fused(int m) { return convp_mode_ha(m) && convp_back_two_phase(convp_mode(m).back); }

// the table against itself: find() inverts it; a half-array mode stands in for an existing full-array mode of its own
// layout, back end and spectrum
constexpr bool convp_mode_table_ok()
{
	for (int m = -1; m <= kConvpModeEnd; m++)
	{
		const ConvpMode d = convp_mode(m);
		if (!convp_mode_exists(m)) continue;
		if (m >= kConvpModeEnd || convp_mode_find(d.layout, d.back, d.cx, d.half) != m) return false;
		if ((d.half != kHalfNone) != (d.full != kConvpModeNone)) return false;
		if (d.half != kHalfNone && (d.full != convp_mode_find(d.layout, d.back, d.cx) || convp_mode_half_form(d.full, d.half) != m))
			return false;
	}
	return true;
}
static_assert(convp_mode_table_ok(), "pair kernel modes: the table contradicts itself");
static_assert(!convp_mode_exists(2) && !convp_mode_exists(24) && !convp_mode_exists(26) && convp_mode_exists(33), "pair kernel modes");

} // namespace r8bhip

#endif
