// r8b_engine.cpp -- see r8b_engine.h.  Host C++ only; every device operation goes through
// r8b_launch.h.
#include "r8b_engine.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <optional>
#include <stdexcept>

#include "r8b_conv_tables.h"

namespace r8bhip {

// LDS of the fast path: one padded complex array of n elements (r8b_convx.h, convx_lds_doubles)
static size_t convx_work_bytes(int n) { return (size_t) 2 * (n + (n >> 4)) * sizeof(double); }

// LDS of the generic convolver kernel: forward and backward arrays side by side; transforms of
// equal length can share one array (each spectral slot rewrites exactly the two bins it read)
static bool generic_conv_two_arrays(const ConvGeom& g)
{
	return (size_t) (g.n_in + g.n_out) * sizeof(double) <= 160 * 1024;
}
static bool generic_conv_fits(const ConvGeom& g)
{
	return generic_conv_two_arrays(g) ||
		(g.n_in == g.n_out && (size_t) g.n_in * sizeof(double) <= 160 * 1024);
}
// ... blocks of the reference's own length where the plan keeps them although the forward array does not fit (2^k
// decimation in the spectrum on 32768-point blocks, r8b_plan.cpp): the forward transform in two halves through LDS
// (k_conv_big)
static bool generic_conv_big(const ConvGeom& g)
{
	return !generic_conv_fits(g) && g.down_pow2 && g.down > 1 && g.n_in <= 32768 &&
		(size_t) g.n_out * sizeof(double) <= 128 * 1024;
}

// LDS row pitch of the tiled polynomial interpolator (doubles).  Lanes 0..15 and 16..31 of an LDS lane group
// read the windows of 16 consecutive outputs (input offsets floor(o * step + phase)) in two ADJACENT channel
// rows; banks repeat every 32 doubles, so the pitch's residue mod 32 decides whether the two rows' slots
// interleave (step 2: any odd residue) or collide.  Chosen by counting, for the step at hand.
static int poly_row_pitch(int span_max, double step)
{
	if (span_max <= 0) return 0;
	int best = 1;
	long best_cost = -1;
	for (int P = 0; P < 32; P++)
	{
		long cost = 0;
		for (int ph = 0; ph < 8; ph++)
		{
			int cnt[32] = { 0 };
			for (int o = 0; o < 16; o++)
			{
				const int xo = (int) std::floor(o * step + ph / 8.0);
				cnt[xo & 31]++;
				cnt[(xo + P) & 31]++;
			}
			int mx = 0;
			for (int i = 0; i < 32; i++) mx = std::max(mx, cnt[i]);
			cost += mx;
		}
		if (best_cost < 0 || cost < best_cost)
		{
			best_cost = cost;
			best = P;
		}
	}
	int pitch = span_max;
	while ((pitch & 31) != best) pitch++;
	return pitch;
}

static long long pow2_at_least(long long v)
{
	long long p = 1;
	while (p < v) p <<= 1;
	return p;
}

// taps of a half-band filter rounded up to the unrolled widths of the kernels (extra taps are zero): 4, 8 or 14 --
// kHbfTapsMax (r8b_launch.h) is 14, the widest, which launch_conv_stage's front names
static_assert(kHbfTapsMax == 14, "the widest half-band kernel takes kHbfTapsMax taps");
static int hb_tap_width(int n) { return n <= 4 ? 4 : (n <= 8 ? 8 : 14); }

Engine::Engine(const std::vector<StageDesc>& descs, int maxin, int nch, int device)
	: nch_(nch), nchw_(nch), act_(nch), act_min_(nch), device_(dev_resolve(device)), dev_(device_)
{
	if (nch < 1) throw std::runtime_error("channel count must be >= 1");
	if (nch > 65535) throw std::runtime_error("channel count must be <= 65535 per batch object "
		"(grid y dimension); split larger batches");
	if (maxin < 1) throw std::runtime_error("MaxInLen must be >= 1");
	// (a throw from here on leaks nothing: what is on the device by then belongs to dev_, whose destructor makes the
	// device current again by itself -- this guard is gone by then)
	DevGuard guard(device_);
	plan_.init(descs, maxin);
	for (int o = 0; o < kOptionCount; o++) opt_[o] = kOptions[o].def;
	dev_.resize(plan_.stages.size());
	// (what the sizes below ask -- the groups, hb_front_possible -- does not depend on the lane tables built further down)
	resolve_forms();
	for (size_t s = 0; s < plan_.stages.size(); s++)
	{
		const StagePlan& sp = plan_.stages[s];
		StageDev& d = dev_[s];
		// (a decimator that option fuse_hbconv may take into the convolver behind it: the larger history of the two forms)
		const long long hist = std::max(stage_history(s), form_[s].hb_front_possible ? hbconv_history(s) : 0LL);
		// (+ one block of the convolver in front of it: the block that holds a call's last output is written whole,
		// ahead of what the call owes -- kBlockAhead, launch_conv_stage)
		// (the same behind a fused convolver + whole-step interpolator: a block's interpolated outputs -- launch_fused)
		// (the larger of the blocks the convolver may run on: the plan's, or its polyphase 3x block -- ConvGeom::p3)
		// (not park_len_of(, false): that bound follows the options -- up3_poly's block, the fused pair's blocking --
		// and is rounded up to whole 64-byte lines; a ring is sized here, once, for whichever block the options choose
		// later, and its size is part of the checkpoint format)
		long long ahead = s > 0 && plan_.stages[s - 1].desc.kind == kConv ?
			std::max(plan_.stages[s - 1].cg.in_len, plan_.stages[s - 1].cg.p3 ? 3 * plan_.stages[s - 1].cg.p3_m : 0) /
				plan_.stages[s - 1].cg.down + 2 : 0;
		if (s > 1 && plan_.stages[s - 1].desc.kind == kFrac && plan_.stages[s - 1].whole &&
			plan_.stages[s - 2].desc.kind == kConv)
			ahead = (long long) plan_.stages[s - 2].cg.in_len * plan_.stages[s - 1].out_step / plan_.stages[s - 1].in_step +
				plan_.stages[s - 1].out_step + 2;
		d.ring_size = pow2_at_least(s == 0 ? hist : hist + plan_.stage_max_in[s] + ahead);
		// rings are allocated on first use (ensure_ring): the ring between two fused stages is
		// never touched and would be the largest allocation (cfg2: 512 MB)
		if (sp.desc.kind == kConv)
		{
			const ConvGeom& g = sp.cg;
			if (g.n_in < 32 || g.n_out < 32)
				throw std::runtime_error("block convolver transform too short");
			// the generic kernel keeps both transforms' arrays in LDS, the fast path works in place
			const bool convx = convx_edge3(g) || convx_plain(g);
			const PairTables pk = pair_tables(g);
			const bool long_block = pk == kTabSplit || pk == kTabSolo || pk == kTabSoloDown;
			if (!generic_conv_fits(g) && !generic_conv_big(g) &&
				!(convx && convx_work_bytes(std::max(g.n_in, g.n_out) / 2) <= 160 * 1024))
				throw std::runtime_error("low-pass filter too long for the LDS-resident "
					"block convolver (transition band too narrow)");
			// (minimum phase, or an alignment moved by inherited latency -- a complex spectrum: 16384 points 1:1 in place; 2x
			// up-sampling or decimating at that length: neither array pair of the generic kernel fits)
			if (g.complex_h && !generic_conv_fits(g) && !long_block && !generic_conv_big(g))
				throw std::runtime_error("minimum-phase filter too long for the generic block convolver");
			const ConvTables T = conv_tables(sp);
			d.hp3.upload(T.hp3);
			d.ptw3.upload(T.ptw3);
			d.H.upload(T.H);
			d.Hc.upload(T.Hc);
			d.tw_len = g.bl2;
			d.tw.upload(T.tw);
			d.spec.upload(T.spec);
			d.spec2.upload(T.spec2);
			d.hp.upload(T.hp);
			d.ptw.upload(T.ptw);
		}
		else if (sp.desc.kind == kFrac)
		{
			d.table.upload(sp.bank->table);
			if (sp.whole) d.wtab.upload(whole_step_rows(sp));
		}
	}
	plan_transforms();
	for (size_t s = 0; s + 1 < plan_.stages.size(); s++)
		if (form_[s].group == kGroupConvWhole) prepare_two_phase(s);
	resolve_forms(); // (once more, now that the lane tables exist: the two-phase forms)
}

// The lane tables of the fused pair (convolver s, whole-step interpolator s + 1), where the interpolator has any
// (two_phase_tables, r8b_conv_tables.h)
void Engine::prepare_two_phase(size_t s)
{
	const std::optional<TwoPhaseTables> T = two_phase_tables(plan_.stages[s + 1]);
	if (!T) return;
	StageDev& d = dev_[s + 1];
	d.ptab.upload(T->ptab);
	d.ctab.upload(T->ctab);
	d.nsets = T->nsets;
	d.taps2 = T->taps2;
}

// ---- the per-stage record (StageForm, r8b_engine.h) ---------------------------------------------------------------
// Is a half-array form (r8b_convp.h cp_ha_*) worth taking for convolver stage s?  The forms pay where a launch holds more
// workgroups than the chip has slots for the full-array kernel -- two per CU, 512 --: channel pairs x blocks of the object's
// LARGEST call.  A constant of the object (its channel count, its MaxInLen, the stage's block), never of a call: on the
// device the two forms of a kernel agree to rounding only, and a stream stays with one.  Measured (r06_experiments.txt
// item 12): 1024 ch x 16384 -10.6 %, 256 ch -8.9 %, 64 ch x 16384 (384 workgroups) +0.6 %, 64 ch x 1024 (32) +0.5 %.
bool Engine::half_worth(size_t s) const
{
	const ConvGeom& g = plan_.stages[s].cg;
	const long long pairs = ((long long) form_nch() + 1) / 2;
	const long long per_block = std::max(1, g.in_len / std::max(1, g.up)); // stage input samples one block brings
	const long long blocks = ((long long) plan_.stage_max_in[s] + per_block - 1) / per_block;
	return pairs * blocks >= 512;
}

// The channel count every choice made by the object's size is made for: half_worth, the walk form, the half-band cascade's
// tile, runs of half-band decimators as one kernel, the channel groups of the polynomial interpolator.  Option
// "form_channels" (> 0) stands in for the object's own count, so that the shards of one batch choose as the whole batch
// does.
int Engine::form_nch() const
{
	return opt(kFormChannels) > 0 ? opt(kFormChannels) : nch_;
}

// The geometry stage s runs with: the plan's, or its polyphase 3x block (ConvGeom::p3, option up3_poly)
ConvGeom Engine::eff_geom(size_t s) const
{
	ConvGeom g = plan_.stages[s].cg;
	if (g.p3 && opt(kUp3Poly) && opt(kPairConv) && opt(kFastConv))
	{
		g.poly3 = true;
		g.in_len = 3 * g.p3_m;
		g.bl2 = 3 * g.p3_n;
		g.n_in = g.n_out = g.p3_n;
		g.blk_off = g.p3_off;
	}
	return g;
}

// which kernel family runs a convolver of (effective) geometry g on its own
ConvPath Engine::conv_path(const ConvGeom& g) const
{
	if (g.poly3) return kPathPairP3;
	const ConvPath generic = generic_conv_big(g) ? kPathGenericBig : kPathGeneric;
	if (!(opt(kFastConv) || !generic_conv_fits(g))) return generic;
	const bool up3 = !g.up_pow2 && g.up == 3, down3 = !g.down_pow2 && g.down == 3;
	const bool pair = opt(kPairConv) && pair_plain(g);
	// (8192 -> 16384-point blocks: the split 2x up-sampling form of the pair kernel, two channels per workgroup; 16384-point
	// blocks: its one-channel form -- instead of the one-channel kernel)
	// (with a complex kernel spectrum -- modes 12 ... 15 -- these forms are the only path such blocks have when the generic
	// kernel's arrays do not fit: the options do not switch them off then)
	const bool cx_only = g.complex_h && !generic_conv_fits(g);
	switch (pair_tables(g))
	{
	case kTabSplit: if ((opt(kPairConv) && opt(kPairSplit)) || cx_only) return down3 ? kPathPair3 : kPathPair; break;
	case kTabSolo: if ((opt(kPairConv) && opt(kPairSolo)) || cx_only) return up3 || down3 ? kPathPair3 : kPathPair; break;
	case kTabSoloDown: if ((opt(kPairConv) && opt(kPairSolo)) || cx_only) return up3 ? kPathPair3 : kPathPair; break;
	default: break;
	}
	if (opt(kPairConv) && pair_edge3(g)) return kPathPair3;
	if (g.complex_h) return pair ? kPathPair : generic; // (complex spectrum: pair kernel or generic)
	if (convx_edge3(g)) return kPathConvx3;
	if (pair) return kPathPair;
	if (convx_plain(g)) return kPathConvx;
	return generic;
}

// ... the pair kernel with two phases per thread (modes 4 / 5 / 16 / 17 carry the shifts of a chain with a fractional
// latency -- fused_shift) and nothing else in the pair of stages that the fused launch does not model
bool Engine::fuse_latency_ok(size_t s) const
{
	const StagePlan& c = plan_.stages[s];
	const StagePlan& w = plan_.stages[s + 1];
	if (!opt(kFuseLatency) || !opt(kPairTwo) || w.frac0 != 0.0) return false;
	return c.out_skip >= 0 && w.out_skip >= 0 && w.pos0 >= 0 && w.pos0 < w.out_step && two_phase_possible(w, nullptr);
}

// Convolver s + the whole-step interpolator behind it as one launch (launch_fused), and which kernel form runs it
FusedForm Engine::fused_form(size_t s) const
{
	if (!opt(kFuse) || !opt(kFastConv) || s + 1 >= plan_.stages.size()) return kFusedNone;
	const StagePlan& w = plan_.stages[s + 1];
	const ConvGeom& g = form_[s].g;
	if (plan_.stages[s].desc.kind != kConv || w.desc.kind != kFrac || !w.whole || g.down != 1) return kFusedNone;
	const bool pair = opt(kPairConv) && convp_fused_ok(g.n_in, g.n_out, g.up, g.down, g.up_pow2);
	// (the run's place in the array of the two-phase form: behind the zeros in front of it, whole 16-byte columns)
	const int run_off = (w.in_step + 16 + 15) / 16 * 16;
	const bool run_fits = run_off + g.in_len + w.in_step + 32 + 16 <= g.n_out;
	if (latency_chain_ && !(pair && run_fits && fuse_latency_ok(s))) return kFusedNone;
	// (8192 -> 16384-point blocks: the pair kernel's split form + the unfused interpolator beat the fused one-channel kernel;
	// 16384-point 1:1 blocks: the pair kernel's one-channel form with the interpolator fused in -- r8b_convp.h mode 18: real
	// kernel spectrum, plain load)
	if (opt(kSoloFuse) && opt(kPairSolo) && opt(kPairConv) && !g.complex_h && g.up_pow2 && g.up == 1 &&
		form_[s].path == kPathPair && pair_tables(g) == kTabSolo)
		return w.flen <= 32 && g.in_len >= 4 * w.flen && g.in_len + 64 <= g.n_out ? kFusedSolo : kFusedNone;
	if (form_[s].path == kPathPair && !pair) return kFusedNone; // (the long-block layouts)
	if (!convx_plain(g) && !pair) return kFusedNone;
	// (the linear output run and the zeros behind it live in the block's own part of the array)
	if (pair && g.in_len + 32 > g.n_out) return kFusedNone;
	// (one phase per thread in the one-channel kernel; the pair kernel walks tid, tid + 256, ...)
	if (w.out_step > (pair ? 2048 : 256) || w.flen > 32 || g.in_len < 4 * w.flen) return kFusedNone;
	if (!pair) return kFusedConvx;
	// two phases per thread only where construction built the lane tables (prepare_two_phase: for the pairs fused under the
	// DEFAULT options, where two_phase_possible holds)
	return opt(kPairTwo) && dev_[s + 1].ptab != nullptr && run_fits ? kFusedPair2 : kFusedPair1;
}

// Half-band decimator s in front of convolver s + 1 as one launch (r8b_convp.h mode 20, option fuse_hbconv): linear-phase
// chains, the 4096 -> 2048-point decimating geometry of the pair kernel (176400 -> 44100, 192000 -> 48000 ... at the
// 24-bit preset) -- whatever the options say (the rings are sized once, for either form)
bool Engine::hbconv_possible(size_t s) const
{
	if (s + 1 >= plan_.stages.size()) return false;
	const StagePlan& h = plan_.stages[s];
	const StagePlan& c = plan_.stages[s + 1];
	if (h.desc.kind != kHBDown || c.desc.kind != kConv || latency_chain_) return false;
	if (h.out_skip != 0 || h.hb_n > kHbfTapsMax || h.hb_n < 1) return false;
	const ConvGeom& g = form_[s + 1].g;
	if (g.poly3 || g.complex_h || !g.up_pow2 || g.up != 1 || !g.down_pow2 || g.down != 2) return false;
	return g.n_in == 2 * kHbfRound && g.n_out == kHbfRound && (g.in_len & 1) == 0;
}

// LDS of the decimating cascade: the stages' inputs alternate between two buffers, each sized for a full tile of `tile`
// last-stage outputs walked back through the (rounded) tap counts; returns the doubles of both
static const int kHbdMinTile = 32;
static size_t hbd_lds_doubles(const int* ntaps, int glen, int tile, int* buf, int* buf2)
{
	long long lo = 0, hi = tile, even = 0, odd = 0;
	for (int g = glen - 1; g >= 0; g--)
	{
		const int T = ntaps[g];
		const long long ilo = 2 * lo - (2 * T - 1), ihi = 2 * (hi - 1) + (2 * T - 1) + 1;
		lo = ilo;
		hi = ihi;
		long long& m = (g & 1) ? odd : even;
		m = std::max(m, hi - lo);
	}
	if (buf) *buf = (int) even + 8;
	if (buf2) *buf2 = (int) odd + 8;
	return (size_t) (even + 8 + odd + 8);
}

// stages of the run of half-band stages that starts at s (1: no run)
int Engine::run_len(size_t s) const
{
	const StageKind kind = plan_.stages[s].desc.kind;
	// Runs of decimators: one kernel saves two launches and the intermediate streams, but pays
	// ~25 % of halo recomputation and holds 25 KB of LDS per workgroup; measured on sacd.cpp's
	// 2822400 -> 176400 it wins on small batches (64 ch x 65536: 0.032 vs 0.037 ms) and loses on
	// large ones (256 ch: 0.111 vs 0.099 ms).  The choice must not change between calls (the
	// unfused stages keep their history in rings the fused kernel never writes): it is made from
	// the object's constants.
	const bool down_ok = opt(kFuseHbd) == 1 || (opt(kFuseHbd) == 2 &&
		(long long) form_nch() * plan_.stage_max_in[s] < (8LL << 20));
	if (!opt(kFuseHb) || !(kind == kHBUp || (kind == kHBDown && down_ok))) return 1;
	int n = 1;
	// (a decimator that goes into the convolver behind it is not part of a run)
	while (s + n < plan_.stages.size() && plan_.stages[s + n].desc.kind == kind && n < kMaxCascade &&
		form_[s + n].group != kGroupHbConv) n++;
	// A run of decimators keeps every stage's input of a tile in LDS, and each stage doubles the span and the halos of
	// the stages behind it: eight stages with a 14-wide filter at the end (DSD512 -> 44100 at 180 dB) ask for 220 KB at
	// the smallest tile, which the device refuses.  Such a run ends where it still fits; the rest starts the next run.
	// (From the object's constants, like the choice above.)
	if (kind == kHBDown)
		for (; n > 1; n--)
		{
			int ntaps[kMaxCascade];
			for (int g = 0; g < n; g++)
			{
				const int hb_n = plan_.stages[s + g].hb_n;
				ntaps[g] = hb_tap_width(hb_n);
			}
			if (hbd_lds_doubles(ntaps, n, kHbdMinTile, nullptr, nullptr) * sizeof(double) <= (size_t) kLdsMaxBytes) break;
		}
	return n;
}

// The one place that decides which kernel form runs each stage, from the plan, the options, form_nch() and the tables
// that exist.  Every path follows from the stage's EFFECTIVE geometry.  (A stage that takes the polyphase 3x form is never
// fused with the interpolator behind it and never fronted by a half-band decimator: up = 3 is no power of two, and both
// forms ask for one -- so the plan's geometry and the effective one give every group the same answer.)
void Engine::resolve_forms()
{
	const size_t ns = plan_.stages.size();
	form_.assign(ns, StageForm());
	latency_chain_ = false;
	for (const StagePlan& sp : plan_.stages)
		if (sp.out_skip != 0 || sp.pos0 != 0 || sp.frac0 != 0.0 || (sp.desc.kind == kConv && sp.cg.complex_h))
			latency_chain_ = true;
	for (size_t s = 0; s < ns; s++)
		if (plan_.stages[s].desc.kind == kConv)
		{
			form_[s].g = eff_geom(s);
			form_[s].path = conv_path(form_[s].g);
		}
	// groups, last stage first (a run of decimators ends in front of a decimator that goes into its convolver).  (Chains
	// with a fractional latency: the convolver + interpolator pair -- fuse_latency_ok -- and the half-band runs, whose
	// cascade kernels know the stages' skipped outputs, under option fuse_latency; nothing else)
	for (size_t s = ns; s-- > 0;)
	{
		StageForm& f = form_[s];
		const StageKind kind = plan_.stages[s].desc.kind;
		f.hb_front_possible = hbconv_possible(s);
		f.fused = fused_form(s);
		if (latency_chain_ && !opt(kFuseLatency)) continue;
		if (f.fused != kFusedNone) f.group = kGroupConvWhole;
		else if (opt(kFuseHbconv) && opt(kFastConv) && opt(kPairConv) && f.hb_front_possible && form_[s + 1].path == kPathPair &&
			pair_plain(form_[s + 1].g))
			f.group = kGroupHbConv;
		else if (kind == kHBUp || kind == kHBDown) f.glen = run_len(s);
		if (f.glen > 1) f.group = kGroupHbRun;
		if (f.group == kGroupConvWhole || f.group == kGroupHbConv) f.glen = 2;
	}
	for (size_t g = 0; g < ns; g += (size_t) form_[g].glen)
		for (int k = 1; k < form_[g].glen; k++) form_[g + k].member = true;
	// the convolvers' kernels (r8b_convp_mode.h) and what they do with the block that holds a call's last output -- park it
	// (the pair kernel's forms that know ConvxLaunch::park_*), keep it in an output ring (the one-channel kernel, whose
	// store only clips at the range's end), or compute it again (the generic kernel; the fused pair kernel with one phase
	// per thread)
	for (size_t s = 0; s < ns; s++)
	{
		StageForm& f = form_[s];
		if (plan_.stages[s].desc.kind != kConv) continue;
		const ConvGeom& g = f.g;
		const PairTables pk = pair_tables(g);
		const int lay = pk == kTabSolo || pk == kTabSoloDown ? kLaySolo : (pk == kTabSplit ? kLaySplit : kLayPair);
		f.quad = opt(kQuad) != 0 ? 1 : 0;
		f.half = opt(kHalf) == 2 || (opt(kHalf) == 1 && half_worth(s)) ? 1 : 0;
		f.half_fused = opt(kHalfFused) == 2 || (opt(kHalfFused) == 1 && half_worth(s)) ? 1 : 0;
		const int taps2 = s + 1 < ns ? dev_[s + 1].taps2 : 0;
		switch (f.fused)
		{
		case kFusedPair2:
			f.mode = convp_mode_find(kLayPair, taps2 == 27 ? kBackWhole2W : kBackWhole2, g.complex_h);
			f.run_off = (plan_.stages[s + 1].in_step + 16 + 15) / 16 * 16;
			f.last = kBlockPark;
			break;
		// (a complex spectrum needs the two-phase tables -- fuse_latency_ok --: no mode, launch_fused refuses)
		case kFusedPair1: f.mode = g.complex_h ? kConvpModeNone : convp_mode_find(kLayPair, kBackWhole1, false); f.last = kBlockAgain; break;
		case kFusedSolo: f.mode = convp_mode_find(kLaySolo, kBackWhole1, false); f.last = kBlockPark; break;
		case kFusedConvx: f.mode = kBackWhole1; f.last = kBlockOutRing; break;
		case kFusedNone:
			switch (f.path)
			{
			case kPathGeneric: case kPathGenericBig: f.last = kBlockAgain; break;
			case kPathConvx: f.mode = kBackConv; f.last = kBlockOutRing; break;
			case kPathConvx3: f.mode = kBackEdge3; f.last = kBlockOutRing; break;
			case kPathPairP3: f.mode = convp_mode_find(kLayP3, kBackConv, false); f.last = kBlockPark; break;
			case kPathPair3: f.mode = convp_mode_find(lay, kBackEdge3, g.complex_h); f.last = kBlockPark; break;
			case kPathPair:
				f.mode = f.member ? convp_mode_find(kLayHbf, kBackConv, false) : convp_mode_find(lay, kBackConv, g.complex_h);
				f.last = kBlockPark;
				break;
			}
			break;
		}
		f.end = s + (size_t) (f.group == kGroupConvWhole ? 2 : 1) == ns;
		f.parks = opt(kPark) && f.end && f.last != kBlockAgain;
	}
	// PCM at the edges (Engine::process_planar): a streaming kernel or the generic convolver decodes / encodes planar PCM
	// caller buffers in place; the compile-time-sized convolvers (r8b_convx.h, r8b_convp.h) exist for fp64 views only --
	// r8b_kernels.hip, top -- and have the samples brought to them through the staging rows (r8b_capi.cpp).
	pcm_in_ = ns > 0 && form_[0].group != kGroupHbConv && !(plan_.stages[0].desc.kind == kConv && form_[0].fast());
	pcm_out_ = ns > 0 && !(ns >= 2 && form_[ns - 2].group == kGroupConvWhole) &&
		!(plan_.stages[ns - 1].desc.kind == kConv && form_[ns - 1].fast());
}

// The policy of one launch (LastBlock, r8b_engine.h).  At the end of the chain -- the caller's fp64 rows, the one
// destination that cannot take outputs ahead of their call -- the kernel's own form; in the middle of the chain every
// form that computes the block once simply writes it ahead into the next stage's ring (nobody reads it before it is due;
// the ring was sized for it -- Engine::Engine).  Option park = 0, PCM rows: kBlockAgain.
LastBlock Engine::last_block(size_t s, const DstView& dst) const
{
	const StageForm& f = form_[s];
	if (!opt(kPark) || dst.fmt != kPcmF64 || f.end != (dst.mask == -1)) return kBlockAgain;
	const LastBlock policy = f.end || f.last == kBlockAgain ? f.last : kBlockAhead;
	if ((policy == kBlockPark || policy == kBlockOutRing) && !f.parks)
		throw std::logic_error("a stage without park buffers asked to park");
	return policy;
}

// doubles per channel of a park buffer (end_of_chain; the stage parks): what one block can hold, rounded up to
// whole 64-byte lines -- or, as an output ring, a call's outputs plus one block's, a power of two.
// (end_of_chain = false: the bound on what a stage in the MIDDLE of a chain writes ahead into the next ring -- one
// block's outputs, whatever kernel runs it; load_state checks a blob's counters against it.  The ring's own size is
// another bound: Engine::Engine.)
long long Engine::park_len_of(size_t s, bool end_of_chain) const
{
	const StageForm& f = form_[s];
	if (end_of_chain && !f.parks) throw std::logic_error("park buffer of a stage that does not park");
	long long n;
	if (f.fused != kFusedNone)
	{
		long long S = 0, off = 0;
		fused_blocking(s, &S, &off);
		const StagePlan& w = plan_.stages[s + 1];
		n = (S * w.out_step + w.in_step - 1) / w.in_step + 2;
		// (block 0 holds every output whose window ends inside its valid run [-fl2, in_len - fl2): more than a later
		// block's share when fl2 is small -- a minimum-phase filter's few samples)
		const long long e0 = (long long) f.g.in_len + off - f.g.fl2 - w.fl2 - fused_shift(s).d;
		if (e0 > 0) n = std::max(n, (e0 * w.out_step + w.in_step - 1) / w.in_step + 2);
	}
	else n = f.g.in_len / f.g.down + 2;
	if (end_of_chain && f.last == kBlockOutRing) return pow2_at_least(plan_.max_out_len + n + 16);
	return (n + 7) / 8 * 8 + 8;
}

void Engine::ensure_park(size_t s)
{
	StageDev& d = dev_[s];
	const long long len = park_len_of(s, true);
	if (d.park[0] != nullptr && d.park_stride == len) return;
	// (the row length follows the structural options -- pair_solo, pair_conv, align_groups ... --, which may change
	// between clear() and the next process(): buffers of another length are replaced, and they hold nothing then)
	if (d.park[0] != nullptr)
	{
		if (d.park_end > d.park_base) throw std::logic_error("park buffer resized while it holds outputs");
		d.park[0].reset();
		d.park[1].reset();
		d.park_cur = 0;
	}
	d.park_stride = len;
	const size_t bytes = (size_t) d.park_stride * (size_t) nch_ * sizeof(double);
	d.park[0].alloc(bytes);
	d.park[1].alloc(bytes);
}

// kBlockOutRing: where the kernel writes (the current channel window of the ring in park[0]) ...
DstView Engine::out_ring_view(size_t s) const
{
	const StageDev& d = dev_[s];
	DstView v;
	v.p = d.park[0] + (long long) ch0_ * d.park_stride;
	v.stride = d.park_stride;
	v.mask = d.park_stride - 1;
	v.off = 0;
	v.fmt = kPcmF64;
	return v;
}

// ... and the copy of the call's outputs [a, b) from there to the caller's rows (k_tail)
void Engine::ring_to_rows(size_t s, long long a, long long b, const DstView& dst, void* stream)
{
	const DstView ring = out_ring_view(s);
	TailLaunch T;
	T.src.ring = ring.p;
	T.src.ring_stride = ring.stride; T.src.ring_mask = ring.mask;
	T.src.cur = T.src.ring; T.src.cur_stride = 0; T.src.cur_base = LLONG_MAX;
	T.src.cur_fmt = kPcmF64;
	T.p0 = a; T.p1 = b;
	T.ring = dst.p + dst.off; T.ring_stride = dst.stride; T.ring_mask = -1;
	T.nch = nchw_;
	// (the stage's symbol stays its convolver's: this copy follows every one of its launches -- as in the emulator,
	// whose copy notes none)
	const char* const sym = launch_symbol_last();
	launch_tail(T, stream);
	launch_symbol_note(sym);
}

// What the previous call's last block left of this call's outputs [a, b): returns the first output the call still has
// to compute; kBlockPark: the launch takes [a, that) out of the park buffer beside its loads (X.park_src ...)
long long Engine::take_parked(size_t s, LastBlock policy, long long a, long long b, ConvxLaunch& X)
{
	const StageDev& d = dev_[s];
	if (policy == kBlockAgain || d.park_end <= a) return a;
	const long long ca = std::min(d.park_end, b);
	if (policy == kBlockPark)
	{
		if (d.park_base > a) throw std::logic_error("parked outputs start behind the call's first output");
		X.park_src = d.park[d.park_cur] + (long long) ch0_ * d.park_stride + (a - d.park_base);
		X.park_stride = d.park_stride;
		X.park_j0 = a;
		X.park_n = (int) (ca - a);
		if (ch0_ == 0) stat_[kParkCalls]++;
	}
	return ca;
}

// A (short) call with nothing left to compute: its outputs are in the next stage's ring already (kBlockAhead), or come
// out of the park buffer / the output ring by a plain copy; the stream's history is kept by process() (tail_done_
// stays false)
void Engine::serve_parked(size_t s, LastBlock policy, const ConvxLaunch& X, long long a, long long b, const DstView& dst,
	void* stream)
{
	if (policy == kBlockPark)
	{
		TailLaunch T;
		T.src.ring = X.park_src; T.src.ring_stride = 0; T.src.ring_mask = 0;
		T.src.cur = X.park_src; T.src.cur_stride = X.park_stride; T.src.cur_base = a;
		T.src.cur_fmt = kPcmF64;
		T.p0 = a; T.p1 = b;
		T.ring = dst.p + dst.off; T.ring_stride = dst.stride; T.ring_mask = -1;
		T.nch = nchw_;
		launch_tail(T, stream);
	}
	if (policy == kBlockOutRing) ring_to_rows(s, a, b, dst, stream);
	if ((policy == kBlockPark || policy == kBlockOutRing) && ch0_ == 0) stat_[kParkOnlyCalls]++;
}

// The call's last block is computed whole, its outputs end at pend >= b: is there room for [b, pend) where the policy
// puts them?  (`next`: the stage that reads this launch's outputs.  kBlockPark: park_beyond)
void Engine::check_last_block(size_t s, size_t next, LastBlock policy, const DstView& dst, long long a, long long b,
	long long pend) const
{
	if (pend < b) throw std::logic_error("block bookkeeping of the convolver");
	if (policy == kBlockAhead &&
		(dst.mask == -1 || dst.mask + 1 < stage_history(next) + plan_.stage_max_in[next] + (pend - b)))
		throw std::logic_error("ring too small for a block written ahead");
	if (policy == kBlockOutRing && pend - a > dev_[s].park_stride) throw std::logic_error("output ring too small");
}

// kBlockPark: the launch's last block leaves [b, pend) in the other park buffer (the span fields of X.park_blk that
// the fused forms read are the caller's)
void Engine::park_beyond(size_t s, ConvxLaunch& X, long long b, long long pend) const
{
	const StageDev& d = dev_[s];
	if (pend - b > d.park_stride) throw std::logic_error("park buffer too small");
	X.park_out = 1;
	X.park_dst = d.park[d.park_cur ^ 1] + (long long) ch0_ * d.park_stride;
	X.park_stride = d.park_stride;
	X.park_blk.jlo = b;
	X.park_blk.jhi = pend;
}

// the counters once per call, after its last channel window: the stream's outputs [b, pend) exist already
void Engine::commit_last_block(size_t s, LastBlock policy, long long b, long long pend)
{
	if (policy == kBlockAgain || ch0_ + nchw_ < act_) return;
	StageDev& d = dev_[s];
	if (policy == kBlockPark && pend > b) d.park_cur ^= 1;
	d.park_base = b;
	d.park_end = pend;
}

// the descriptor's optional forms: none parked, none of the alternative kernel forms
static void no_optional_forms(ConvxLaunch& X)
{
	X.park_n = 0; X.park_out = 0; X.park_slices = 0; X.park_j0 = 0; X.park_stride = 0;
	X.park_src = nullptr; X.park_dst = nullptr;
	X.park_blk = SpanInfo();
	X.walk = 0;
	X.quad = 0; X.half = 0; X.half_fused = 0;
}

// History for the next call, exactly (a fast convolver at stage 0 keeps it itself: fill_conv asked for history(), the
// bound over every way of cutting the stream into calls -- about twice what a call of MaxInLen samples needs): the next
// call's first block reads back to input position wstart, and no later block reads further back.  Even: pairs of
// samples.
static void next_call_tail_p0(ConvLaunch& L, long long wstart)
{
	const long long p0 = std::min(std::max(L.tail_p0, wstart - 8), L.tail_p1);
	L.tail_p0 = p0 < 0 ? 0 : (p0 & ~1LL);
}

Engine::StageDevs::~StageDevs()
{
	if (empty()) return;
	// (a destructor: a device that cannot be made current any more -- runtime unloaded at interpreter exit, sticky
	// error -- must not throw here; the frees below then fail silently)
	int prev = -1;
	try { prev = dev_swap(device); } catch (...) { prev = -1; }
	struct Restore { int prev; ~Restore() { if (prev >= 0) dev_restore(prev); } } restore{prev};
	for (StageDev& d : *this)
	{
		for (auto& pr : d.pending)
		{
			dev_event_destroy(pr.first);
			dev_event_destroy(pr.second);
		}
		for (void* e : d.free_events) dev_event_destroy(e);
	}
	clear(); // (every stage's blocks are freed here, with the device current; `restore` goes after them)
}

void Engine::plan_transforms()
{
	for (size_t s = 0; s < plan_.stages.size(); s++)
	{
		const StagePlan& sp = plan_.stages[s];
		if (sp.desc.kind != kConv) continue;
		const bool big = generic_conv_big(sp.cg);
		dev_[s].fwd_radix = plan_radices(sp.cg.n_in / 2, opt(kConvRadix));
		std::vector<int> inv = plan_radices(sp.cg.n_out / 2, big ? 16 : opt(kConvRadix));
		if (big)
		{
			// (k_conv_big: a radix-2 stage in the load, then the two sub-blocks of half the length on their own, on 512
			// threads -- one radix-16 butterfly each)
			dev_[s].fwd_radix = plan_radices(sp.cg.n_in / 4, 16);
			dev_[s].fwd_radix.insert(dev_[s].fwd_radix.begin(), 2);
		}
		// backward passes run with growing sub-transform length: smallest radix group first
		dev_[s].inv_radix.assign(inv.rbegin(), inv.rend());
	}
}

bool Engine::set_option(const std::string& name, int value)
{
	int o = 0;
	while (o < kOptionCount && name != kOptions[o].name) o++;
	if (o == kOptionCount) return false;
	const bool started = std::any_of(plan_.stages.begin(), plan_.stages.end(), [](const StagePlan& sp) { return sp.m != 0; });
	if (started && kOptions[o].structural && opt_[o] != value) return false;
	const bool changed = opt_[o] != value;
	opt_[o] = value;
	plan_transforms();
	if (changed) resolve_forms();
	return true;
}

long long Engine::stat(const std::string& name) const
{
	for (int c = 0; c < kCounterCount; c++)
		if (name == kCounterNames[c]) return stat_[c];
	return -1;
}

void Engine::ensure_ring(size_t s)
{
	StageDev& d = dev_[s];
	if (d.ring != nullptr) return;
	const size_t bytes = (size_t) d.ring_size * (size_t) nch_ * sizeof(double);
	d.ring.alloc(bytes);
	if (s == 0) d.ring_alt.alloc(bytes);
}

// backward-spectrum arrays of the long-block generic convolver (k_conv_big), one per workgroup of its launch: grown,
// never shrunk; growing waits for the device (the arrays may be in use by an earlier launch), which happens on an
// object's first calls only
void Engine::ensure_work(size_t s, int slots, void* stream)
{
	StageDev& d = dev_[s];
	if (d.work != nullptr && d.work_slots >= slots) return;
	if (d.work != nullptr) dev_sync(stream); // (hipFree waits for the device besides)
	d.work.alloc((size_t) slots * (size_t) plan_.stages[s].cg.n_out * sizeof(double));
	d.work_slots = slots;
}

// a half-band launch takes the call's pending history copy with it (Engine::process)
void Engine::take_carried_tail(TailLaunch& T, int* carry)
{
	*carry = 0;
	T = carry_tail_;
	if (!carry_) return;
	carry_ = false;
	tail_done_ = true;
	if (carry_tail_.p1 > carry_tail_.p0) *carry = 1;
}

void* Engine::get_event(StageDev& d)
{
	if (!d.free_events.empty())
	{
		void* e = d.free_events.back();
		d.free_events.pop_back();
		return e;
	}
	return dev_event_create();
}

bool Engine::stage_timing(size_t stage, double* ms_sum, int* launches, std::string* kernel,
	long long* in_samples, long long* out_samples)
{
	if (stage >= dev_.size()) return false;
	StageDev& d = dev_[stage];
	for (auto& pr : d.pending)
	{
		d.ms_sum += dev_event_elapsed_ms(pr.first, pr.second);
		d.launches++;
		d.free_events.push_back(pr.first);
		d.free_events.push_back(pr.second);
	}
	d.pending.clear();
	if (ms_sum) *ms_sum = d.ms_sum;
	if (launches) *launches = d.launches;
	if (in_samples) *in_samples = d.t_in;
	if (out_samples) *out_samples = d.t_out;
	if (kernel)
	{
		const StagePlan& sp = plan_.stages[stage];
		const StageForm& f = form_[stage];
		switch (sp.desc.kind)
		{
		case kConv:
			*kernel = f.fused != kFusedNone ? (f.fused == kFusedConvx ? "k_convx_whole" : "k_convp_whole") :
				(f.pair() ? "k_convp" : (f.fast() ? "k_convx" : "k_conv"));
			break;
		case kFrac: *kernel = sp.whole ? "k_whole" : "k_poly"; break;
		case kHBUp: *kernel = f.glen > 1 ? "k_hbcascade" : "k_hbup"; break;
		case kHBDown: *kernel = f.group == kGroupHbConv ? "k_convp_hb" : (f.glen > 1 ? "k_hbdcascade" : "k_hbdown"); break;
		}
	}
	d.ms_sum = 0.0;
	d.launches = 0;
	d.t_in = d.t_out = 0;
	return true;
}

std::string Engine::stage_symbol(size_t stage) const
{
	return stage < dev_.size() ? dev_[stage].symbol : std::string();
}

void Engine::clear()
{
	// ring contents need no reset: positions restart at 0 and every position >= 0 is rewritten
	// before it is read again, positions < 0 read as zero by construction
	plan_.clear();
	act_min_ = nch_;
	// (park_cur too: the output-ring use of the buffers -- kBlockOutRing -- knows park[0] only)
	for (StageDev& d : dev_)
	{
		d.park_base = d.park_end = 0;
		d.park_cur = 0;
	}
}

#ifdef R8B_TEST_HOOKS
long long Engine::test_skip_silence(long long n, void* stream)
{
	if (n < 0) throw std::runtime_error("negative sample count");
	for (const StagePlan& sp : plan_.stages)
	{
		if (sp.m != 0 || sp.done != 0)
			throw std::runtime_error("the object has processed samples since creation / r8b_batch_clear()");
		if (sp.desc.kind == kFrac && !sp.whole)
			throw std::runtime_error("the chain holds a polynomial interpolator: its position counter is stepped per output");
	}
	// (an object in use before its clear() holds that stream's samples in its rings: at positions behind 0 nobody would
	// read them, at the positions behind n the next call does)
	DevGuard guard(device_);
	for (size_t s = 0; s < dev_.size(); s++)
	{
		StageDev& d = dev_[s];
		const size_t bytes = (size_t) d.ring_size * (size_t) nch_ * sizeof(double);
		if (d.ring != nullptr) dev_zero(d.ring, bytes, stream);
		if (d.ring_alt != nullptr) dev_zero(d.ring_alt, bytes, stream);
	}
	for (StagePlan& sp : plan_.stages) n = sp.skip(n);
	return n;
}
#endif

// ---- checkpoint -------------------------------------------------------------------------------
// blob: StateHeader, then per stage a StageState followed by the stage's input ring (nch x
// ring_size doubles) when that ring exists (the ring between two fused stages never does)
namespace {
struct StateHeader
{
	char magic[8];
	unsigned long long config;
	long long nstages, nch;
};
struct StageState
{
	long long m, done, rpos, ring_size, has_ring;
	double pos_frac, pos_shift;
	long long in_counter, in_pos_int;
	// parked outputs (StageForm::parks): doubles per channel (0: the stage does not park), the stream positions the
	// buffer holds; the buffer itself (nch x park_len doubles) follows the ring
	long long park_len, park_base, park_end;
};
}

unsigned long long Engine::config_hash() const
{
	// FNV-1a over everything that shapes the rings and the schedule
	std::string key = plan_.describe();
	key += "|maxin=" + std::to_string(plan_.max_in) + "|nch=" + std::to_string(nch_);
	// (the hashed options in their names' order, as once kept in a std::map: blobs of earlier builds still load)
	std::map<std::string, int> hashed;
	for (int o = 0; o < kOptionCount; o++)
		if (kOptions[o].hashed) hashed[kOptions[o].name] = opt_[o];
	for (const auto& kv : hashed) key += "|" + kv.first + "=" + std::to_string(kv.second);
	unsigned long long h = 1469598103934665603ull;
	for (unsigned char c : key)
	{
		h ^= c;
		h *= 1099511628211ull;
	}
	return h;
}

// does stage s ever own an input ring?  (the ring between the two stages of a fused pair / inside
// a fused run is never touched)
bool Engine::stage_owns_ring(size_t s) const
{
	return !form_[s].member;
}

size_t Engine::state_size() const
{
	// the same before and after the first process() call: every ring a stage will ever own counts,
	// allocated yet or not (save_state allocates the missing ones, their content is all zero)
	size_t n = sizeof(StateHeader);
	for (size_t s = 0; s < dev_.size(); s++)
	{
		n += sizeof(StageState);
		if (stage_owns_ring(s)) n += (size_t) dev_[s].ring_size * (size_t) nch_ * sizeof(double);
		if (form_[s].parks) n += (size_t) park_len_of(s, true) * (size_t) nch_ * sizeof(double);
	}
	return n;
}

size_t Engine::save_state(void* buf, size_t cap, void* stream)
{
	const size_t need = state_size();
	if (cap < need) throw std::runtime_error("state buffer too small");
	DevGuard guard(device_);
	for (size_t s = 0; s < dev_.size(); s++)
	{
		if (stage_owns_ring(s)) ensure_ring(s);
		if (form_[s].parks) ensure_park(s);
	}
	dev_sync(stream);
	unsigned char* p = static_cast<unsigned char*>(buf);
	StateHeader h;
	std::memcpy(h.magic, "R8BHIPS2", 8);
	h.config = config_hash();
	h.nstages = (long long) dev_.size();
	h.nch = nch_;
	std::memcpy(p, &h, sizeof(h));
	p += sizeof(h);
	for (size_t s = 0; s < dev_.size(); s++)
	{
		const StagePlan& sp = plan_.stages[s];
		const StageDev& d = dev_[s];
		StageState st;
		st.m = sp.m; st.done = sp.done;
		st.rpos = sp.poly.rpos; st.pos_frac = sp.poly.pos_frac; st.pos_shift = sp.poly.pos_shift;
		st.in_counter = sp.poly.in_counter; st.in_pos_int = sp.poly.in_pos_int;
		st.ring_size = d.ring_size;
		st.has_ring = stage_owns_ring(s) ? 1 : 0;
		st.park_len = form_[s].parks ? park_len_of(s, true) : 0;
		if (st.park_len != 0 && st.park_len != d.park_stride) throw std::logic_error("park buffer length");
		st.park_base = d.park_base; st.park_end = d.park_end;
		std::memcpy(p, &st, sizeof(st));
		p += sizeof(st);
		if (st.has_ring)
		{
			const size_t bytes = (size_t) d.ring_size * (size_t) nch_ * sizeof(double);
			dev_download(p, d.ring, bytes, stream);
			p += bytes;
		}
		if (st.park_len > 0)
		{
			const size_t bytes = (size_t) st.park_len * (size_t) nch_ * sizeof(double);
			if ((size_t) (p - static_cast<unsigned char*>(buf)) + bytes > need) throw std::logic_error("state size");
			dev_download(p, d.park[d.park_cur], bytes, stream);
			p += bytes;
		}
	}
	if ((size_t) (p - static_cast<unsigned char*>(buf)) != need) throw std::logic_error("state size");
	return need;
}

void Engine::load_state(const void* buf, size_t size, void* stream)
{
	const unsigned char* p = static_cast<const unsigned char*>(buf);
	const unsigned char* const end = p + size;
	StateHeader h;
	if (size < sizeof(h)) throw std::runtime_error("state blob truncated");
	std::memcpy(&h, p, sizeof(h));
	p += sizeof(h);
	if (std::memcmp(h.magic, "R8BHIPS2", 8) != 0) throw std::runtime_error("not a state blob");
	if (h.config != config_hash() || h.nstages != (long long) dev_.size() || h.nch != nch_)
		throw std::runtime_error("state blob was saved by a differently configured resampler");
	// pass 1: the whole blob against this object, nothing touched yet (a truncated or foreign blob
	// must not leave a half-restored stream behind)
	if (size != state_size()) throw std::runtime_error("state blob has the wrong size");
	std::vector<StageState> sts(dev_.size());
	std::vector<const unsigned char*> rings(dev_.size(), nullptr), parks(dev_.size(), nullptr);
	for (size_t s = 0; s < dev_.size(); s++)
	{
		const StageDev& d = dev_[s];
		StageState& st = sts[s];
		if ((size_t) (end - p) < sizeof(st)) throw std::runtime_error("state blob truncated");
		std::memcpy(&st, p, sizeof(st));
		p += sizeof(st);
		if (st.ring_size != d.ring_size) throw std::runtime_error("state blob ring size mismatch");
		if ((st.has_ring != 0) != stage_owns_ring(s))
			throw std::runtime_error("state blob ring layout mismatch");
		if (st.m < 0 || st.done < 0 || st.in_counter < 0 || st.in_pos_int < 0 ||
			st.in_counter > INT_MAX || st.in_pos_int > INT_MAX || !(st.pos_frac >= 0.0 && st.pos_frac < 1.0))
			throw std::runtime_error("state blob holds impossible counters");
		if (st.has_ring)
		{
			const size_t bytes = (size_t) d.ring_size * (size_t) nch_ * sizeof(double);
			if ((size_t) (end - p) < bytes) throw std::runtime_error("state blob truncated");
			rings[s] = p;
			p += bytes;
		}
		if (st.park_len != (form_[s].parks ? park_len_of(s, true) : 0))
			throw std::runtime_error("state blob park layout mismatch");
		// (a stage that writes its last block ahead into a ring has counters but no buffer: what lies between them is
		// at most one block's outputs -- a larger park_end would make the next calls skip their blocks and hand out
		// whatever the ring holds --, and only a convolver ever has any)
		if (st.park_base < 0 || st.park_end < st.park_base || (st.park_len > 0 && st.park_end - st.park_base > st.park_len))
			throw std::runtime_error("state blob holds impossible counters");
		if (st.park_len == 0 && st.park_end - st.park_base >
			(plan_.stages[s].desc.kind == kConv && s + 1 < dev_.size() ? park_len_of(s, false) : 0))
			throw std::runtime_error("state blob holds impossible counters");
		if (st.park_len > 0)
		{
			const size_t bytes = (size_t) st.park_len * (size_t) nch_ * sizeof(double);
			if ((size_t) (end - p) < bytes) throw std::runtime_error("state blob truncated");
			parks[s] = p;
			p += bytes;
		}
	}
	if (p != end) throw std::runtime_error("state blob has trailing bytes");
	// pass 2: commit
	DevGuard guard(device_);
	dev_sync(stream);
	act_min_ = nch_; // (the blob holds every channel's state)
	for (size_t s = 0; s < dev_.size(); s++)
	{
		StagePlan& sp = plan_.stages[s];
		const StageState& st = sts[s];
		sp.m = st.m; sp.done = st.done;
		sp.poly.rpos = st.rpos; sp.poly.pos_frac = st.pos_frac; sp.poly.pos_shift = st.pos_shift;
		sp.poly.in_counter = (int) st.in_counter; sp.poly.in_pos_int = (int) st.in_pos_int;
		if (rings[s] != nullptr)
		{
			ensure_ring(s);
			dev_upload(dev_[s].ring, rings[s], (size_t) dev_[s].ring_size * (size_t) nch_ * sizeof(double));
		}
		if (parks[s] != nullptr)
		{
			// (buffers of an earlier life under other options are replaced here -- while the old counters still say
			// whether they may be)
			dev_[s].park_base = dev_[s].park_end = 0;
			ensure_park(s);
		}
		dev_[s].park_base = st.park_base; dev_[s].park_end = st.park_end;
		if (parks[s] != nullptr)
		{
			dev_upload(dev_[s].park[dev_[s].park_cur], parks[s], (size_t) dev_[s].park_stride * (size_t) nch_ * sizeof(double));
		}
	}
}

// A convolver stage on its own.  hb_front >= 0 (launch_hbconv): the half-band decimator whose filter the launch takes
// in its load -- `src` is then the DECIMATOR's input stream, and the return value is where the next call's first block
// starts reading that raw stream (the history the call has to leave; LLONG_MIN: the call computed no block, or there is
// no front).
long long Engine::launch_conv_stage(size_t s, long long hb_front, long long a, long long b, const SrcView& src,
	const DstView& dst, void* stream)
{
	const StageDev& d = dev_[s];
	const StageForm& f = form_[s];
	const ConvGeom& g = f.g;
	const ConvPath path = f.path;
	ConvxLaunch X;
	ConvLaunch& L = X.c;
	fill_conv(s, L, src);
	if (hb_front >= 0)
	{
		// (kernel mode 20 has no per-block spans, the front's parameters lie over the end of that array)
		const StagePlan& hp = plan_.stages[(size_t) hb_front];
		HbFront& F = X.hbf.p;
		F.n = hp.hb_n;
		F.np = hb_tap_width(hp.hb_n);
		F.end = hp.m;
		for (int i = 0; i < kHbfTapsMax; i++) F.taps[i] = i < hp.hb_n ? hp.hb_taps[i] : 0.0;
		L.vec_ok = 0;
	}
	if (g.poly3)
	{
		// polyphase 3x form (ConvGeom::p3; r8b_convp.h mode 19): a block is a window of p3_n INPUT samples, its valid
		// outputs the 3 p3_m virtual samples from k in_len + blk_off - fl2 (a multiple of 3) on; rot carries the
		// components' reach into the past
		L.bl2 = g.bl2; L.in_len = g.in_len; L.n_in = L.n_out = g.n_in;
		L.blk_stride = g.in_len; L.blk_offset = g.blk_off;
		L.rot = g.p3_b;
		L.hp = d.hp3; L.ptw = d.ptw3;
	}
	// Every block once (LastBlock): the block that holds the call's last output is computed whole, and the next call
	// starts behind it instead of computing that block again (one block in 13.4 for 44100 -> 88200 at BASELINE's call
	// size, one in 7.1 for 88200 -> 44100, one in 6.4 for 48000 -> 32000; cf. launch_fused).  The pair kernels put what
	// the block holds beyond b into the park buffer themselves (kBlockPark).  The one-channel fast path (r8b_convx.h:
	// 16384-point blocks and what else the pair form does not cover) only clips its store at L.b, so the same is had
	// without a kernel change by moving L.b to the block's end -- in the middle of a chain as for every kernel
	// (kBlockAhead), at the end of the chain with the output ring as the kernel's destination (kBlockOutRing: 2 x 8
	// bytes per output more for the copy, for one block in 5.2 less at 48000 -> 32000 with a 0.5 % transition band)
	const LastBlock policy = last_block(s, dst);
	// (blk_off: 0 but for the polyphase 3x form, whose blocks start on multiples of 3 -- <= 0, so the sum stays >= 0)
	auto blk_of = [&](long long q) { return ((long long) g.down * q + g.fl2 - g.blk_off) / g.in_len; };
	auto blk_end = [&](long long k) // the first output block k does not hold
	{
		const long long v = (k + 1) * (long long) g.in_len + g.blk_off - g.fl2;
		return v <= 0 ? 0LL : (v + g.down - 1) / g.down;
	};
	no_optional_forms(X);
	X.quad = f.quad;
	X.half = f.half;
	if (policy == kBlockPark || policy == kBlockOutRing) ensure_park(s);
	const long long ca = take_parked(s, policy, a, b, X); // the first output this call has to compute
	if (ca >= b)
	{
		serve_parked(s, policy, X, a, b, dst, stream);
		return LLONG_MIN;
	}
	L.k0 = blk_of(ca);
	const long long k1 = blk_of(b - 1);
	L.nblk = (int) (k1 - L.k0 + 1);
	L.a = ca; L.b = b;
	L.dst = policy == kBlockOutRing ? out_ring_view(s) : dst;
	long long pend = b; // end of what the call's last block holds
	if (policy != kBlockAgain)
	{
		pend = blk_end(k1);
		check_last_block(s, s + 1, policy, dst, a, b, pend);
		if (policy != kBlockPark) L.b = pend;
	}
	if (!f.fast())
	{
		L.tail_ring = nullptr;
		if (path == kPathGenericBig)
		{
			// (the reference's 32768-point block in front of a decimation in the spectrum: the launch's workgroups --
			// one per CU, 128 KB of LDS each -- walk the (block, channel) items; a workgroup's packed backward spectrum
			// passes through its own array in global memory)
			const long long items = (long long) L.nblk * L.nch;
			const int slots = (int) std::min<long long>(items, 256);
			ensure_work(s, slots, stream);
			L.work = dev_[s].work;
			L.work_slots = slots;
			L.threads = 512;
		}
		launch_conv(L, stream);
		return LLONG_MIN;
	}
	X.in_step = X.out_step = 1; X.flen = 2; X.fl2w = X.fllw = 0; X.run_off = 0;
	X.ptab = nullptr; X.ctab = nullptr; X.nsets = 0;
	X.table = nullptr; X.wtab = nullptr; X.wa = X.wb = 0; X.wdst = L.dst;
	if (policy == kBlockPark && pend > b) park_beyond(s, X, b, pend);
	// (the next call's first block: the one behind this call's last when every block is computed once, else the one
	// that holds output b)
	const long long kn = policy != kBlockAgain ? k1 + 1 : blk_of(b);
	// (its window starts p3_b input samples before its first output's input position)
	if (path == kPathPairP3 && L.tail_ring != nullptr)
		next_call_tail_p0(L, (kn * (long long) g.in_len + g.blk_off - g.fl2) / 3 - g.p3_b);
	if ((path == kPathPair || path == kPathPair3) && L.tail_ring != nullptr && g.up_pow2)
	{
		// (blocks sit at multiples of in_len, a block's window is n_in input samples ending in_len / up behind its
		// start -- cf. launch_fused; up is 1 or 2 on this path)
		if (g.up > 2) throw std::logic_error("pair convolver: up-sampling factor");
		next_call_tail_p0(L, ((kn * g.in_len) >> (g.up > 1 ? 1 : 0)) - ((long long) g.n_in - g.in_len / g.up));
	}
	if (ch0_ == 0) stat_[kConvBlocks] += L.nblk;
	if ((hb_front >= 0) != f.member) throw std::logic_error("half-band front of a convolver resolved without one");
	if (f.pair()) launch_convp(X, f.mode, stream);
	else launch_convx(X, f.mode, stream);
	if (L.tail_ring != nullptr) tail_done_ = true;
	if (policy == kBlockOutRing) ring_to_rows(s, a, b, dst, stream);
	commit_last_block(s, policy, b, pend);
	// (the half-band front: that block's window starts n_in - in_len convolver inputs before the block)
	return hb_front < 0 ? LLONG_MIN : 2 * (kn * (long long) g.in_len - ((long long) g.n_in - g.in_len)) - 2 * kHbfTapsMax - 8;
}

void Engine::launch_stage(size_t s, long long a, long long b, const PolyState& ps, const SrcView& src,
	const DstView& dst_in, void* stream)
{
	const StagePlan& sp = plan_.stages[s];
	const StageDev& d = dev_[s];
	DstView dst = dst_in;
	// emitted sample q is sample q + out_skip of the stage's stream function (fractional-latency chains
	// only): compute the shifted range, store it out_skip positions earlier
	a += sp.out_skip;
	b += sp.out_skip;
	dst.off -= sp.out_skip;
	switch (sp.desc.kind)
	{
	case kConv:
		launch_conv_stage(s, -1, a, b, src, dst, stream);
		break;
	case kFrac:
		if (sp.whole)
		{
			WholeLaunch L;
			L.in_step = sp.in_step; L.out_step = sp.out_step; L.flen = sp.flen;
			L.fl2 = sp.fl2; L.fll = sp.fll;
			L.pos0 = sp.pos0;
			L.table = d.table;
			// transposed table in output order (built for whole-step stages at construction): usable when
			// in_step is invertible mod out_step and the product phase * inverse stays in 32 bits
			L.wtab = nullptr; L.inv_in = 0;
			if (d.wtab != nullptr && sp.out_step < 46340)
			{
				long long inv = 0;
				for (long long k = 1; k < sp.out_step; k++) // (out_step is a few hundred at most; once per call)
					if (k * (sp.in_step % sp.out_step) % sp.out_step == 1) { inv = k; break; }
				if (sp.out_step == 1) inv = 0;
				if (inv != 0 || sp.out_step == 1) { L.wtab = d.wtab; L.inv_in = (int) inv; }
			}
			L.a = a; L.b = b;
			// as large as keeps the tile's input span within 32 KB of LDS (four to five workgroups per CU): a
			// thread's set-up -- a 64-bit division and its row fetch -- is paid once per tile (44100 -> 96000,
			// 1024 channels: tile 1024 0.237 ms, 2048 0.191, 4096 0.156)
			L.tile = opt(kWholeTile);
			L.span_max = (int) ((long long) L.tile * sp.in_step / sp.out_step) + sp.flen + 4 + 32;
			while ((L.span_max > 4096 && L.tile > 1024) || (L.span_max > 12288 && L.tile > 64))
			{
				L.tile /= 2;
				L.span_max = (int) ((long long) L.tile * sp.in_step / sp.out_step) + sp.flen + 4 + 32;
			}
			L.nch = nchw_;
			L.src = src; L.dst = dst;
			launch_whole(L, stream);
		}
		else
		{
			PolyLaunch L;
			L.flen = sp.flen; L.fl2 = sp.fl2; L.fll = sp.fll; L.fracs = sp.bank->fracs;
			L.table = d.table;
			L.ssr = sp.ssr; L.dsr = sp.dsr;
			L.rpos0 = ps.rpos; L.fpos0 = ps.pos_frac;
			L.counter0 = ps.in_counter; L.pos_int0 = ps.in_pos_int; L.shift = ps.pos_shift;
			L.a = a; L.b = b; L.nch = nchw_;
			// tile of 64 outputs spans at most 64*Src/Dst + taps input samples (+ slack for the
			// counter's rounding)
			L.span_max = opt(kPolyTiled) ?
				(int) std::ceil(64.0 * sp.ssr / sp.dsr) + sp.flen + 4 + 8 : 0; // (+ kPolyPad zeros)
			L.pitch = poly_row_pitch(L.span_max, sp.ssr / sp.dsr);
			L.front = L.span_max > 0 && L.span_max - 8 <= 16 * 12; // (kPolyPad, kPolyNV)
			if (L.front && ch0_ == 0) stat_[kPolyFront]++;
			L.src = src; L.dst = dst;
			launch_poly(L, stream);
		}
		break;
	case kHBUp:
	case kHBDown:
	{
		HBLaunch L;
		L.ntaps = sp.hb_n;
		if (sp.hb_n > 16) throw std::runtime_error("half-band filter too long");
		for (int i = 0; i < 16; i++) L.taps[i] = i < sp.hb_n ? sp.hb_taps[i] : 0.0;
		L.a = a; L.b = b;
		L.tile = opt(kHbTile);
		L.nch = nchw_;
		L.src = src; L.dst = dst;
		take_carried_tail(L.tail, &L.carry_tail);
		if (sp.desc.kind == kHBUp) launch_hbup(L, stream);
		else launch_hbdown(L, stream);
		break;
	}
	}
}

int Engine::process_planar(const void* d_in, int in_fmt, long long in_stride, int l, void* d_out,
	int out_fmt, long long out_stride, void* stream)
{
	// The first stage decodes the caller's samples as it loads them, the last one encodes as it stores (src_load /
	// dst_store: no staging copy, 2-4 bytes per sample at the HBM edge) -- WHERE that stage's kernel exists for PCM
	// views: the streaming kernels and the generic convolver (pcm_fused_in / pcm_fused_out).  The compile-time-sized
	// convolvers are built for fp64 views only; a PCM side in front of / behind one of them has to arrive as fp64 rows
	// (r8b_capi.cpp batch_process_pcm decodes / encodes through the object's staging rows, one extra pass over that
	// side).  Refused here, for every caller, instead of failing inside a launcher.
	if (in_fmt != kPcmF64 && !pcm_fused_in())
		throw std::runtime_error("planar PCM input in front of a compile-time-sized convolver: decode it into fp64 rows "
			"first (r8b_batch_process_pcm does)");
	if (out_fmt != kPcmF64 && !pcm_fused_out())
		throw std::runtime_error("planar PCM output behind a compile-time-sized convolver: take fp64 rows and encode "
			"them (r8b_batch_process_pcm does)");
	struct Reset
	{
		Engine& e;
		~Reset() { e.io_in_fmt_ = e.io_out_fmt_ = kPcmF64; }
	} reset{*this};
	io_in_fmt_ = in_fmt;
	io_out_fmt_ = out_fmt;
	return process(static_cast<const double*>(d_in), in_stride, l, static_cast<double*>(d_out),
		out_stride, stream);
}

int Engine::process(const double* d_in, long long in_stride, int l, double* d_out,
	long long out_stride, void* stream, int active)
{
	if (l < 0 || l > plan_.max_in) throw std::runtime_error("input length exceeds MaxInLen");
	if (active == 0) active = nch_;
	if (active < 0 || active > nch_ || (active != nch_ && (active & 1) != 0))
		throw std::runtime_error("active channel count must be even, or the object's channel count");
	// (a channel that a step left out has a hole in its rings: it cannot come back before clear())
	if (active > act_min_) throw std::runtime_error("active channel count grew since the last clear()");
	if (l == 0) return 0;
	act_min_ = active;
	struct Active
	{
		Engine& e;
		~Active() { e.act_ = e.nch_; }
	} whole{*this};
	act_ = active;
	// raw device pointers from a foreign host: refuse what would read or write outside the rows
	if (d_in == nullptr || d_out == nullptr) throw std::runtime_error("null device pointer");
	if (nch_ > 1 && (in_stride < l || in_stride < 0))
		throw std::runtime_error("in_stride is smaller than the number of input samples per row");
	{
		// what this call will return (the plan is advanced only by the stage loop below)
		ChainPlan probe = plan_;
		int n = l;
		for (StagePlan& sp : probe.stages)
		{
			long long a, b;
			sp.step(n, &a, &b, nullptr);
			n = (int) (b - a);
		}
		if (plan_.stages.empty()) n = l;
		if (nch_ > 1 && out_stride < n)
			throw std::runtime_error("out_stride is smaller than the number of output samples of "
				"this call (" + std::to_string(n) + "): rows would overlap");
	}
	if ((io_in_fmt_ == kPcmF64 && ((size_t) d_in & 7) != 0) || (io_out_fmt_ == kPcmF64 && ((size_t) d_out & 7) != 0))
		throw std::runtime_error("fp64 buffers must be 8-byte aligned");
	DevGuard guard(device_);
	const size_t ns = plan_.stages.size();
	if (ns == 0)
	{
		// Src == Dst: the reference hands the input back (reference CDSPResampler.h:534-535);
		// the batch entry copies it into the caller's output buffer
		TailLaunch T;
		T.src.ring = d_in; T.src.ring_stride = 0; T.src.ring_mask = 0;
		T.src.cur = d_in; T.src.cur_stride = in_stride; T.src.cur_base = 0;
		T.src.cur_fmt = kPcmF64;
		if (io_in_fmt_ != kPcmF64 || io_out_fmt_ != kPcmF64)
			throw std::logic_error("pass-through of PCM buffers goes through the staging rows");
		T.p0 = 0; T.p1 = l;
		T.ring = d_out; T.ring_stride = out_stride; T.ring_mask = -1;
		T.nch = act_;
		launch_tail(T, stream);
		return l;
	}
	// Pass 1 (host only): advance the plan, stage group by stage group; what each launch has to produce.
	struct Rec
	{
		size_t s;
		int glen;
		long long m_prev, a, b, wa, wb;
		PolyState ps;
		bool fused, work;
	};
	std::vector<Rec> recs;
	int n = l;
	for (size_t s = 0; s < ns; s++)
	{
		StagePlan& sp = plan_.stages[s];
		Rec r;
		r.s = s;
		r.m_prev = sp.m;
		sp.step(n, &r.a, &r.b, &r.ps);
		// stages [s, s+glen) are executed by one launch: convolver + whole-step interpolator, or a
		// run of half-band up-samplers
		r.glen = form_[s].glen;
		r.fused = r.glen > 1;
		r.wa = r.a;
		r.wb = r.b;
		for (int g = 1; g < r.glen; g++)
		{
			long long ga, gb;
			plan_.stages[s + g].step((int) (r.wb - r.wa), &ga, &gb, nullptr);
			r.wa = ga;
			r.wb = gb;
		}
		r.work = r.fused ? r.wb > r.wa : r.b > r.a;
		n = (int) (r.fused ? r.wb - r.wa : r.b - r.a);
		recs.push_back(r);
		s += r.glen - 1;
	}
	// Pass 2: the launches, for the channel window [ch0_, ch0_ + nchw_).
	auto launch_rec = [&](const Rec& r)
	{
		const size_t s = r.s;
		const StagePlan& sp = plan_.stages[s];
		const size_t last = s + r.glen - 1; // stage whose output this launch produces
		SrcView src;
		src.ring = dev_[s].ring + (long long) ch0_ * dev_[s].ring_size;
		src.ring_stride = dev_[s].ring_size;
		src.ring_mask = dev_[s].ring_size - 1;
		if (s == 0)
		{
			src.cur = d_in + (long long) ch0_ * in_stride; // (windows are used with fp64 buffers only)
			src.cur_stride = in_stride;
			src.cur_base = r.m_prev;
			src.cur_fmt = io_in_fmt_;
		}
		else
		{
			src.cur = nullptr;
			src.cur_stride = 0;
			src.cur_base = LLONG_MAX;
			src.cur_fmt = kPcmF64;
		}
		DstView dst;
		if (last + 1 == ns)
		{
			dst.p = d_out + (long long) ch0_ * out_stride;
			dst.stride = out_stride;
			dst.mask = -1;
			dst.off = -(r.fused ? r.wa : r.a);
			dst.fmt = io_out_fmt_;
		}
		else
		{
			dst.p = dev_[last + 1].ring + (long long) ch0_ * dev_[last + 1].ring_size;
			dst.stride = dev_[last + 1].ring_size;
			dst.mask = dev_[last + 1].ring_size - 1;
			dst.off = 0;
			dst.fmt = kPcmF64;
		}
		if (s == 0)
		{
			tail_done_ = false;
			// History for the next call: the last history() samples of the stream go into the OTHER ring (this call's
			// kernels may still be reading the current one).  The fast convolver does the copy itself (tail_done_);
			// otherwise it is CARRIED by the call's next half-band launch -- stage 0's own or a later one's: extra
			// workgroups of that grid, nobody reads the other ring in this call -- and only when the call has none by
			// the copy kernel (k_tail, below and behind the stage loop).  (fp64 caller rows, the whole batch in one
			// launch: a later stage's kernel is the fp64 build, a channel window has its own tail.)
			carry_ = false;
			carry_tail_.src = src;
			carry_tail_.p1 = sp.m;
			carry_tail_.p0 = sp.m - stage_history(0);
			if (carry_tail_.p0 < 0) carry_tail_.p0 = 0;
			carry_tail_.ring = dev_[0].ring_alt + (long long) ch0_ * dev_[0].ring_size;
			carry_tail_.ring_stride = dev_[0].ring_size;
			carry_tail_.ring_mask = dev_[0].ring_size - 1;
			carry_tail_.nch = nchw_;
			carry_ = opt(kFoldTail) != 0 && src.cur_fmt == kPcmF64 && nchw_ == act_;
		}
		if (r.work)
		{
			const bool timing = opt(kTiming) != 0;
			void *e0 = nullptr, *e1 = nullptr;
			if (timing)
			{
				e0 = get_event(dev_[s]);
				e1 = get_event(dev_[s]);
				dev_event_record(e0, stream);
			}
			if (r.fused && sp.desc.kind == kConv) launch_fused(s, r.wa, r.wb, src, dst, stream);
			else if (form_[s].group == kGroupHbConv) launch_hbconv(s, r.wa, r.wb, src, dst, stream);
			else if (r.fused && sp.desc.kind == kHBDown) launch_dcascade(s, r.glen, r.wa, r.wb, src, dst, stream);
			else if (r.fused) launch_cascade(s, r.glen, r.wa, r.wb, src, dst, stream);
			else launch_stage(s, r.a, r.b, r.ps, src, dst, stream);
			if (timing)
			{
				dev_event_record(e1, stream);
				dev_[s].pending.emplace_back(e0, e1);
				// (what the launcher really started for this stage: rocprofv3's name for it)
				if (const char* sym = launch_symbol_last()) dev_[s].symbol = sym;
				// (one (in, out) count per call, however many channel windows it is launched in)
				if (ch0_ == 0)
				{
					dev_[s].t_in += (long long) (sp.m - r.m_prev);
					dev_[s].t_out += r.fused ? r.wb - r.wa : r.b - r.a;
				}
			}
		}
		if (s == 0 && tail_done_) carry_ = false;
		if (s == 0 && !tail_done_ && !carry_)
		{
			launch_tail(carry_tail_, stream);
			if (ch0_ == 0) stat_[kTailLaunches]++;
		}
	};
	for (const Rec& r : recs)
	{
		ensure_ring(r.s);
		if (r.s + r.glen < ns) ensure_ring(r.s + r.glen);
	}
	ch0_ = 0;
	nchw_ = act_;
	for (size_t i = 0; i < recs.size(); i++)
	{
		// A convolver followed by the polynomial interpolator (non-whole-step ratios, 44100 -> 44101): two launches
		// with the convolver's whole 2x stream between them -- 268 MB for BASELINE's batch, written to HBM and read
		// back.  Walked in channel groups whose stream (<= ~96 MB) stays in the 256 MB Infinity Cache between the
		// two launches, the interpolator reads it from there (reference CDSPFracInterpolator.h:1069-1179 behind
		// CDSPBlockConvolver.h:252-354).  Channels are independent, so results do not change.
		const Rec& r = recs[i];
		int groups = 1;
		if (i + 1 < recs.size() && opt(kPolyGroups) && !r.fused && !recs[i + 1].fused && r.work && recs[i + 1].work &&
			plan_.stages[r.s].desc.kind == kConv && plan_.stages[recs[i + 1].s].desc.kind == kFrac &&
			!plan_.stages[recs[i + 1].s].whole && io_in_fmt_ == kPcmF64 && io_out_fmt_ == kPcmF64)
		{
			// (the groups of an object of form_nch() channels -- a shard walks its own channels in the batch's windows)
			const double between = 8.0 * (double) form_nch() * (double) (r.b - r.a);
			const double cap = opt(kPolyGroups) > 1 ? 1024.0 * opt(kPolyGroups) : 96.0 * 1048576.0;
			groups = (int) std::ceil(between / cap);
			// (whole channel pairs per group, at least 256 pairs each: smaller launches do not fill the chip)
			// (an explicit cap -- tests -- may cut down to single pairs)
			const int min_per = opt(kPolyGroups) > 1 ? 2 : 512;
			while (groups > 1 && (form_nch() / groups) < min_per) groups--;
		}
		if (groups <= 1)
		{
			launch_rec(r);
			continue;
		}
		const int per = ((form_nch() + groups - 1) / groups + 1) & ~1;
		for (int c0 = 0; c0 < act_; c0 += per)
		{
			ch0_ = c0;
			nchw_ = std::min(per, act_ - c0);
			launch_rec(r);
			launch_rec(recs[i + 1]);
		}
		ch0_ = 0;
		nchw_ = act_;
		i++;
	}
	if (carry_)
	{
		// (no launch of this call could carry the history copy)
		carry_ = false;
		launch_tail(carry_tail_, stream);
		stat_[kTailLaunches]++;
	}
	if (ns > 0) std::swap(dev_[0].ring, dev_[0].ring_alt);
	return n;
}

void Engine::launch_hbconv(size_t s, long long wa, long long wb, const SrcView& src, const DstView& dst, void* stream)
{
	// (no skipped outputs to shift by, as launch_stage does: the form exists in linear-phase chains only)
	const long long next_raw = launch_conv_stage(s + 1, (long long) s, wa, wb, src, dst, stream);
	// History for the next call (stage 0: the caller's buffer is gone then): the raw stream from where the next call's
	// first block starts reading -- not the whole stage_history() the pending copy was set up with
	if (s == 0 && next_raw != LLONG_MIN && (carry_ || !tail_done_))
	{
		long long p0 = std::max(carry_tail_.p0, next_raw);
		p0 = std::min(p0, carry_tail_.p1);
		carry_tail_.p0 = p0 < 0 ? 0 : p0;
	}
}

// input samples a stage must keep from earlier calls.  A run of half-band decimators executed as
// one kernel looks back over the accumulated filter spans of the whole run.
long long Engine::hbconv_history(size_t s) const
{
	return 2LL * plan_.stages[s + 1].history() + 4 * kHbfTapsMax + 64;
}

long long Engine::stage_history(size_t s) const
{
	const StagePlan& sp = plan_.stages[s];
	if (sp.desc.kind != kHBDown) return sp.history();
	// (decimator + convolver as one launch: the convolver's history, in raw samples, + the decimator's own reach with its
	// taps rounded up + the samples the decimator has taken without an output yet)
	if (form_[s].group == kGroupHbConv) return hbconv_history(s);
	long long span = 0;
	int g = 0;
	while (s + g < plan_.stages.size() && plan_.stages[s + g].desc.kind == kHBDown && g < kMaxCascade)
	{
		const int T = hb_tap_width(plan_.stages[s + g].hb_n);
		span += (long long) (2 * T - 1) << g;
		g++;
	}
	return std::max<long long>(sp.history(), 2 * span + (2LL << g) + 64);
}

// What the descriptor of a run of half-band stages [s, s + glen), up or down, starts with: the stages' taps, rounded up to
// the kernels' widths, and -- chains with a fractional latency -- their skipped outputs.  A stage emits its stream from
// output out_skip on: between the stages of the run that is HBCascadeLaunch::skip; for the last one, as in launch_stage,
// the range [*fa, *fb) is shifted and stored out_skip earlier (dst->off)
static void hb_run_open(HBCascadeLaunch& L, const ChainPlan& plan, size_t s, int glen, long long* fa, long long* fb, DstView* dst)
{
	L.nst = glen;
	L.has_skip = 0;
	for (int g = 0; g < kMaxCascade; g++)
	{
		L.ntaps[g] = 0;
		L.skip[g] = 0;
		for (int k = 0; k < 14; k++) L.taps[g][k] = 0.0;
	}
	for (int g = 0; g + 1 < glen; g++)
	{
		L.skip[g] = (int) plan.stages[s + g].out_skip;
		if (L.skip[g] != 0) L.has_skip = 1;
	}
	const long long sk_last = plan.stages[s + glen - 1].out_skip;
	*fa += sk_last;
	*fb += sk_last;
	dst->off -= sk_last;
	for (int g = 0; g < glen; g++)
	{
		const StagePlan& sp = plan.stages[s + g];
		if (sp.hb_n > 14) throw std::runtime_error("half-band filter too long");
		L.ntaps[g] = hb_tap_width(sp.hb_n);
		for (int k = 0; k < sp.hb_n; k++) L.taps[g][k] = sp.hb_taps[k];
	}
}

void Engine::launch_dcascade(size_t s, int glen, long long fa, long long fb, const SrcView& src,
	const DstView& dst_in, void* stream)
{
	HBCascadeLaunch L;
	DstView dst = dst_in;
	hb_run_open(L, plan_, s, glen, &fa, &fb, &dst);
	L.a = fa; L.b = fb;
	// last-stage outputs per workgroup: about 4096 first-stage input samples -- fewer where the stages' halos, doubled
	// stage by stage, would not leave that much of the LDS (run_len admits only runs that fit at kHbdMinTile)
	int tile = std::max(kHbdMinTile, opt(kHbdSpan) >> glen);
	while (tile > kHbdMinTile && hbd_lds_doubles(L.ntaps, glen, tile, nullptr, nullptr) * sizeof(double) > (size_t) kLdsMaxBytes)
		tile >>= 1;
	L.tile = tile;
	hbd_lds_doubles(L.ntaps, glen, tile, &L.buf, &L.buf2);
	L.pair_ok = 0;
	L.in_end = plan_.stages[s].m;
	L.nch = nchw_;
	L.src = src; L.dst = dst;
	take_carried_tail(L.tail, &L.carry_tail);
	launch_hbdcascade(L, stream);
}

void Engine::launch_cascade(size_t s, int glen, long long fa, long long fb, const SrcView& src,
	const DstView& dst_in, void* stream)
{
	HBCascadeLaunch L;
	DstView dst = dst_in;
	hb_run_open(L, plan_, s, glen, &fa, &fb, &dst);
	hbc_fill_ranges(L);
	L.a = fa; L.b = fb;
	// last-stage outputs per workgroup: a multiple of 2^glen.  A tile costs ~1.7 us of a CU
	// whatever its size (six dependent phases), so large batches take 8192 (51 KB LDS, 3
	// workgroups per CU: 0.19 vs 0.22 ms on cfg5 x 1024 channels) and small ones 4096, which
	// keeps every CU busy
	int want = opt(kHbcTile);
	if (want == 0) want = (fb - fa + 8191) / 8192 * (long long) form_nch() >= 256 * 6 ? 8192 : 4096;
	int tile = 1 << glen;
	while (tile < want) tile <<= 1;
	L.tile = tile;
	if (tile == 8192 && ch0_ == 0) stat_[kHbcTile8192]++;
	L.buf = tile / 2 + 96;  // largest intermediate stream of a tile (input of the last stage)
	L.buf2 = tile / 4 + 96; // the one before it (the buffers alternate)
	L.nch = nchw_;
	L.src = src; L.dst = dst;
	L.in_end = plan_.stages[s].m;
	// 16-byte stores of output pairs: output q is even for the first of an (even, odd) pair, whose element
	// index is even when the offset is (1); with an odd offset the aligned pairs are (odd, next even) (2)
	L.pair_ok = dst.fmt == kPcmF64 && ((size_t) dst.p & 15) == 0 && (dst.stride & 1) == 0 ?
		((dst.off & 1) == 0 ? 1 : 2) : 0;
	take_carried_tail(L.tail, &L.carry_tail);
	launch_hbcascade(L, stream);
}

// The interpolator of a chain with a fractional latency emits sample j as sample q = j + out_skip of its stream, whose
// position is q In + pos0 (reference CDSPFracInterpolator.h:721-752, 991-1060); its input sample i is the convolver's
// output t = i + out_skip of THAT stage.  With j0 In = pos0 (mod Out) -- In and Out are coprime -- and m = (j0 In - pos0)
// / Out, floor((q In + pos0) / Out) = floor((q + j0) In / Out) - m and the phases agree: the stream is the canonical one
// (position J In, start phase 0) renumbered, J = j + out_skip_w + j0, read from convolver outputs floor(J In / Out) + d,
// d = out_skip_c - m.
Engine::FusedShift Engine::fused_shift(size_t s) const
{
	const StagePlan& c = plan_.stages[s];
	const StagePlan& w = plan_.stages[s + 1];
	FusedShift f;
	f.js = 0; f.d = 0; f.t_zero = 0;
	if (c.out_skip == 0 && w.out_skip == 0 && w.pos0 == 0) return f;
	const long long In = w.in_step, Out = w.out_step;
	long long j0 = 0;
	while (j0 < Out && (j0 * In) % Out != (long long) w.pos0 % Out) j0++;
	if (j0 >= Out) throw std::logic_error("fused_shift: the interpolator's start phase has no canonical output");
	const long long m = (j0 * In - w.pos0) / Out;
	f.js = w.out_skip + j0;
	f.d = c.out_skip - m;
	f.t_zero = (int) c.out_skip;
	return f;
}

void Engine::fill_conv(size_t s, ConvLaunch& L, const SrcView& src) const
{
	const StagePlan& sp = plan_.stages[s];
	const StageDev& d = dev_[s];
	const ConvGeom& g = sp.cg;
	L.up = g.up; L.down = g.down; L.fl2 = g.fl2; L.bl2 = g.bl2; L.in_len = g.in_len;
	L.rot = 0; L.fl2r = g.fl2;
	L.n_in = g.n_in; L.n_out = g.n_out;
	L.blk_stride = g.in_len;
	L.blk_offset = 0;
	// aligned 16-byte loads of sample pairs need even positions on every side of the selection
	L.vec_ok = src.cur_fmt == kPcmF64 && (src.cur == nullptr || (((size_t) src.cur & 15) == 0 &&
		(src.cur_stride & 1) == 0 && (src.cur_base & 1) == 0)) && (src.ring_stride & 1) == 0 &&
		((g.in_len / g.up) & 1) == 0 ? 1 : 0;
	L.inplace = generic_conv_two_arrays(g) || generic_conv_big(g) ? 0 : 1;
	L.work = nullptr; L.work_slots = 0;
	L.up_pow2 = g.up_pow2 ? 1 : 0;
	L.down_pow2 = g.down_pow2 ? 1 : 0;
	L.n_fwd = (int) d.fwd_radix.size();
	L.n_inv = (int) d.inv_radix.size();
	if (L.n_fwd > kMaxPasses || L.n_inv > kMaxPasses)
		throw std::runtime_error("transform plan too deep");
	for (int i = 0; i < L.n_fwd; i++) L.fwd_radix[i] = d.fwd_radix[(size_t) i];
	for (int i = 0; i < L.n_inv; i++) L.inv_radix[i] = d.inv_radix[(size_t) i];
	L.H = d.H; L.Hc = d.Hc; L.tw = d.tw; L.tw_len = d.tw_len; L.spec = d.spec; L.spec2 = d.spec2; L.hp = d.hp; L.ptw = d.ptw;
	L.t_zero = 0;
	L.nch = nchw_;
	// (short transforms: fewer threads per block -- a 64-point transform on 256 threads is four waves
	// meeting at barriers with nothing to do)
	{
		int th = 64;
		while (th < opt(kConvThreads) && th * 8 < std::max(g.n_in, g.n_out)) th *= 2;
		L.threads = std::min(std::min(th, opt(kConvThreads)), 256); // (the kernels are built for <= 256)
	}
	L.src = src;
	L.tail_ring = nullptr; L.tail_p0 = L.tail_p1 = 0;
	L.tail_flags = 0; L.tail_bf = 0; L.tail_c0 = L.tail_c1 = 0;
	if (s == 0 && opt(kFoldTail))
	{
		// stage 0 on the fast path: let the kernel keep the history (see process())
		const StagePlan& sp0 = plan_.stages[0];
		L.tail_ring = dev_[0].ring_alt + (long long) ch0_ * dev_[0].ring_size;
		L.tail_p1 = sp0.m;
		L.tail_p0 = sp0.m - stage_history(0);
		if (L.tail_p0 < 0) L.tail_p0 = 0;
	}
}

// Block anchoring of a fused pair (convolver s, whole-step interpolator s + 1): blocks start S virtual samples apart,
// block 0's first fresh sample sits at virtual position off.  Constants of the object (its options included).
void Engine::fused_blocking(size_t s, long long* S_out, long long* off_out) const
{
	const StagePlan& c = plan_.stages[s];
	const StagePlan& w = plan_.stages[s + 1];
	const StageDev& dw = dev_[s + 1];
	const int in_len = c.cg.in_len, fl2c = c.cg.fl2, up = c.cg.up;
	const long long In = w.in_step;
	const bool pair_two = form_[s].fused == kFusedPair2;
	// Blocks start S virtual samples apart with S = in_len - (interpolator taps, rounded up to
	// the up factor): the valid ranges [k*S - fl2, k*S - fl2 + in_len) of consecutive blocks
	// overlap by at least flen-1 convolver outputs, so each interpolator tap window lies inside
	// one block.  An output belongs to the FIRST block that contains its window.  That block's
	// input is complete whenever the reference has emitted the output (its latency covers one
	// whole block of in_len >= S samples), so block contents -- and therefore the stream -- do
	// not depend on how the input is cut into calls.
	long long S = in_len - (w.flen + up - 1) / up * up;
	// keep block starts on even input positions (pairs of samples load as 16 bytes)
	while ((S / up) & 1) S -= up;
	// Two-phase pair kernel: whole output GROUPS per block.  A group is Out consecutive outputs (In convolver
	// samples); the kernel's threads own phase pairs and take the groups of a block in nsets interleaved sets.
	// With S = G In and block 0 shifted by `off` so that (end of a block's valid run - right half of the
	// window) is a multiple of In, every block owns exactly G whole groups starting at phase 0: no partly
	// filled first / last group, and with G a multiple of nsets every set takes G / nsets groups (cfg2: 18
	// groups, 3 sets: 6 rounds per thread instead of 7 for 0.4 % more blocks).  Blocks stay anchored at
	// absolute positions (k S + off), so chunk invariance is untouched.  Only taken when it costs < 3 % of
	// the block's valid run.
	long long off = 0;
	if (pair_two && opt(kAlignGroups))
	{
		long long G = S / In;
		while (G > 0 && (G * In) % up != 0) G--;
		const long long G2 = G - G % dw.nsets;
		if (G2 > 0 && (G2 * In) % up == 0 && G2 * In * 100 >= S * 98) G = G2;
		if (G > 0 && G * In * 100 >= S * 97)
		{
			// (chains with a fractional latency: the canonical stream sits fused_shift().d convolver outputs later)
			const long long r = (((long long) in_len - fl2c - w.fl2 - fused_shift(s).d) % In + In) % In;
			long long o = -r;
			for (int t = 0; t < up && o % up != 0; t++) o -= In;
			if (o % up == 0)
			{
				S = G * In;
				off = o;
			}
		}
	}
	*S_out = S;
	*off_out = off;
}

static long long ceil_div_nonneg(long long a, long long b) { return a <= 0 ? 0 : (a + b - 1) / b; }

void Engine::launch_fused(size_t s, long long wa, long long wb, const SrcView& src,
	const DstView& dst_in, void* stream)
{
	const StagePlan& c = plan_.stages[s];
	const StagePlan& w = plan_.stages[s + 1];
	// Chains with a fractional latency (fused_shift): everything below works on the CANONICAL stream -- output J at
	// position J In, phase J In mod Out, its window starting at convolver output floor(J In / Out) + D -- of which the
	// call's emitted outputs [wa, wb) are J - js; they are stored js columns (ring slots) earlier.  (js = D = 0 in
	// linear-phase chains.)
	const FusedShift fs = fused_shift(s);
	const long long D = fs.d;
	wa += fs.js;
	wb += fs.js;
	DstView dst = dst_in;
	dst.off -= fs.js;
	ConvxLaunch X;
	fill_conv(s, X.c, src);
	X.c.t_zero = fs.t_zero;
	X.c.a = 0; X.c.b = 0;
	X.c.dst = dst; // unused in fused mode
	X.in_step = w.in_step; X.out_step = w.out_step; X.flen = w.flen;
	X.fl2w = w.fl2; X.fllw = w.fll;
	X.table = dev_[s + 1].table;
	X.wtab = dev_[s + 1].wtab;
	X.wa = wa; X.wb = wb;
	X.wdst = dst;
	const int in_len = c.cg.in_len, fl2c = c.cg.fl2, up = c.cg.up;
	const long long In = w.in_step, Out = w.out_step;
	X.c.blk_offset = 0;
	const StageDev& dw = dev_[s + 1];
	const StageForm& f = form_[s];
	const int run_off = f.run_off;
	const bool pair_two = f.fused == kFusedPair2;
	X.run_off = run_off;
	X.ptab = dw.ptab; X.ctab = dw.ctab; X.nsets = dw.nsets;
	long long S = 0, off = 0;
	fused_blocking(s, &S, &off);
	X.c.blk_stride = (int) S;
	X.c.blk_offset = (int) off;
	if (((S / up) & 1) != 0 || ((off / up) & 1) != 0) X.c.vec_ok = 0;
	auto owner = [&](long long j) // first block whose valid range ends after the window of j
	{
		const long long v = j * In / Out + D + w.fl2 + fl2c - in_len - off;
		return v < 0 ? 0 : v / S + 1;
	};
	// outputs of block k, not clipped to the call: [first output whose window block k - 1 does not hold, first one
	// block k does not hold either)
	auto block_jlo = [&](long long k)
	{
		return k == 0 ? 0 : ceil_div_nonneg(((k - 1) * S + off - fl2c + in_len - w.fl2 - D) * Out, In);
	};
	auto block_jhi = [&](long long k) { return ceil_div_nonneg((k * S + off - fl2c + in_len - w.fl2 - D) * Out, In); };
	no_optional_forms(X);
	X.half_fused = f.half_fused;
	// Every block once (LastBlock): the block that holds the call's last output is computed ONCE -- what it holds beyond
	// wb waits in the park buffer for the next call(s) (kBlockPark: the two-phase pair form and the one-channel form of
	// the pair kernel, kFusedSolo), is written ahead into the next stage's ring (kBlockAhead) or stays in the
	// output ring (kBlockOutRing: the one-channel kernel, 16384-point blocks; as in launch_conv_stage) instead of being
	// computed again there (one block in 13.4 for BASELINE's cfg2 call, one in 7.5 for cfg3)
	const LastBlock policy = last_block(s, dst);
	const bool solo_fused = f.fused == kFusedSolo;
	if (policy == kBlockPark || policy == kBlockOutRing) ensure_park(s);
	if (policy == kBlockOutRing) X.wdst = out_ring_view(s);
	const long long ja = take_parked(s, policy, wa, wb, X); // the first output this call has to compute
	if (ja >= wb)
	{
		serve_parked(s, policy, X, wa, wb, dst, stream);
		return;
	}
	const long long kfirst = owner(ja), klast = owner(wb - 1);
	// (the next call's first block: the one behind this call's last when every block is computed once)
	const long long knext = policy != kBlockAgain ? klast + 1 : owner(wb);
	// end of what the call's last block holds, and where the interpolator's outputs are cut (kBlockPark: at the call's
	// end -- the kernel puts [wb, pend) into the park buffer by X.park_blk)
	const long long pend = policy != kBlockAgain ? block_jhi(klast) : wb;
	const long long wcut = policy == kBlockPark ? wb : pend;
	if (policy != kBlockAgain) check_last_block(s, s + 2, policy, dst, wa, wb, pend);
	if (X.c.tail_ring != nullptr && (pair_two || solo_fused) && c.cg.up_pow2)
	{
		// (r8b_convp.h cp_load: a block's window is n_in input samples ending in_len / up behind the block's start; up is
		// 1 or 2 here: convp_fused_ok)
		if (up > 2) throw std::logic_error("fused pair kernel: up-sampling factor");
		next_call_tail_p0(X.c, ((knext * S + off) >> (up > 1 ? 1 : 0)) - ((long long) c.cg.n_in - in_len / up));
	}
	double* const tail_ring = X.c.tail_ring;
	const double* const park_src = X.park_src;
	const int park_n = X.park_n;
	// the spans of block k's outputs [B.jlo, B.jhi): one phase per thread, and what the two-phase form reads instead
	auto one_phase_span = [&](SpanInfo& B, long long k)
	{
		const long long t0 = k * S + off - fl2c; // first valid time of block k
		B.jlo_mod = (int) (B.jlo % Out);
		B.ph_lo = (int) ((B.jlo * In) % Out);
		B.u_lo = (int) (B.jlo * In / Out + D - w.fll - t0);
		B.pad = 0;
	};
	auto two_phase_span = [&](SpanInfo& B, long long k)
	{
		B.pad = 0;
		if (B.jhi <= B.jlo) return;
		const long long t0 = k * S + off - fl2c;
		const long long g0 = B.jlo / Out, glast = (B.jhi - 1) / Out;
		B.ph_lo = (int) (glast - g0);
		B.pad = (int) (B.jhi - glast * Out); // the phase the block's last group ends before
		B.u_lo = (int) (In * g0 + D - w.fll - t0) + run_off;
	};
	for (long long k0 = kfirst; k0 <= klast; k0 += kConvxMaxBlocks)
	{
		const long long k1 = std::min(klast, k0 + kConvxMaxBlocks - 1);
		// (the history with the call's LAST launch: its blocks are the ones that hold the tail in registers)
		X.c.tail_ring = k1 == klast ? tail_ring : nullptr;
		// (the parked outputs of the previous call with the FIRST launch)
		X.park_src = k0 == kfirst ? park_src : nullptr;
		X.park_n = k0 == kfirst ? park_n : 0;
		X.c.k0 = k0;
		X.c.nblk = (int) (k1 - k0 + 1);
		// Walk form: enough channel pairs to fill the chip with one workgroup each (2 per CU on 256 CUs: from 128 pairs on
		// a launch is worth it) and at least two blocks to walk; the launcher ignores it where the kernel has no walk form
		X.walk = 0;
		if (pair_two && (opt(kWalk) == 2 || (opt(kWalk) == 1 && form_nch() >= 256 && X.c.nblk >= 2)))
			X.walk = opt(kWalkLen) > 0 ? std::min(opt(kWalkLen), X.c.nblk) : X.c.nblk;
		if (ch0_ == 0) stat_[kConvBlocks] += X.c.nblk;
		for (int i = 0; i < X.c.nblk; i++)
		{
			SpanInfo& B = X.blk[i];
			B.jlo = std::max(block_jlo(k0 + i), ja);
			B.jhi = std::max(std::min(block_jhi(k0 + i), wcut), B.jlo);
			one_phase_span(B, k0 + i);
			if (pair_two) two_phase_span(B, k0 + i);
		}
		// (kBlockPark, with the call's LAST launch: what its last block holds beyond the call goes into the other buffer)
		if (policy == kBlockPark && k1 == klast && pend > wb)
		{
			park_beyond(s, X, wb, pend);
			one_phase_span(X.park_blk, klast);
			if (pair_two) two_phase_span(X.park_blk, klast);
		}
		if (pair_two)
		{
			// (blocks the launcher put on the walk body: counted per engine, once per call like conv_blocks)
			const long long w0 = launch_walk_blocks();
			launch_convp(X, f.mode, stream);
			if (ch0_ == 0) stat_[kWalkBlocks] += launch_walk_blocks() - w0;
		}
		else if (f.mode == kConvpModeNone)
			// (fuse_latency_ok admits a complex spectrum only where the two-phase tables exist)
			throw std::logic_error("fused launch: complex kernel spectrum without the two-phase tables");
		else if (f.fused == kFusedConvx) launch_convx(X, f.mode, stream);
		else launch_convp(X, f.mode, stream);
		if (X.c.tail_ring != nullptr) tail_done_ = true;
	}
	if (policy == kBlockOutRing) ring_to_rows(s, wa, wb, dst, stream);
	commit_last_block(s, policy, wb, pend);
}

} // namespace r8bhip

// The table unit travels in this translation unit: the build files and every test program name the library's sources one by
// one, and a suite older than the unit, run over these sources, must still get a whole library from the four it knows.
// r8b_conv_tables.cpp stays a translation unit of its own all the same -- tests/cxx_conv_tables.cpp links it with the
// designer and the plan alone -- and comes last here, so that nothing above sees more of it than its header.
#include "r8b_conv_tables.cpp"
