// r8b_engine.h -- N-channel batch resampler: host schedule (r8b_plan.h) + device state + launches.
//
// One Engine = `nch` independent streams that share one ChainPlan.  process() mirrors
// r8b::CDSPResampler::process (reference CDSPResampler.h:559-575): it walks the stage chain, but
// instead of ping-ponging host buffers it enqueues one position-addressed kernel per stage on a
// HIP stream.  Stage-to-stage streams live in per-channel rings in HBM; the first stage reads the
// caller's device buffer directly (plus a short history ring), the last stage writes the caller's
// device buffer directly.
#ifndef R8B_ENGINE_H
#define R8B_ENGINE_H

#include <utility>
#include <string>
#include <vector>

#include "r8b_convp_mode.h"
#include "r8b_devblock.h"
#include "r8b_launch.h"
#include "r8b_plan.h"

namespace r8bhip {

// The engine's options (Engine::set_option, r8b_batch_set_option), one kOptions entry each in EngineOption's order.  A
// STRUCTURAL one may change only before the first sample or after clear() (it decides where a stage's history lives, or
// how the device rounds); one not hashed stays out of config_hash (it changes neither the state nor a bit of the stream)
enum EngineOption { kConvRadix, kConvThreads, kWholeTile, kHbTile, kFuseHbd, kHbdSpan, kHbcTile, kTiming, kFastConv, kFuse,
	kFuseHb, kPolyTiled, kPolyGroups, kPairConv, kPairTwo, kFuseLatency, kPairSplit, kPairSolo, kAlignGroups, kFoldTail,
	kPark, kSoloFuse, kUp3Poly, kQuad, kHalf, kHalfFused, kFuseHbconv, kWalk, kWalkLen, kFormChannels, kOptionCount };
constexpr struct OptionDef { const char* name; int def; bool structural, hashed; } kOptions[] = {
	{ "conv_radix", 8, false, true },
	{ "conv_threads", 256, false, true },
	{ "whole_tile", 4096, false, true },
	{ "hb_tile", 1024, false, true },
	{ "fuse_hbd", 2, true, true },     // runs of half-band decimators as one kernel: 0 never, 1 always, 2 by batch size
	{ "hbd_span", 2048, false, true }, // first-stage input samples per workgroup of the decimating cascade
	{ "hbc_tile", 0, false, true },    // last-stage outputs per workgroup of the half-band cascade (0: by batch)
	{ "timing", 0, false, false },
	{ "fast_conv", 1, true, true },    // compile-time-sized convolver kernel when the geometry allows
	{ "fuse", 1, true, true },         // ... with the whole-step interpolator behind it fused in
	{ "fuse_hb", 1, true, true },      // runs of half-band up-samplers as one kernel
	{ "poly_tiled", 1, false, true },  // polynomial interpolator: 16 channels share each coefficient fetch
	// convolver + polynomial interpolator walked in channel groups (1: 96 MB between them; n > 1: n KB; 0: off).  Off:
	// measured on MI355X (profiles/r03_poly_groups.txt) the interpolator gains 2 % from reading the stream out of the
	// Infinity Cache and the convolver loses 8 % to its smaller launches (44100 -> 44101 x 1024 ch: 0.285 vs 0.280 ms)
	{ "poly_groups", 0, false, true },
	// two channels per workgroup as one complex transform (r8b_convp.h) where the geometry allows
	{ "pair_conv", 1, true, true },
	// ... with two adjacent phases per thread in the fused interpolator when it up-samples
	{ "pair_two", 1, true, true }, // (In <= Out: half the LDS reads per output, nearly all lanes busy)
	// chains with a fractional latency (minimum phase): convolver + interpolator in one launch too
	{ "fuse_latency", 1, true, true },
	{ "pair_split", 1, true, true }, // 8192 -> 16384-point 2x up-sampling blocks on the pair kernel's split form (else k_convx)
	{ "pair_solo", 1, true, true },    // 16384-point 1:1 blocks on the pair kernel's one-channel form (else k_convx)
	{ "align_groups", 1, true, true }, // ... with whole output groups per block (launch_fused)
	{ "fold_tail", 1, true, true },    // fast convolver at stage 0 keeps the input history itself
	// the call's last block of a fused pair at the end of the chain is computed once: what it holds beyond the call
	// is parked for the next one (launch_fused)
	{ "park", 1, true, true },
	// 16384-point 1:1 blocks (one-channel form of the pair kernel) with the whole-step interpolator behind them fused in
	{ "solo_fuse", 1, true, true }, // (kernel mode 18; 0: the interpolator as a launch of its own, as before round 5)
	// 3x up-sampling convolvers in the polyphase form -- one forward transform of the INPUT samples, three backward ones,
	// no stuffed zeros transformed (r8b_convp.h mode 19, ConvGeom::p3); 0: the zero-stuffing block, as before round 5
	{ "up3_poly", 1, true, true },
	// eight elements per thread (r8b_convq.h): the 2048 -> 4096-point convolver-only block pair on 512 threads (four waves
	// per SIMD instead of two); same blocks, same state, results differ from the 256-thread form by rounding
	{ "quad", 0, true, true },
	// half-array form of that block pair (r8b_convp.h cp_ha_*, kernel mode 21): the backward side's two exchanges move the
	// real parts, then the imaginary parts through an array of DOUBLES -- 32 KB, four workgroups per CU, no pass added.
	// Measured on MI355X (profiles/r06_experiments.txt item 12): 44100 -> 88200 at 1024 channels 0.1429 -> 0.1277 ms per
	// call (kernel 0.138 -> 0.118), at 256 channels -9 %, at 4096 -13 %; launches that do not fill the chip twice gain
	// nothing (64 channels: +0.5 %).  1: objects whose largest call holds at least 512 workgroups of the stage -- channel
	// pairs x blocks, Engine::half_worth -- (decided per OBJECT, never per call: the two forms do the same arithmetic on the
	// same values -- bitwise equal under host emulation -- but the device compiler contracts multiply-adds differently in
	// the two kernels, so on the GPU they agree to rounding, 4e-17 RMS, and an object must stay with one of them to remain
	// bitwise chunk invariant); 2: every object; 0: the 64 KB form
	{ "half", 1, true, true },
	// ... and of the fused two-phase block pair 2048 -> 4096 points + whole-step interpolator (kernel modes 23 / 25: the
	// array is the interpolator's run, 52 KB with flag words and twiddle table, three workgroups per CU; taken in place of
	// modes 4 / 5 and of the walk form).  Measured on cfg2 (profiles/r06_experiments.txt item 13): -1.3 ... -2.1 % per call
	// against the walk form, -4.2 % against a workgroup per block; kernel events level with the walk form.  Values as for
	// "half"
	{ "half_fused", 1, true, true },
	// a half-band decimator in front of a 4096 -> 2048-point decimating convolver taken in the convolver's load (kernel mode
	// 20: one launch, the decimator's stream never leaves LDS).  Off: measured on MI355X the fused launch takes 92.6 us
	// + a 19 us history copy against 52.5 + 42.6 us for the two launches (176400 -> 44100, 1024 ch x 16384) -- a block
	// cannot start before its 133 KB of raw samples have arrived and all workgroups ask at once: 38 000 of a block's
	// 66 000 cycles are the two staging rounds at 4.2 TB/s (profiles/r06_experiments.txt item 10); the raw-domain
	// history a call has to leave (avg 5 300 samples per channel) is 4x the convolver-domain one besides
	{ "fuse_hbconv", 0, true, true },
	// fused two-phase pair kernel in its walk form (r8b_convp.h convp_walk): a workgroup per channel pair takes the call's
	// blocks one after the other (0: a workgroup per block, as before round 5; 2: whatever the batch size -- tests)
	{ "walk", 1, false, false },
	{ "walk_len", 0, false, false },   // blocks per workgroup of the walk form (0: the launch's whole run of blocks)
	// the channel count the size-driven choices are made for (0: the object's own; Engine::form_nch): a shard of a
	// larger batch gives the batch's total, so that it runs the kernels the unsharded object runs -- the half-array forms
	// round differently from the full-array ones on the device -- and stays bitwise equal to it (BatchSharded.h)
	{ "form_channels", 0, true, true },
};

// counters since creation (Engine::stat, r8b_batch_stat), named by kCounterNames
// (clip_steps / clip_channel_steps: the process() steps the clip calls made and the sum of their active channel counts --
// r8b_capi.cpp batch_resample_clips; their ratio over channels() is the share of stage work a dropping call has left)
enum EngineCounter { kConvBlocks, kWalkBlocks, kTailLaunches, kParkCalls, kParkOnlyCalls, kPcmStagedSides, kHbcTile8192,
	kClipSteps, kClipChannelSteps, kPolyFront, kCounterCount };
constexpr const char* kCounterNames[] = { "conv_blocks", "walk_blocks", "tail_launches", "park_calls", "park_only_calls",
	"pcm_staged_sides", "hbc_tile_8192", "clip_steps", "clip_channel_steps", "poly_front" };
static_assert(std::size(kOptions) == kOptionCount && std::size(kCounterNames) == kCounterCount, "one entry per enumerator");

// What becomes of the block that holds a call's last output (Engine::last_block).  A convolver's blocks sit at fixed
// places in the stream and a call's outputs usually end inside one: that block is computed again by the next call
// (kBlockAgain), or computed once and whole, and what it holds beyond the call
//   kBlockPark    waits in the stage's park buffer (ConvxLaunch::park_*; the pair kernel at the end of the chain),
//   kBlockAhead   is written ahead into the next stage's ring (any fast kernel in the middle of the chain),
//   kBlockOutRing stays in an output ring of the stage's own, kept in park[0], from which a copy kernel takes every
//                 call's outputs to the caller's rows (the one-channel kernel at the end of the chain).
enum LastBlock { kBlockAgain, kBlockPark, kBlockAhead, kBlockOutRing };

// Which kernel form runs a stage: one record per stage (Engine::form_), filled by Engine::resolve_forms() and by nothing
// else -- at the end of construction and whenever set_option changes a value.  A constant of the object and its options;
// what belongs to a call (the destination's format in Engine::last_block, vec_ok, walk, the block range) is not here.
enum StageGroup { kGroupAlone, kGroupConvWhole, kGroupHbConv, kGroupHbRun };
enum ConvPath { kPathGeneric, kPathGenericBig, kPathConvx, kPathConvx3, kPathPair, kPathPair3, kPathPairP3 };
enum FusedForm { kFusedNone, kFusedConvx, kFusedPair1, kFusedPair2, kFusedSolo };
struct StageForm
{
	// the launch that starts at this stage runs stages [s, s + glen): alone, a convolver + the whole-step interpolator
	// behind it, a half-band decimator taken in the load of the convolver behind it, or a run of half-band stages up or
	// down.  member: no launch starts here -- the stage belongs to an earlier stage's group, and owns no ring
	StageGroup group = kGroupAlone;
	int glen = 1;
	bool member = false;
	bool hb_front_possible = false; // kGroupHbConv under SOME setting of the options (the rings are sized once)
	// a convolver:
	ConvGeom g;                     // the geometry it runs with: the plan's, or its polyphase 3x block (ConvGeom::p3)
	ConvPath path = kPathGeneric;
	FusedForm fused = kFusedNone;   // kGroupConvWhole: one-channel kernel, pair kernel with one / two phases per thread,
	                                // one-channel form of the pair kernel
	int mode = kConvpModeNone;      // what launch_convp (the pair paths) / launch_convx gets; none: nothing to launch
	int run_off = 0;                // kFusedPair2: where the interpolator's run starts in the block's array
	int quad = 0, half = 0, half_fused = 0; // ConvxLaunch's fields of these names
	LastBlock last = kBlockAgain;   // what the kernel can do with the block that holds a call's last output
	bool end = false;               // its launch writes the caller's rows
	bool parks = false;             // it owns park buffers (kBlockPark: two used in turn; kBlockOutRing: the ring)
	bool fast() const { return path != kPathGeneric && path != kPathGenericBig; }
	bool pair() const { return path == kPathPair || path == kPathPair3 || path == kPathPairP3; }
};

class Engine
{
public:
	Engine(const std::vector<StageDesc>& descs, int maxin, int nch, int device);
	Engine(const Engine&) = delete;
	Engine& operator=(const Engine&) = delete;

	// returns output samples per channel produced by this call.
	// active: the step's launches run channels [0, active) only (0: all of them).  The plan advances as ever -- it is one
	// for all channels --, the rings and park buffers of channels [active, channels()) are simply not advanced, and their
	// rows of d_out are not written.  For a caller that needs those channels no more before the next clear() (the clip
	// calls, once a clip's last output is out): a channel left behind must not be taken up again, so `active` may only
	// shrink between two clear()s.  `active` is even or channels() (the pair kernels take channels two by two); the
	// kernel forms stay those of the object (form_nch()), whatever the count: the samples of the active channels are the
	// full step's bit for bit
	int process(const double* d_in, long long in_stride, int l, double* d_out,
		long long out_stride, void* stream, int active = 0);
	// the same with PLANAR buffers of PCM samples (PcmFormat; strides in samples), converted by
	// the first stage's loads and the last stage's stores; needs at least one stage (Src != Dst)
	// can the first / last stage of the chain take planar PCM caller buffers itself?
	bool pcm_fused_in() const { return pcm_in_; }
	bool pcm_fused_out() const { return pcm_out_; }
	int process_planar(const void* d_in, int in_fmt, long long in_stride, int l, void* d_out,
		int out_fmt, long long out_stride, void* stream);
	void clear();
#ifdef R8B_TEST_HOOKS
	// TEST builds only (r8b_batch_test_skip_silence, include/r8bsrc.h): the state n zero samples fed through process()
	// would leave, without a launch -- the plan's counters by their closed forms, every ring all zero, nothing parked or
	// written ahead (park_base / park_end as clear() leaves them: the next call computes its first block whole, as after a
	// call that parked nothing).  Everything else a call works with is a function of those counters (fused_shift, the
	// block ranges, the history copy's range, HbFront::end).  Returns the outputs those calls would have returned; throws
	// for an object that has been fed, n < 0, and a chain with a polynomial interpolator
	long long test_skip_silence(long long n, void* stream);
#endif
	bool set_option(const std::string& name, int value); // false: unknown name, or a structural option changed mid-stream
	// a counter since creation by name (kCounterNames); -1: unknown name
	long long stat(const std::string& name) const;
	void bump(EngineCounter c, long long n = 1) { stat_[c] += n; } // (counters kept for the layers above: kPcmStagedSides, kClip*)

	// per-stage kernel time accumulated since the last call (only while option "timing" is 1):
	// resolves pending events, returns total milliseconds and the number of launches
	bool stage_timing(size_t stage, double* ms_sum, int* launches, std::string* kernel,
		long long* in_samples, long long* out_samples);

	// device symbol of the stage's most recent launch made while option "timing" was 1, as rocprofv3 prints it without
	// namespace and argument list ("k_convp_walk<11, 1, 4, 24>"); empty before the first one.  stage_timing's name is
	// the engine's LABEL for the stage's form ("k_convp_whole": convolver + interpolator in one launch)
	std::string stage_symbol(size_t stage) const;
	// ... and of the PCM boundary's kernels, which the layer above launches around process() (r8b_capi.cpp: side 0 the
	// ingest, 1 the egress; R8B_STAGE_PCM_IN / R8B_STAGE_PCM_OUT of include/r8bsrc.h).  timing(): option "timing" is 1
	bool timing() const { return opt(kTiming) != 0; }
	void pcm_symbol_note(int side, const char* symbol) { pcm_symbol_[side] = symbol != nullptr ? symbol : ""; }
	const std::string& pcm_symbol(int side) const { return pcm_symbol_[side]; }

	// Checkpoint of the streaming state of all channels: the plan's counters
	// and the contents of every history ring, as one host blob.  load_state() accepts only a blob
	// saved by an object of the same configuration (rates, filter parameters, MaxInLen, channel
	// count, engine options); a stream resumed from it continues bit-identically.  Both wait for
	// `stream`, the stream the process() calls were enqueued on.  state_size() is a constant of the
	// object; load_state() checks the whole blob before it changes anything.
	size_t state_size() const;
	size_t save_state(void* buf, size_t cap, void* stream);
	void load_state(const void* buf, size_t size, void* stream);

	const ChainPlan& plan() const { return plan_; }
	int channels() const { return nch_; }
	int device() const { return device_; }

private:
	// One stage's device memory, each block with its owner (DevBlock: move-only, and so is the stage), and its events
	struct StageDev
	{
		DevBlock<double> ring; // input ring of this stage, nch x ring_size
		DevBlock<double> ring_alt; // stage 0 only: second history ring (calls alternate: process() swaps the two)
		long long ring_size = 0;
		DevBlock<double> H;
		DevBlock<cd> Hc;     // complex kernel spectrum (minimum phase; generic kernel only)
		DevBlock<cd> tw;
		DevBlock<cd> spec;  // fast-path spectral constants
		DevBlock<cd> spec2; // the same per backward position (up 1 or 2)
		DevBlock<cd> hp;     // pair kernel: kernel constants of the middle pass (r8b_convp.h)
		DevBlock<cd> ptw;    // pair kernel: twiddle base powers per pass and thread
		DevBlock<cd> hp3;    // polyphase 3x form (ConvGeom::p3, r8b_convp.h mode 19): spectra of the three components
		DevBlock<cd> ptw3;   // ... and the twiddles of its 4096-point 1:1 geometry
		int tw_len = 0;
		DevBlock<double> table;
		DevBlock<double> wtab; // whole-step bank, transposed per residue class (fused kernel)
		// pair kernel, two adjacent phases per thread (mode 4): thread table and 25-tap row pairs
		DevBlock<int> ptab;
		DevBlock<double> ctab;
		int nsets = 0;
		int taps2 = 25; // entries per row: 25 (In <= Out) or 27
		// kBlockPark (ConvxLaunch::park_*): two buffers of nch x park_stride doubles used in turn (a call reads the one the
		// previous call filled while its own last block fills the other); outputs [park_base, park_end) of the stream sit
		// at indices 0 .. of buffer park_cur.  kBlockOutRing: park[0] is the ring.  kBlockAhead: the two counters alone
		DevBlock<double> park[2];
		long long park_stride = 0;
		long long park_base = 0, park_end = 0;
		int park_cur = 0;
		// generic convolver on the reference's 32768-point blocks (k_conv_big): the packed backward spectra on their way
		// between the two forward halves and the backward transform, one array of n_out doubles per workgroup of the launch
		DevBlock<double> work;
		int work_slots = 0;
		std::vector<int> fwd_radix, inv_radix;
		std::vector<std::pair<void*, void*>> pending; // (start, stop) events not yet read
		std::vector<void*> free_events;
		double ms_sum = 0.0;
		int launches = 0;
		long long t_in = 0, t_out = 0; // per-channel samples in/out over the timed launches
		std::string symbol; // device symbol of the stage's most recent timed launch (launch_symbol_last)
	};
	// The stages of an object, sized once by the constructor.  Its destructor is the one place where an object's device
	// memory and events go -- at the end of the object's life, and when the constructor throws half way, whose own
	// DevGuard is gone by the time the members are destroyed.  Two properties are kept there (~StageDevs):
	//   every free runs with the object's device current, and the caller's device is restored afterwards;
	//   it never throws, and tolerates a runtime that can no longer make the device current.
	struct StageDevs : std::vector<StageDev>
	{
		const int device;
		explicit StageDevs(int device) : device(device) {}
		~StageDevs();
	};
	void* get_event(StageDev& d);
	// Convolver + whole-step interpolator of a chain with a fractional latency (minimum phase) as ONE launch: the shifts
	// that map the interpolator's emitted outputs onto the canonical stream the fused kernels compute (launch_fused)
	struct FusedShift
	{
		long long js; // canonical output J = emitted j + js
		long long d;  // convolver output time of J's window start = floor(J In / Out) + d
		int t_zero;   // the interpolator's stream starts at this convolver output
	};
	FusedShift fused_shift(size_t s) const;
	unsigned long long config_hash() const;
	bool stage_owns_ring(size_t s) const;

	void plan_transforms();
	void ensure_ring(size_t s);
	void ensure_work(size_t s, int slots, void* stream);
	void take_carried_tail(TailLaunch& T, int* carry);
	// half-band decimator s + convolver s + 1 as ONE launch (r8b_convp.h mode 20: the decimator taken in the block's load)
	long long hbconv_history(size_t s) const;
	void launch_hbconv(size_t s, long long wa, long long wb, const SrcView& src, const DstView& dst, void* stream);
	long long launch_conv_stage(size_t s, long long hb_front, long long a, long long b, const SrcView& src,
		const DstView& dst, void* stream);
	// the resolver and its rules (nobody else asks them)
	void resolve_forms();
	ConvGeom eff_geom(size_t s) const;
	ConvPath conv_path(const ConvGeom& g) const;
	FusedForm fused_form(size_t s) const;
	bool fuse_latency_ok(size_t s) const;
	bool hbconv_possible(size_t s) const;
	int run_len(size_t s) const;
	bool half_worth(size_t s) const;
	int form_nch() const;
	void fused_blocking(size_t s, long long* S, long long* off) const;
	// the last-block policy (LastBlock) and the steps a convolver launch, fused with the interpolator or not, takes for it
	LastBlock last_block(size_t s, const DstView& dst) const;
	long long park_len_of(size_t s, bool end_of_chain) const;
	void ensure_park(size_t s);
	DstView out_ring_view(size_t s) const;
	void ring_to_rows(size_t s, long long a, long long b, const DstView& dst, void* stream);
	long long take_parked(size_t s, LastBlock policy, long long a, long long b, ConvxLaunch& X);
	void serve_parked(size_t s, LastBlock policy, const ConvxLaunch& X, long long a, long long b, const DstView& dst,
		void* stream);
	void check_last_block(size_t s, size_t next, LastBlock policy, const DstView& dst, long long a, long long b,
		long long pend) const;
	void park_beyond(size_t s, ConvxLaunch& X, long long b, long long pend) const;
	void commit_last_block(size_t s, LastBlock policy, long long b, long long pend);
	void prepare_two_phase(size_t s);
	void launch_cascade(size_t s, int glen, long long fa, long long fb, const SrcView& src,
		const DstView& dst, void* stream);
	void launch_dcascade(size_t s, int glen, long long fa, long long fb, const SrcView& src,
		const DstView& dst, void* stream);
	long long stage_history(size_t s) const;
	void fill_conv(size_t s, ConvLaunch& L, const SrcView& src) const;
	void launch_fused(size_t s, long long wa, long long wb, const SrcView& src,
		const DstView& dst, void* stream);
	void launch_stage(size_t s, long long a, long long b, const PolyState& ps, const SrcView& src, const DstView& dst,
		void* stream);

	ChainPlan plan_;
	int nch_;
	// channel window of the launches being issued (process() walks a convolver + polynomial-interpolator pair in
	// channel groups so that the stream between them stays in the 256 MB Infinity Cache; [0, nch_) otherwise)
	int ch0_ = 0, nchw_ = 0;
	// channels the current process() step runs ([0, act_): process()'s `active`; nch_ between steps), and the smallest
	// such count since clear()
	int act_ = 0, act_min_ = 0;
	int device_;
	StageDevs dev_;
	std::vector<StageForm> form_;
	// chain-wide: some stage carries fractional-latency state (minimum phase); PCM caller buffers at the two edges
	bool latency_chain_ = false, pcm_in_ = false, pcm_out_ = false;
	int opt_[kOptionCount];
	long long stat_[kCounterCount] = {};
	std::string pcm_symbol_[2];
	int opt(EngineOption o) const { return opt_[o]; }
	int io_in_fmt_ = kPcmF64, io_out_fmt_ = kPcmF64; // formats of the current call's buffers
	bool tail_done_ = false; // stage-0 history already written by the convolver kernel
	// the call's history copy while it waits for a launch to carry it (Engine::process, take_carried_tail)
	TailLaunch carry_tail_{};
	bool carry_ = false;
};

} // namespace r8bhip

#endif
