// r8b_capi.cpp -- the C ABI of include/r8bsrc.h over r8bhip::Engine.
#include "../../include/r8bsrc.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "r8b_engine.h"
// (the true-peak meter's body, for the serial host form of launch_true_peak below)
#ifndef R8B_HD
#define R8B_HD inline
#endif
#include "r8b_truepeak.h"
#include "r8b_loudness.h"

using namespace r8bhip;

namespace r8bhip {

// The true-peak launch as a loop on the host: r8b_truepeak.h's phases for every (row, tile), tid = 0 and nthr = 1, the
// "device" arrays being host memory.  WEAK: the device library links r8b_kernels.hip's strong definition (k_truepeak)
// over it and never runs this one; the host emulation of the tests has no other and so runs the kernel's very body
// without a source file of its own for it.
__attribute__((weak)) void launch_true_peak(const TruePeakLaunch& L, void*)
{
	std::vector<double> xs((size_t) kTpLdsDoubles);
	const long long tiles = (L.n + kTpTile - 1) / kTpTile;
	for (int row = 0; row < L.nch; row++)
		for (long long bx = 0; bx < tiles; bx++)
		{
			const long long t0 = bx * kTpTile;
			// (pad slots are never written and must never matter)
			std::fill(xs.begin(), xs.end(), std::numeric_limits<double>::quiet_NaN());
			tp_load(L, xs.data(), row, t0, 0, 1);
			if (bx + 1 == tiles) tp_history(L, xs.data(), row, t0, 0, 1);
			tp_compute(tp_tile(L, row, t0), xs.data(), 0, 1, [&L](int ch, unsigned long long pk)
			{
				if (pk > L.values[ch]) L.values[ch] = pk;
			});
		}
}

// The loudness launch as a loop on the host: r8b_loudness.h's ld_row for every row, tid = 0 and NTHR = 1, a barrier that
// does nothing.  WEAK, as launch_true_peak above: the device library links k_loudness's launcher over it.
__attribute__((weak)) void launch_loudness(const LoudnessLaunch& L, void*)
{
	std::vector<double> lds((size_t) kLdLdsDoubles);
	for (int row = 0; row < L.nch; row++) ld_row<1>(L, lds.data(), row, 0, [] {});
}

// The loudness meter's constants for the destination rate fs (include/r8bsrc.h "loudness"): the ten coefficients in
// plain fp64, the hand-off matrix by the recurrence itself, the sub-block's frames
void loudness_design(double fs, double* coef, double* phi, long long* hop)
{
	const double pi = 3.141592653589793;
	{
		const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
		const double K = tan(pi * f0 / fs), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416);
		const double a0 = 1.0 + K / Q + K * K;
		coef[0] = (Vh + Vb * K / Q + K * K) / a0;
		coef[1] = 2.0 * (K * K - Vh) / a0;
		coef[2] = (Vh - Vb * K / Q + K * K) / a0;
		coef[3] = 2.0 * (K * K - 1.0) / a0;
		coef[4] = (1.0 - K / Q + K * K) / a0;
	}
	{
		const double f0 = 38.13547087602444, Q = 0.5003270373238773;
		const double K = tan(pi * f0 / fs);
		const double a0 = 1.0 + K / Q + K * K;
		coef[5] = 1.0;
		coef[6] = -2.0;
		coef[7] = 1.0;
		coef[8] = 2.0 * (K * K - 1.0) / a0;
		coef[9] = (1.0 - K / Q + K * K) / a0;
	}
	for (int j = 0; j < 4; j++)
	{
		double s[4] = { 0.0, 0.0, 0.0, 0.0 };
		s[j] = 1.0;
		for (int f = 0; f < kLdSeg; f++) ld_frame(coef, 0.0, s);
		for (int i = 0; i < 4; i++) phi[4 * i + j] = s[i];
	}
	*hop = (long long) (fs / 10 + 0.5);
}

} // namespace r8bhip

namespace {

thread_local std::string g_err;

void set_err(const char* where, const std::exception& e)
{
	g_err = std::string(where) + ": " + e.what();
}

struct Batch
{
	std::unique_ptr<Engine> eng;
	// staging for the host-pointer entry points
	double* d_in = nullptr;
	double* d_out = nullptr;
	long long in_cap = 0, out_cap = 0; // per-channel capacities
	// PCM egress finish (r8b_batch_set_dither, r8b_batch_meter_*): settings of the handle, not of the engine -- they are
	// no engine option, enter no configuration hash and no checkpoint
	int dither_mode = 0, first_channel = 0;
	unsigned long long seed = 0;
	bool meters_on = false;
	unsigned long long* d_meters = nullptr; // peak | clipped | nonfinite, channels() entries each; allocated on first enable
	// true-peak meter (r8b_batch_true_peak_*; r8b_truepeak.h): a setting of the handle like the meters.  d_tp: channels()
	// values, then two history arrays of kTpHistStride doubles per channel, taken in turn -- tp_cur is the one the next
	// launch reads, tp_live whether it holds the stream's last frames (false: they read as zeros); the y of the next
	// tp_skip frames are not metered (the history refills after r8b_batch_state_load)
	bool tp_on = false, tp_live = false;
	double* d_tp = nullptr;
	int tp_cur = 0, tp_skip = 0;
	// loudness meter (r8b_batch_loudness_*; r8b_loudness.h), a setting of the handle too.  d_ld: kLdStateStride doubles of
	// state per row, then ld_cap sums per channel.  The host knows everything but the values: ld_m meter frames have run
	// (whole segments), ld_pending more wait in the state; slot 0 of the store is sub-block ld_store0; ld_count[c] slots
	// of channel c are filled (one number for all channels but after a clip call, ld_clip, whose store the next metered
	// call empties).  ld_fresh: the device state reads as zeros
	bool ld_on = false, ld_fresh = true, ld_clip = false;
	double* d_ld = nullptr;
	double dst_rate = 0.0; // (0: an object made of one stage has none)
	long long ld_cap = 0, ld_hop = 0, ld_m = 0, ld_store0 = 0;
	int ld_pending = 0;
	std::vector<long long> ld_count;
	double ld_coef[10], ld_phi[16];
	// output frames since creation / clear() of a pass-through object (no stage counts them): the dither's frame number
	long long pass_frames = 0;
	// r8b_batch_resample_clips: the device copies of a call's length arrays (input lengths, then output lengths,
	// channels() entries each).  A call's kernels read them long after the call has returned, so kClipSlots copies are
	// used in turn, each with the host block its upload reads and an event recorded behind the call's last launch; a
	// slot is taken again only once that event has passed (include/r8bsrc.h)
	struct ClipSlot
	{
		long long* d_len = nullptr;
		std::vector<long long> host;
		// r8b_batch_resample_clips_mix: the call's matrix beside its lengths -- a device block of mix_cap doubles
		// (allocated or enlarged when the slot is taken, i.e. behind its event) and the host block its upload reads
		double* d_mix = nullptr;
		size_t mix_cap = 0;
		std::vector<double> host_mix;
		// r8b_batch_resample_clips_packed: the call's bases (PcmLaunch::clip_base) lie behind the lengths in both blocks and
		// travel in the same upload -- the input side's and then the output side's, one per row of a planar side, one per
		// clip of an interleaved one, none for a strided one.  len_cap: entries of d_len (enlarged, like the matrix's block,
		// when the slot is taken, i.e. behind its event)
		size_t len_cap = 0;
		void* done = nullptr;
		bool used = false;
	};
	static const int kClipSlots = 4;
	ClipSlot clip_slot[kClipSlots];
	int clip_next = 0;
	~Batch()
	{
		dev_free(d_in);
		dev_free(d_out);
		dev_free(d_meters);
		dev_free(d_tp);
		dev_free(d_ld);
		for (ClipSlot& s : clip_slot)
		{
			dev_free(s.d_len);
			dev_free(s.d_mix);
			dev_event_destroy(s.done);
		}
	}
	size_t meter_bytes() const { return (size_t) 3 * eng->channels() * sizeof(unsigned long long); }
	size_t tp_bytes() const { return (size_t) (1 + 2 * kTpHistStride) * eng->channels() * sizeof(double); }
	// whether the stream has taken samples since creation / clear() (the clip entries' "fresh object" rule)
	bool streaming() const { return eng->plan().stages.empty() ? pass_frames != 0 : eng->plan().stages.front().m != 0; }
	// the history is gone (a checkpoint was loaded, the meter was off for a while): zeros, and the next 11 frames only refill it
	void tp_drop_history()
	{
		tp_live = false;
		tp_skip = kTpHist;
	}
	// the true-peak launch beside an egress launch over n frames of rows [0, nch) of the staging rows; T: the clip fields
	void true_peak(TruePeakLaunch T, int nch, long long n, void* stream)
	{
		double* const hist = d_tp + eng->channels();
		const size_t one = (size_t) kTpHistStride * eng->channels();
		T.rows = d_out;
		T.stride = out_cap;
		T.nch = nch;
		T.n = n;
		T.skip = tp_skip < n ? tp_skip : (int) n;
		T.hist_in = tp_live ? hist + one * tp_cur : nullptr;
		T.hist_out = hist + one * (tp_cur ^ 1);
		T.values = reinterpret_cast<unsigned long long*>(d_tp);
		launch_true_peak(T, stream);
		tp_cur ^= 1;
		tp_live = true;
		tp_skip -= T.skip;
	}
	// the loudness meter starts again at meter frame 0; what the store holds stays in front of what comes
	void ld_restart()
	{
		ld_fresh = true;
		ld_pending = 0;
		ld_m = 0;
		ld_store0 = ld_clip || ld_count.empty() ? 0 : -ld_count[0];
	}
	// the store is empty from here on: slot 0 is the next sub-block to complete
	void ld_empty()
	{
		std::fill(ld_count.begin(), ld_count.end(), 0);
		ld_clip = false;
		ld_store0 = ld_hop > 0 ? ld_m / ld_hop : 0;
	}
	// sub-blocks a streaming call of n output frames would leave in the store; throws if they do not fit
	long long ld_after(long long n) const
	{
		const long long m = (ld_m + ld_pending + n) / kLdSeg * kLdSeg;
		const long long count = m / ld_hop - (ld_clip ? ld_m / ld_hop : ld_store0);
		if (count > ld_cap)
			throw std::runtime_error("the loudness store holds " + std::to_string(ld_cap) + " sub-blocks per channel and this call "
				"would complete the " + std::to_string(count) + "th: read with drain first");
		return count;
	}
	// the loudness launch beside an egress launch over n frames of rows [0, nch) of the staging rows; T: the clip fields
	void loudness(LoudnessLaunch T, int nch, long long n, void* stream)
	{
		T.rows = d_out;
		T.stride = out_cap;
		T.nch = nch;
		T.n = n;
		T.pending = ld_pending;
		T.fresh = ld_fresh ? 1 : 0;
		T.m0 = ld_m;
		T.hop = ld_hop;
		T.store0 = ld_store0;
		T.capacity = ld_cap;
		T.state = d_ld;
		T.sums = d_ld + (size_t) kLdStateStride * eng->channels();
		memcpy(T.coef, ld_coef, sizeof(ld_coef));
		memcpy(T.phi, ld_phi, sizeof(ld_phi));
		launch_loudness(T, stream);
		const long long total = ld_pending + n;
		ld_m += total / kLdSeg * kLdSeg;
		ld_pending = (int) (total % kLdSeg);
		ld_fresh = false;
	}
	void count_pass(int n)
	{
		if (n > 0 && eng->plan().stages.empty()) pass_frames += n;
	}
	void clear()
	{
		eng->clear();
		pass_frames = 0;
		if (d_meters)
		{
			DevGuard guard(eng->device());
			dev_zero(d_meters, meter_bytes(), nullptr);
		}
		if (d_tp)
		{
			DevGuard guard(eng->device());
			dev_zero(d_tp, tp_bytes(), nullptr);
		}
		tp_live = false;
		tp_skip = 0;
		ld_clip = false;
		ld_restart();
		ld_empty();
	}
	void need_staging()
	{
		if (d_in) return;
		in_cap = eng->plan().max_in;
		out_cap = eng->plan().max_out_len > 0 ? eng->plan().max_out_len : 1;
		d_in = (double*) dev_alloc((size_t) in_cap * eng->channels() * sizeof(double));
		d_out = (double*) dev_alloc((size_t) out_cap * eng->channels() * sizeof(double));
	}
};

// the reference-shaped single-stream object (r8b_create ... r8b_process)
struct Single
{
	Batch b;
	std::vector<double> out;
};

double res_atten(int res)
{
	// reference DLL/r8bsrc.cpp:67-85 -> CDSPResampler16 / 16IR / 24 (CDSPResampler.h:746,777,807)
	switch (res)
	{
	case r8brr16: return 136.45;
	case r8brr16IR: return 109.56;
	default: return 180.15;
	}
}

int copy_text(const std::string& s, char* buf, int cap)
{
	if (buf != nullptr && cap > 0)
	{
		const int n = (int) s.size() < cap - 1 ? (int) s.size() : cap - 1;
		memcpy(buf, s.data(), (size_t) n);
		buf[n] = 0;
	}
	return (int) s.size();
}

int batch_process_host(Batch* h, const double* in, long long in_stride, int l, double* out,
	long long out_stride)
{
	h->need_staging();
	Engine& e = *h->eng;
	const int nch = e.channels();
	if (l > h->in_cap) throw std::runtime_error("input length exceeds MaxInLen");
	std::vector<double> tmp;
	if (l > 0)
	{
		if (in_stride == l && h->in_cap == l)
			dev_upload(h->d_in, in, (size_t) l * nch * sizeof(double));
		else
			for (int c = 0; c < nch; c++)
				dev_upload(h->d_in + (long long) c * h->in_cap, in + (long long) c * in_stride,
					(size_t) l * sizeof(double));
	}
	const int n = e.process(h->d_in, h->in_cap, l, h->d_out, h->out_cap, nullptr);
	h->count_pass(n);
	dev_sync(nullptr);
	dev_check_last("r8b process");
	for (int c = 0; c < nch && n > 0; c++)
		dev_download(out + (long long) c * out_stride, h->d_out + (long long) c * h->out_cap,
			(size_t) n * sizeof(double), nullptr);
	return n;
}

// A launch of the PCM boundary.  With option "timing" = 1 the engine keeps the symbol of what the launcher started
// (side 0 the ingest, 1 the egress: r8b_batch_stage_symbol's pseudo-stages); boundary_begin() at a call's start, so
// that a side the call launches nothing for reads ""
void boundary_begin(Engine& e)
{
	if (!e.timing()) return;
	e.pcm_symbol_note(0, nullptr);
	e.pcm_symbol_note(1, nullptr);
}

void boundary_launch(Engine& e, int side, const PcmLaunch& L, void* stream)
{
	const bool timing = e.timing();
	if (timing) launch_symbol_note(nullptr);
	if (side == 0) launch_pcm_in(L, stream);
	else launch_pcm_out(L, stream);
	if (timing) e.pcm_symbol_note(side, launch_symbol_last());
}

// PCM boundary.  Planar buffers are decoded by the first stage's loads and encoded by the last
// stage's stores (Engine::process_planar); an interleaved side goes through a transposing kernel
// and the staging rows.  Everything is enqueued on `stream`, nothing synchronises.
int batch_process_pcm(Batch* h, const void* d_in, int in_fmt, int in_interleaved,
	long long in_stride, int l, void* d_out, int out_fmt, int out_interleaved, long long out_stride,
	void* stream)
{
	Engine& e = *h->eng;
	auto valid = [](int f) { return pcm_io_bytes(f) != 0; };
	if (!valid(in_fmt) || !valid(out_fmt)) throw std::runtime_error("unknown PCM sample format");
	if (l < 0 || l > e.plan().max_in) throw std::runtime_error("input length exceeds MaxInLen");
	boundary_begin(e);
	if (l == 0) return 0;
	// Src == Dst has no stage to fuse into: both sides staged
	const bool pass = e.plan().stages.empty();
	// the loudness store must take what this call completes: refused here, before anything is enqueued
	long long ld_count = 0;
	if (h->ld_on)
	{
		ChainPlan probe = e.plan();
		long long nout = l;
		for (StagePlan& sp : probe.stages)
		{
			long long a, b;
			sp.step((int) nout, &a, &b, nullptr);
			nout = b - a;
		}
		ld_count = h->ld_after(nout);
	}
	// ... and so has a planar PCM side whose first / last stage is a compile-time-sized convolver (fp64 views only)
	// ... and so has every output side while dither (integer formats; the float ones ignore it) or meters are on: the
	// finishing egress kernels do both (r8b_pcm.h)
	const bool dither = h->dither_mode != 0 && pcm_io_dithers(out_fmt);
	const bool finish = dither || h->meters_on;
	// ... and so has every side in a one-byte format: the stage kernels' codec does not know them (r8b_pcm_codec.h)
	const bool stage_in = in_interleaved || pass || (in_fmt != kPcmF64 && !e.pcm_fused_in()) || pcm_io_bytes(in_fmt) == 1;
	// ... and so has every output side while the true-peak meter is on: it reads the staging rows (which egress kernel
	// runs stays `finish`'s matter)
	const bool stage_out = out_interleaved || pass || finish || h->tp_on || h->ld_on || (out_fmt != kPcmF64 && !e.pcm_fused_out()) ||
		pcm_io_bytes(out_fmt) == 1;
	// absolute output frame of this call's first one: what the last stage has emitted so far (StagePlan::done, in the
	// checkpoint blob); a pass-through object has no stage and counts in the handle
	const long long frame0 = pass ? h->pass_frames : e.plan().stages.back().done;
	if (stage_in || stage_out) h->need_staging();
	if (stage_in && !in_interleaved && !pass) e.bump(kPcmStagedSides);
	if (stage_out && !out_interleaved && !pass) e.bump(kPcmStagedSides);
	PcmLaunch P;
	P.nch = e.channels();
	if (stage_in)
	{
		P.pcm = const_cast<void*>(d_in);
		P.fmt = in_fmt;
		P.interleaved = in_interleaved ? 1 : 0;
		P.pcm_stride = in_stride;
		P.planar = h->d_in;
		P.planar_stride = h->in_cap;
		P.n = l;
		boundary_launch(e, 0, P, stream);
		d_in = h->d_in;
		in_fmt = kPcmF64;
		in_stride = h->in_cap;
	}
	void* const out = stage_out ? h->d_out : d_out;
	const int n = pass ? e.process(static_cast<const double*>(d_in), in_stride, l, h->d_out,
		h->out_cap, stream) : e.process_planar(d_in, in_fmt, in_stride, l, out,
		stage_out ? (int) kPcmF64 : out_fmt, stage_out ? (long long) h->out_cap : out_stride, stream);
	h->count_pass(n);
	if (stage_out && n > 0)
	{
		P.pcm = d_out;
		P.fmt = out_fmt;
		P.interleaved = out_interleaved ? 1 : 0;
		P.pcm_stride = out_stride;
		P.planar = h->d_out;
		P.planar_stride = h->out_cap;
		P.n = n;
		if (dither)
		{
			P.dither = h->dither_mode;
			P.seed = h->seed;
			P.first_channel = h->first_channel;
			P.frame0 = frame0;
		}
		if (h->meters_on)
		{
			P.m_peak = h->d_meters;
			P.m_clipped = P.m_peak + P.nch;
			P.m_nonfinite = P.m_clipped + P.nch;
		}
		boundary_launch(e, 1, P, stream);
		if (h->tp_on) h->true_peak(TruePeakLaunch(), P.nch, n, stream);
		if (h->ld_on)
		{
			if (h->ld_clip) h->ld_empty();
			h->loudness(LoudnessLaunch(), P.nch, n, stream);
			std::fill(h->ld_count.begin(), h->ld_count.end(), ld_count);
		}
	}
	return n;
}

// The order of r8b_batch_resample_clips_sched / r8b_clip_schedule: order[g] is the clip that rides in slot g -- the
// identity, or, longest_first, the clips by output length descending, equal lengths by ascending index
void clip_order(int nclips, const long long* out_len, bool longest_first, int* order)
{
	for (int i = 0; i < nclips; i++) order[i] = i;
	if (longest_first)
		std::stable_sort(order, order + nclips, [out_len](int a, int b) { return out_len[a] > out_len[b]; });
}

// The channels a dropping step runs when `done` outputs exist: slot g is live while its clip still owes outputs; the
// slots up to the last live one, as whole clips -- and whole channel pairs (the pair kernels take channels two by two):
// an odd count takes the next clip along, unless it is the whole object already.  Never grows with `done`
int clip_active(int nclips, int K, const long long* out_len, const int* order, long long done)
{
	int hi = 0;
	for (int g = 0; g < nclips; g++)
		if (out_len[order[g]] > done) hi = g + 1;
	int A = hi * K;
	if ((A & 1) != 0 && hi < nclips) A += K;
	return A;
}

// A batch of clips of unequal length in one call (include/r8bsrc.h r8b_batch_resample_clips): the loop a host would
// write around r8b_batch_process_pcm -- MaxInLen frames per step, zeros once the clips have ended, until the last
// output has come out (reference CDSPResampler.h:592-651, bench/r8bfreesrc.cpp:92-136) -- with both sides going through
// the staging rows and the masked row kernels of r8b_clip.h, which know every clip's length.
// clip_channels = K: clip i is channels i K .. i K + K - 1 and has one entry in each length array; a side is planar (row
// c at c * stride) or, with K > 1, may hold the clips frame-major (clip i at i * stride: r8b_clip_frames.h).
// Kin != 0 (r8b_batch_resample_clips_mix): the input side holds Kin channels per clip in either layout and the
// ingest mixes them down (or up) to the K object channels by the K x Kin HOST matrix `mix` (r8b_clip_mix.h); the
// matrix travels as the lengths do, through a host and a device block of the call's slot.  Kin = 0: no mix (the entry
// has checked Kin's range and the pointer).
// in_off / out_off != nullptr (r8b_batch_resample_clips_packed): that side is packed -- clip i's region starts at element
// in_off[i] / out_off[i] of its buffer and holds the clip's channels at the clip's own length (r8b_clip_packed.h); the
// stride is ignored.  The kernels get one base per row of a planar side and one per clip of an interleaved one, worked
// out here and sent through the slot behind the lengths.  nullptr: strided.
// flags (r8b_batch_resample_clips_sched; 0: none of this, the calls above as they always ran):
//   R8B_CLIPS_LONGEST_FIRST  clip order[g] rides in slot g = staging rows and object channels g K .. g K + K - 1
//     (clip_order: by output length, longest first).  Everything the kernels read per row or per clip -- lengths, bases --
//     is filled here in slot order, a strided side gets bases too (row or clip times the stride), and the egress learns
//     each row's channel in the caller's numbering (PcmLaunch::clip_chan: dither key, meters) and whether to store the
//     padding behind a base (PcmLaunch::clip_pad: a strided output); r8b_clip_sched.h.
//   R8B_CLIPS_DROP_FINISHED  a step's ingest and stages run channels [0, A) only (clip_active: the slots that still owe
//     outputs, as whole clips and whole channel pairs); a packed egress covers the same rows, a strided one every row --
//     a finished row's frames all lie at or past its length there, so it stores padding and loads nothing.
long long batch_resample_clips(Batch* h, int K, int Kin, const double* mix, const void* d_in, int in_fmt,
	int in_interleaved, long long in_stride, const long long* in_off, const long long* in_len, void* d_out, int out_fmt,
	int out_interleaved, long long out_stride, const long long* out_off, const long long* out_len, void* stream,
	int flags = 0)
{
	Engine& e = *h->eng;
	auto valid = [](int f) { return pcm_io_bytes(f) != 0; };
	const bool mixing = Kin != 0;
	if ((flags & ~(R8B_CLIPS_DROP_FINISHED | R8B_CLIPS_LONGEST_FIRST)) != 0) throw std::runtime_error("flags holds an unknown bit");
	const bool drop = (flags & R8B_CLIPS_DROP_FINISHED) != 0, ordered = (flags & R8B_CLIPS_LONGEST_FIRST) != 0;
	if (!valid(in_fmt) || !valid(out_fmt)) throw std::runtime_error("unknown PCM sample format");
	if (in_len == nullptr || out_len == nullptr) throw std::runtime_error("null length array");
	const int nch = e.channels();
	if (K < 1 || K > kClipChannelsMax) throw std::runtime_error("clip_channels must be 1 .. 64");
	if (nch % K != 0) throw std::runtime_error("clip_channels does not divide the object's channel count");
	const int nclips = nch / K;
	if (mixing)
		for (int j = 0; j < K * Kin; j++)
			if (!(mix[j] - mix[j] == 0.0)) throw std::runtime_error("mix holds a coefficient that is not finite");
	long long max_in = 0, P = 0;
	for (int c = 0; c < nclips; c++)
	{
		if (in_len[c] < 0 || out_len[c] < 0) throw std::runtime_error("negative clip length");
		if (in_len[c] > max_in) max_in = in_len[c];
		if (out_len[c] > P) P = out_len[c];
	}
	const bool pass = e.plan().stages.empty();
	if (pass ? h->pass_frames != 0 : e.plan().stages.front().m != 0)
		throw std::runtime_error("the object has processed samples since creation / r8b_batch_clear()");
	// (one channel per clip: a frame-major clip IS a row)
	const bool in_frames = in_interleaved && (mixing ? Kin : K) > 1, out_frames = out_interleaved && K > 1;
	const int Kc = mixing ? Kin : K; // channels of a clip in the input buffer
	if (in_off == nullptr && in_stride < max_in * (in_frames ? Kc : 1))
		throw std::runtime_error("in_stride is smaller than the longest clip");
	if (out_off == nullptr && out_stride < P * (out_frames ? K : 1))
		throw std::runtime_error("out_stride is smaller than the longest output");
	for (int c = 0; c < nclips; c++)
	{
		if (in_off != nullptr && in_off[c] < 0) throw std::runtime_error("in_offset holds a negative offset");
		if (out_off != nullptr && out_off[c] < 0) throw std::runtime_error("out_offset holds a negative offset");
	}
	if (out_off != nullptr)
	{
		// two clips must not be written to the same elements (inputs may share theirs): the non-empty regions in order
		std::vector<std::pair<long long, long long>> reg;
		for (int c = 0; c < nclips; c++)
			if (out_len[c] > 0) reg.emplace_back(out_off[c], out_off[c] + out_len[c] * K);
		std::sort(reg.begin(), reg.end());
		for (size_t j = 1; j < reg.size(); j++)
			if (reg[j].first < reg[j - 1].second) throw std::runtime_error("out_offset: the regions of two clips overlap");
	}
	// the loudness store must take the longest clip's sub-blocks: refused here, before anything is enqueued
	if (h->ld_on && P / h->ld_hop > h->ld_cap)
		throw std::runtime_error("the loudness store holds " + std::to_string(h->ld_cap) + " sub-blocks per channel and the longest "
			"clip has " + std::to_string(P / h->ld_hop));
	boundary_begin(e);
	if (h->ld_on)
	{
		// state and store start empty at the call; what a clip will have stored is known now
		h->ld_clip = false;
		h->ld_restart();
		h->ld_empty();
		h->ld_clip = true;
		for (int c = 0; c < nch; c++) h->ld_count[c] = out_len[c / K] / h->ld_hop;
	}
	if (P == 0) return 0;
	if (d_out == nullptr || (d_in == nullptr && max_in > 0)) throw std::runtime_error("null device pointer");
	if ((in_fmt == kPcmF64 && ((size_t) d_in & 7) != 0) || (out_fmt == kPcmF64 && ((size_t) d_out & 7) != 0))
		throw std::runtime_error("fp64 buffers must be 8-byte aligned");
	DevGuard guard(e.device());
	h->need_staging();
	// the lengths: into the next slot, uploaded on `stream` in front of this call's kernels
	Batch::ClipSlot& slot = h->clip_slot[h->clip_next];
	h->clip_next = (h->clip_next + 1) % Batch::kClipSlots;
	if (slot.done == nullptr) slot.done = dev_event_create();
	// (the call made kClipSlots calls ago: waits only while all the slots are in flight)
	if (slot.used) dev_event_elapsed_ms(slot.done, slot.done);
	// the bases of the packed sides behind the lengths: a planar side's row k of clip i starts k clip lengths behind the
	// clip's offset
	// (an ordered call: both sides have bases, and the rows' object channels lie behind them)
	const size_t in_bases = in_off == nullptr && !ordered ? 0 : (size_t) nclips * (in_frames ? 1 : Kc);
	const size_t out_bases = out_off == nullptr && !ordered ? 0 : (size_t) nclips * (out_frames ? 1 : K);
	const size_t entries = (size_t) 2 * nch + in_bases + out_bases + (ordered ? nch : 0);
	// order[g]: the clip in slot g
	std::vector<int> order((size_t) nclips);
	clip_order(nclips, out_len, ordered, order.data());
	if (slot.len_cap < entries)
	{
		// (the slot's event has passed: no kernel reads the block that is replaced)
		dev_free(slot.d_len);
		slot.d_len = nullptr;
		slot.len_cap = 0;
		slot.d_len = (long long*) dev_alloc(entries * sizeof(long long));
		dev_sync(nullptr); // (dev_alloc zeroes on the null stream, which a non-blocking `stream` does not follow)
		slot.len_cap = entries;
	}
	// (one length per channel, the clip's: the masked row kernels read their row's, the tile kernels the clip's first)
	slot.host.resize((size_t) 2 * nch);
	for (int c = 0; c < nch; c++)
	{
		slot.host[c] = in_len[order[c / K]];
		slot.host[nch + c] = out_len[order[c / K]];
	}
	// (a strided side of an ordered call: clip c's rows or region where the stride puts them)
	for (int g = 0; in_bases != 0 && g < nclips; g++)
		for (int k = 0, c = order[g]; k < (in_frames ? 1 : Kc); k++)
			slot.host.push_back(in_off != nullptr ? in_off[c] + k * in_len[c] : ((long long) c * (in_frames ? 1 : Kc) + k) * in_stride);
	for (int g = 0; out_bases != 0 && g < nclips; g++)
		for (int k = 0, c = order[g]; k < (out_frames ? 1 : K); k++)
			slot.host.push_back(out_off != nullptr ? out_off[c] + k * out_len[c] : ((long long) c * (out_frames ? 1 : K) + k) * out_stride);
	for (int r = 0; ordered && r < nch; r++) slot.host.push_back((long long) order[r / K] * K + r % K);
	dev_upload_async(slot.d_len, slot.host.data(), slot.host.size() * sizeof(long long), stream);
	slot.used = true;
	if (mixing)
	{
		// (the slot's event has passed: no kernel reads the block that is replaced)
		const size_t count = (size_t) K * Kin;
		if (slot.mix_cap < count)
		{
			dev_free(slot.d_mix);
			slot.d_mix = nullptr;
			slot.mix_cap = 0;
			slot.d_mix = (double*) dev_alloc(count * sizeof(double));
			dev_sync(nullptr); // (as above)
			slot.mix_cap = count;
		}
		slot.host_mix.assign(mix, mix + count);
		dev_upload_async(slot.d_mix, slot.host_mix.data(), count * sizeof(double), stream);
	}
	// whatever happens below, the object is left as after r8b_batch_clear() (but for the meters: the kernels may still
	// be in flight, and the caller reads them afterwards), and the slot knows when this call's last launch is through
	struct Finish
	{
		Batch* h;
		Batch::ClipSlot& slot;
		void* stream;
		~Finish()
		{
			h->eng->clear();
			h->pass_frames = 0;
			h->tp_live = false;
			h->ld_restart();
			try { dev_event_record(slot.done, stream); } catch (const std::exception&) {}
		}
	} finish{h, slot, stream};
	const bool dither = h->dither_mode != 0 && pcm_io_dithers(out_fmt);
	const int l = (int) h->in_cap;
	PcmLaunch I;
	I.nch = nch;
	I.interleaved = in_frames ? 1 : 0;
	I.clip_channels = K;
	I.pcm = const_cast<void*>(d_in);
	I.fmt = in_fmt;
	I.pcm_stride = in_stride;
	I.planar = h->d_in;
	I.planar_stride = h->in_cap;
	I.n = l;
	I.clip_len = slot.d_len;
	if (mixing)
	{
		I.mix_channels = Kin;
		I.mix = slot.d_mix;
	}
	if (in_bases != 0) I.clip_base = slot.d_len + 2 * nch;
	PcmLaunch O;
	O.nch = nch;
	O.interleaved = out_frames ? 1 : 0;
	O.clip_channels = K;
	O.pcm = d_out;
	O.fmt = out_fmt;
	O.pcm_stride = out_stride;
	O.planar = h->d_out;
	O.planar_stride = h->out_cap;
	O.clip_len = slot.d_len + nch;
	if (out_bases != 0) O.clip_base = slot.d_len + 2 * nch + in_bases;
	if (ordered)
	{
		O.clip_chan = slot.d_len + 2 * nch + in_bases + out_bases;
		O.clip_pad = out_off == nullptr ? 1 : 0;
	}
	if (dither)
	{
		O.dither = h->dither_mode;
		O.seed = h->seed;
		O.first_channel = h->first_channel;
	}
	if (h->meters_on)
	{
		O.m_peak = h->d_meters;
		O.m_clipped = O.m_peak + nch;
		O.m_nonfinite = O.m_clipped + nch;
	}
	// the true-peak meter: zero history at the start of the call (the object is fresh), carried from step to step
	h->tp_live = false;
	h->tp_skip = 0;
	TruePeakLaunch TP;
	TP.clip_len = O.clip_len;
	TP.clip_chan = O.clip_chan;
	LoudnessLaunch LD;
	LD.clip_len = O.clip_len;
	LD.clip_chan = O.clip_chan;
	bool zeroed = false;
	// (outputs past P are never asked for: the loop ends with the last one, as the reference's oneshot() does)
	for (long long pos = 0, done = 0; done < P; pos += l)
	{
		// the channels this step runs: all of them, or those of the slots that still owe outputs
		const int A = drop ? clip_active(nclips, K, out_len, order.data(), done) : nch;
		if (pos < max_in)
		{
			I.in_frame0 = pos;
			I.nch = A;
			boundary_launch(e, 0, I, stream);
		}
		else if (!zeroed)
		{
			// every clip has ended: the staging rows are zeros from here on (A only shrinks)
			dev_zero(h->d_in, (size_t) h->in_cap * A * sizeof(double), stream);
			zeroed = true;
		}
		const int n = e.process(h->d_in, h->in_cap, l, h->d_out, h->out_cap, stream, A);
		e.bump(kClipSteps);
		e.bump(kClipChannelSteps, A);
		if (n > 0)
		{
			O.frame0 = done;
			O.n = n < P - done ? n : P - done;
			// (a side that stores padding covers every row: a finished row gets its zeros up to P)
			O.nch = out_off != nullptr ? A : nch;
			boundary_launch(e, 1, O, stream);
			if (h->tp_on)
			{
				// (rows [0, A): a dropped row's clip has ended, and its tail was metered by the step that held its last frame)
				TP.frame0 = done;
				h->true_peak(TP, A, O.n, stream);
			}
			if (h->ld_on)
			{
				LD.frame0 = done;
				h->loudness(LD, A, O.n, stream);
			}
		}
		done += n;
	}
	return P;
}

} // namespace

extern "C" {

R8BSRC_DECL const char* r8b_last_error(void) { return g_err.c_str(); }
R8BSRC_DECL const char* r8b_version(void) { return "r8bsrc-hip 0.1 (gfx950; tracks r8brain-free-src 7.1 semantics)"; }

// ---------------------------------------------------------------- batch object

R8BSRC_DECL CR8BBatch r8b_batch_create(double SrcSampleRate, double DstSampleRate, int MaxInLen,
	double ReqTransBand, double ReqAtten, int nch, int device)
{
	try
	{
		std::unique_ptr<Batch> b(new Batch());
		b->eng.reset(new Engine(build_topology(SrcSampleRate, DstSampleRate, ReqTransBand,
			ReqAtten), MaxInLen, nch, device));
		b->dst_rate = DstSampleRate;
		g_err.clear();
		return b.release();
	}
	catch (const std::exception& e)
	{
		set_err("r8b_batch_create", e);
		return nullptr;
	}
}

R8BSRC_DECL CR8BBatch r8b_batch_create_ex(double SrcSampleRate, double DstSampleRate, int MaxInLen,
	double ReqTransBand, double ReqAtten, int ReqPhase, int nch, int device)
{
	try
	{
		if (ReqPhase != kLinearPhase && ReqPhase != kMinPhase)
			throw std::runtime_error("ReqPhase must be 0 (linear phase) or 1 (minimum phase)");
		std::unique_ptr<Batch> b(new Batch());
		b->eng.reset(new Engine(build_topology(SrcSampleRate, DstSampleRate, ReqTransBand,
			ReqAtten, ReqPhase), MaxInLen, nch, device));
		b->dst_rate = DstSampleRate;
		g_err.clear();
		return b.release();
	}
	catch (const std::exception& e)
	{
		set_err("r8b_batch_create_ex", e);
		return nullptr;
	}
}

R8BSRC_DECL CR8BBatch r8b_batch_create_stage(int kind, double a, double b, double c, double d,
	int i0, int i1, int MaxInLen, int nch, int device)
{
	try
	{
		if (kind < 0 || kind > 3) throw std::runtime_error("stage kind must be 0 (convolver), 1 "
			"(interpolator), 2 (half-band up) or 3 (half-band down)");
		StageDesc sd;
		sd.kind = (StageKind) kind;
		sd.a = a; sd.b = b; sd.c = c; sd.d = d; sd.i0 = i0; sd.i1 = i1;
		std::unique_ptr<Batch> bo(new Batch());
		bo->eng.reset(new Engine(std::vector<StageDesc>(1, sd), MaxInLen, nch, device));
		g_err.clear();
		return bo.release();
	}
	catch (const std::exception& e)
	{
		set_err("r8b_batch_create_stage", e);
		return nullptr;
	}
}

// (the entries that can report an error refuse a NULL handle; the plain getters, like the reference's, do not test it)
static Batch* need(CR8BBatch b)
{
	if (b == nullptr) throw std::runtime_error("null handle");
	return (Batch*) b;
}

R8BSRC_DECL void r8b_batch_delete(CR8BBatch b) { delete (Batch*) b; }

R8BSRC_DECL void r8b_batch_clear(CR8BBatch b)
{
	if (b) ((Batch*) b)->clear();
}

R8BSRC_DECL int r8b_batch_channels(CR8BBatch b) { return ((Batch*) b)->eng->channels(); }

R8BSRC_DECL int r8b_batch_device(CR8BBatch b) { return ((Batch*) b)->eng->device(); }

R8BSRC_DECL int r8b_batch_max_out_len(CR8BBatch b) { return ((Batch*) b)->eng->plan().max_out_len; }

R8BSRC_DECL int r8b_batch_inlen(CR8BBatch b, int ReqOutSamples)
{
	return ((Batch*) b)->eng->plan().input_required(ReqOutSamples);
}

R8BSRC_DECL int r8b_batch_inlen_before_outpos(CR8BBatch b, int OutPos)
{
	return ((Batch*) b)->eng->plan().in_len_before_out_pos(OutPos);
}

R8BSRC_DECL int r8b_batch_process(CR8BBatch b, const double* d_in, long long in_stride, int l,
	double* d_out, long long out_stride, void* stream)
{
	try
	{
		Batch* const h = need(b);
		const int n = h->eng->process(d_in, in_stride, l, d_out, out_stride, stream);
		h->count_pass(n);
		return n;
	}
	catch (const std::exception& e)
	{
		set_err("r8b_batch_process", e);
		return -1;
	}
}

R8BSRC_DECL int r8b_batch_process_host(CR8BBatch b, const double* in, long long in_stride, int l,
	double* out, long long out_stride)
{
	try
	{
		return batch_process_host(need(b), in, in_stride, l, out, out_stride);
	}
	catch (const std::exception& e)
	{
		set_err("r8b_batch_process_host", e);
		return -1;
	}
}

R8BSRC_DECL int r8b_batch_process_pcm(CR8BBatch b, const void* d_in, int in_format,
	int in_interleaved, long long in_stride, int l, void* d_out, int out_format,
	int out_interleaved, long long out_stride, void* stream)
{
	try
	{
		return batch_process_pcm(need(b), d_in, in_format, in_interleaved, in_stride, l, d_out,
			out_format, out_interleaved, out_stride, stream);
	}
	catch (const std::exception& e)
	{
		set_err("r8b_batch_process_pcm", e);
		return -1;
	}
}

R8BSRC_DECL long long r8b_clip_out_len(double SrcSampleRate, double DstSampleRate, long long in_len)
{
	// reference bench/r8bfreesrc.cpp:92
	return (long long) ((double) in_len * DstSampleRate / SrcSampleRate);
}

R8BSRC_DECL long long r8b_batch_resample_clips(CR8BBatch b, const void* d_in, int in_format, long long in_stride,
	const long long* in_len, void* d_out, int out_format, long long out_stride, const long long* out_len, void* stream)
{
	try
	{
		return batch_resample_clips(need(b), 1, 0, nullptr, d_in, in_format, 0, in_stride, nullptr, in_len, d_out, out_format,
			0, out_stride, nullptr, out_len, stream);
	}
	catch (const std::exception& e)
	{
		set_err("r8b_batch_resample_clips", e);
		return -1;
	}
}

R8BSRC_DECL long long r8b_batch_resample_clips_ex(CR8BBatch b, int clip_channels, const void* d_in, int in_format,
	int in_interleaved, long long in_stride, const long long* in_len, void* d_out, int out_format, int out_interleaved,
	long long out_stride, const long long* out_len, void* stream)
{
	try
	{
		return batch_resample_clips(need(b), clip_channels, 0, nullptr, d_in, in_format, in_interleaved, in_stride, nullptr,
			in_len, d_out, out_format, out_interleaved, out_stride, nullptr, out_len, stream);
	}
	catch (const std::exception& e)
	{
		set_err("r8b_batch_resample_clips_ex", e);
		return -1;
	}
}

R8BSRC_DECL long long r8b_batch_resample_clips_mix(CR8BBatch b, int in_channels, int clip_channels, const double* mix,
	const void* d_in, int in_format, int in_interleaved, long long in_stride, const long long* in_len, void* d_out,
	int out_format, int out_interleaved, long long out_stride, const long long* out_len, void* stream)
{
	try
	{
		if (in_channels < 1 || in_channels > kClipChannelsMax) throw std::runtime_error("in_channels must be 1 .. 64");
		if (mix == nullptr) throw std::runtime_error("mix is NULL");
		return batch_resample_clips(need(b), clip_channels, in_channels, mix, d_in, in_format, in_interleaved, in_stride,
			nullptr, in_len, d_out, out_format, out_interleaved, out_stride, nullptr, out_len, stream);
	}
	catch (const std::exception& e)
	{
		set_err("r8b_batch_resample_clips_mix", e);
		return -1;
	}
}

R8BSRC_DECL long long r8b_batch_resample_clips_packed(CR8BBatch b, int in_channels, int clip_channels, const double* mix,
	const void* d_in, int in_format, int in_interleaved, long long in_stride, const long long* in_offset,
	const long long* in_len, void* d_out, int out_format, int out_interleaved, long long out_stride,
	const long long* out_offset, const long long* out_len, void* stream)
{
	try
	{
		if (mix == nullptr)
		{
			if (in_channels != 0 && in_channels != clip_channels)
				throw std::runtime_error("in_channels must be 0 or clip_channels when mix is NULL");
			in_channels = 0;
		}
		else if (in_channels < 1 || in_channels > kClipChannelsMax) throw std::runtime_error("in_channels must be 1 .. 64");
		return batch_resample_clips(need(b), clip_channels, in_channels, mix, d_in, in_format, in_interleaved, in_stride,
			in_offset, in_len, d_out, out_format, out_interleaved, out_stride, out_offset, out_len, stream);
	}
	catch (const std::exception& e)
	{
		set_err("r8b_batch_resample_clips_packed", e);
		return -1;
	}
}

R8BSRC_DECL long long r8b_batch_resample_clips_sched(CR8BBatch b, int in_channels, int clip_channels, const double* mix,
	const void* d_in, int in_format, int in_interleaved, long long in_stride, const long long* in_offset,
	const long long* in_len, void* d_out, int out_format, int out_interleaved, long long out_stride,
	const long long* out_offset, const long long* out_len, int flags, void* stream)
{
	// (flags == 0: the packed entry itself)
	if (flags == 0)
		return r8b_batch_resample_clips_packed(b, in_channels, clip_channels, mix, d_in, in_format, in_interleaved, in_stride,
			in_offset, in_len, d_out, out_format, out_interleaved, out_stride, out_offset, out_len, stream);
	try
	{
		if (mix == nullptr)
		{
			if (in_channels != 0 && in_channels != clip_channels)
				throw std::runtime_error("in_channels must be 0 or clip_channels when mix is NULL");
			in_channels = 0;
		}
		else if (in_channels < 1 || in_channels > kClipChannelsMax) throw std::runtime_error("in_channels must be 1 .. 64");
		return batch_resample_clips(need(b), clip_channels, in_channels, mix, d_in, in_format, in_interleaved, in_stride,
			in_offset, in_len, d_out, out_format, out_interleaved, out_stride, out_offset, out_len, stream, flags);
	}
	catch (const std::exception& e)
	{
		set_err("r8b_batch_resample_clips_sched", e);
		return -1;
	}
}

R8BSRC_DECL int r8b_clip_schedule(int nclips, const long long* out_len, int flags, int* order)
{
	if (nclips < 0 || (flags & ~(R8B_CLIPS_DROP_FINISHED | R8B_CLIPS_LONGEST_FIRST)) != 0) return -1;
	if (nclips > 0 && (out_len == nullptr || order == nullptr)) return -1;
	for (int i = 0; i < nclips; i++)
		if (out_len[i] < 0) return -1;
	clip_order(nclips, out_len, (flags & R8B_CLIPS_LONGEST_FIRST) != 0, order);
	return 0;
}

R8BSRC_DECL long long r8b_clip_pack_offsets(int nclips, const long long* len, int channels, int align, long long* offset)
{
	if (nclips < 0 || channels < 1 || align < 1) return -1;
	for (int i = 0; i < nclips; i++)
		if (len[i] < 0) return -1;
	long long end = 0;
	for (int i = 0; i < nclips; i++)
	{
		const long long base = (end + align - 1) / align * align;
		offset[i] = base;
		end = base + len[i] * channels;
	}
	return end;
}

R8BSRC_DECL int r8b_batch_set_dither(CR8BBatch b, int mode, unsigned long long seed, int first_channel)
{
	try
	{
		Batch* const h = need(b);
		if (mode != R8B_DITHER_NONE && mode != R8B_DITHER_TPDF)
			throw std::runtime_error("dither mode must be 0 (none) or 1 (TPDF)");
		if (first_channel < 0) throw std::runtime_error("first_channel must not be negative");
		h->dither_mode = mode;
		h->seed = seed;
		h->first_channel = first_channel;
		return 0;
	}
	catch (const std::exception& e)
	{
		set_err("r8b_batch_set_dither", e);
		return -1;
	}
}

R8BSRC_DECL int r8b_batch_meter_enable(CR8BBatch b, int on)
{
	try
	{
		Batch* const h = need(b);
		if (on && h->d_meters == nullptr)
		{
			DevGuard guard(h->eng->device());
			h->d_meters = (unsigned long long*) dev_alloc(h->meter_bytes()); // (zeroed)
		}
		h->meters_on = on != 0;
		return 0;
	}
	catch (const std::exception& e)
	{
		set_err("r8b_batch_meter_enable", e);
		return -1;
	}
}

R8BSRC_DECL int r8b_batch_meter_read(CR8BBatch b, double* peak, long long* clipped, long long* nonfinite, int reset,
	void* stream)
{
	try
	{
		Batch* const h = need(b);
		if (h->d_meters == nullptr) throw std::runtime_error("the object's meters were never enabled");
		DevGuard guard(h->eng->device());
		const size_t nch = (size_t) h->eng->channels();
		std::vector<unsigned long long> m(3 * nch);
		dev_download(m.data(), h->d_meters, h->meter_bytes(), stream); // (waits for `stream`)
		// (peak: the bit pattern of a non-negative double; the counts never reach 2^63)
		if (peak) memcpy(peak, m.data(), nch * sizeof(double));
		if (clipped) memcpy(clipped, m.data() + nch, nch * sizeof(long long));
		if (nonfinite) memcpy(nonfinite, m.data() + 2 * nch, nch * sizeof(long long));
		if (reset) dev_zero(h->d_meters, h->meter_bytes(), stream);
		return 0;
	}
	catch (const std::exception& e)
	{
		set_err("r8b_batch_meter_read", e);
		return -1;
	}
}

R8BSRC_DECL int r8b_batch_true_peak_enable(CR8BBatch b, int on)
{
	try
	{
		Batch* const h = need(b);
		if (on && h->d_tp == nullptr)
		{
			DevGuard guard(h->eng->device());
			h->d_tp = (double*) dev_alloc(h->tp_bytes()); // (zeroed)
		}
		// (switched on in mid-stream: the frames that passed meanwhile are not in the history)
		if (on && !h->tp_on && h->streaming()) h->tp_drop_history();
		h->tp_on = on != 0;
		return 0;
	}
	catch (const std::exception& e)
	{
		set_err("r8b_batch_true_peak_enable", e);
		return -1;
	}
}

R8BSRC_DECL int r8b_batch_true_peak_read(CR8BBatch b, double* true_peak, int reset, void* stream)
{
	try
	{
		Batch* const h = need(b);
		if (h->d_tp == nullptr) throw std::runtime_error("the object's true-peak meter was never enabled");
		DevGuard guard(h->eng->device());
		const size_t bytes = (size_t) h->eng->channels() * sizeof(double);
		// (the bit pattern of a non-negative double)
		std::vector<double> v((size_t) h->eng->channels());
		dev_download(v.data(), h->d_tp, bytes, stream); // (waits for `stream`)
		if (true_peak) memcpy(true_peak, v.data(), bytes);
		if (reset) dev_zero(h->d_tp, bytes, stream);
		return 0;
	}
	catch (const std::exception& e)
	{
		set_err("r8b_batch_true_peak_read", e);
		return -1;
	}
}

R8BSRC_DECL int r8b_loudness_design(double rate, double* coefs, double* handoff, long long* hop)
{
	try
	{
		// (the shelf is unstable once the rate approaches twice 1682 Hz; a sub-block must fit the kernels' int)
		if (!(rate >= 8000.0 && rate <= 1e10)) throw std::runtime_error("the loudness meter needs a destination rate of 8000 Hz or more");
		double c[10], phi[16];
		long long h;
		loudness_design(rate, c, phi, &h);
		if (coefs) memcpy(coefs, c, sizeof(c));
		if (handoff) memcpy(handoff, phi, sizeof(phi));
		if (hop) *hop = h;
		return 0;
	}
	catch (const std::exception& e)
	{
		set_err("r8b_loudness_design", e);
		return -1;
	}
}

R8BSRC_DECL int r8b_batch_loudness_enable(CR8BBatch b, int on, long long capacity)
{
	try
	{
		Batch* const h = need(b);
		if (on)
		{
			if (!(h->dst_rate >= 8000.0 && h->dst_rate <= 1e10))
				throw std::runtime_error("the loudness meter needs a destination rate of 8000 Hz or more");
			if (capacity < 1 || capacity > (1LL << 40)) throw std::runtime_error("capacity must be at least 1 sub-block");
			const int nch = h->eng->channels();
			if (h->d_ld == nullptr || capacity != h->ld_cap)
			{
				DevGuard guard(h->eng->device());
				dev_free(h->d_ld);
				h->d_ld = nullptr;
				h->d_ld = (double*) dev_alloc(((size_t) kLdStateStride + (size_t) capacity) * nch * sizeof(double)); // (zeroed)
				h->ld_cap = capacity;
				h->ld_count.assign((size_t) nch, 0);
				h->ld_clip = false;
				h->ld_on = false;
			}
			loudness_design(h->dst_rate, h->ld_coef, h->ld_phi, &h->ld_hop);
			// (switched on: meter frame 0 is the next call's first frame)
			if (!h->ld_on) h->ld_restart();
		}
		h->ld_on = on != 0;
		return 0;
	}
	catch (const std::exception& e)
	{
		set_err("r8b_batch_loudness_enable", e);
		return -1;
	}
}

R8BSRC_DECL long long r8b_batch_loudness_read(CR8BBatch b, double* sums, long long stride, long long* counts, int drain,
	void* stream)
{
	try
	{
		Batch* const h = need(b);
		if (h->d_ld == nullptr) throw std::runtime_error("the object's loudness meter was never enabled");
		const int nch = h->eng->channels();
		long long most = 0;
		for (int c = 0; c < nch; c++) most = std::max(most, h->ld_count[c]);
		if (sums != nullptr && stride < most) throw std::runtime_error("stride is smaller than the largest count");
		DevGuard guard(h->eng->device());
		std::vector<double> v((size_t) h->ld_cap * nch);
		dev_download(v.data(), h->d_ld + (size_t) kLdStateStride * nch, v.size() * sizeof(double), stream); // (waits for `stream`)
		for (int c = 0; c < nch; c++)
		{
			if (counts) counts[c] = h->ld_count[c];
			if (sums) memcpy(sums + c * stride, v.data() + (size_t) c * h->ld_cap, (size_t) h->ld_count[c] * sizeof(double));
		}
		if (drain) h->ld_empty();
		return most;
	}
	catch (const std::exception& e)
	{
		set_err("r8b_batch_loudness_read", e);
		return -1;
	}
}

R8BSRC_DECL int r8b_loudness_integrated(const double* sums, long long stride, const long long* counts, int nprog, int Kp,
	const double* weights, long long hop, double* lufs)
{
	try
	{
		if (sums == nullptr || counts == nullptr || lufs == nullptr) throw std::runtime_error("null pointer");
		if (nprog < 0 || Kp < 1 || hop < 1) throw std::runtime_error("nprog, channels per programme and hop must be positive");
		std::vector<double> G;
		for (int p = 0; p < nprog; p++)
		{
			long long nb = counts[(long long) p * Kp];
			for (int i = 1; i < Kp; i++) nb = std::min(nb, counts[(long long) p * Kp + i]);
			G.clear();
			for (long long j = 0; j + 4 <= nb; j++)
			{
				double g = 0.0;
				for (int i = 0; i < Kp; i++)
				{
					const double* s = sums + ((long long) p * Kp + i) * stride + j;
					g += (weights ? weights[i] : 1.0) * (s[0] + s[1] + s[2] + s[3]);
				}
				G.push_back(g / (4.0 * (double) hop));
			}
			auto lu = [](double g) { return -0.691 + 10.0 * log10(g); };
			// the absolute gate, then the relative one 10 LU below the loudness of what passed it
			double sum = 0.0;
			long long cnt = 0;
			for (double g : G)
				if (lu(g) > -70.0)
				{
					sum += g;
					cnt++;
				}
			lufs[p] = -HUGE_VAL;
			if (cnt == 0) continue;
			const double gate = lu(sum / (double) cnt) - 10.0;
			sum = 0.0;
			cnt = 0;
			for (double g : G)
				if (lu(g) > -70.0 && lu(g) > gate)
				{
					sum += g;
					cnt++;
				}
			if (cnt != 0) lufs[p] = lu(sum / (double) cnt);
		}
		return 0;
	}
	catch (const std::exception& e)
	{
		set_err("r8b_loudness_integrated", e);
		return -1;
	}
}

R8BSRC_DECL int r8b_pcm_sample_bytes(int format)
{
	return pcm_io_bytes(format);
}

R8BSRC_DECL long long r8b_batch_state_size(CR8BBatch b)
{
	return (long long) ((Batch*) b)->eng->state_size();
}

R8BSRC_DECL long long r8b_batch_state_save(CR8BBatch b, void* buf, long long cap, void* stream)
{
	try
	{
		return (long long) need(b)->eng->save_state(buf, cap < 0 ? 0 : (size_t) cap, stream);
	}
	catch (const std::exception& e)
	{
		set_err("r8b_batch_state_save", e);
		return -1;
	}
}

R8BSRC_DECL int r8b_batch_state_load(CR8BBatch b, const void* buf, long long size, void* stream)
{
	try
	{
		Batch* const h = need(b);
		h->eng->load_state(buf, size < 0 ? 0 : (size_t) size, stream);
		h->tp_drop_history();
		h->ld_restart();
		return 0;
	}
	catch (const std::exception& e)
	{
		set_err("r8b_batch_state_load", e);
		return -1;
	}
}

R8BSRC_DECL int r8b_batch_describe(CR8BBatch b, char* buf, int cap)
{
	return copy_text(((Batch*) b)->eng->plan().describe(), buf, cap);
}

R8BSRC_DECL int r8b_batch_set_option(CR8BBatch b, const char* name, int value)
{
	return ((Batch*) b)->eng->set_option(name, value) ? 0 : -1;
}

R8BSRC_DECL double r8b_batch_latency_frac(CR8BBatch b)
{
	// (what the last stage hands on: reference CDSPResampler.h:688, addProcessor)
	const r8bhip::ChainPlan& pl = ((Batch*) b)->eng->plan();
	return pl.stages.empty() ? 0.0 : pl.stages.back().lat_frac;
}

R8BSRC_DECL long long r8b_batch_stat(CR8BBatch b, const char* name)
{
	return name != nullptr ? ((Batch*) b)->eng->stat(name) : -1;
}

R8BSRC_DECL int r8b_batch_stage_count(CR8BBatch b)
{
	return (int) ((Batch*) b)->eng->plan().stages.size();
}

R8BSRC_DECL int r8b_batch_stage_timing(CR8BBatch b, int stage, double* ms_sum, int* launches,
	long long* in_samples, long long* out_samples, char* kernel, int cap)
{
	try
	{
		std::string name;
		if (!need(b)->eng->stage_timing((size_t) stage, ms_sum, launches, &name,
			in_samples, out_samples)) return -1;
		copy_text(name, kernel, cap);
		return 0;
	}
	catch (const std::exception& e)
	{
		set_err("r8b_batch_stage_timing", e);
		return -1;
	}
}

R8BSRC_DECL int r8b_batch_stage_symbol(CR8BBatch b, int stage, char* symbol, int cap)
{
	try
	{
		Batch* B = need(b);
		if (stage == R8B_STAGE_PCM_IN || stage == R8B_STAGE_PCM_OUT)
		{
			copy_text(B->eng->pcm_symbol(stage == R8B_STAGE_PCM_IN ? 0 : 1), symbol, cap);
			return 0;
		}
		if (stage < 0 || stage >= (int) B->eng->plan().stages.size()) return -1;
		copy_text(B->eng->stage_symbol((size_t) stage), symbol, cap);
		return 0;
	}
	catch (const std::exception& e)
	{
		set_err("r8b_batch_stage_symbol", e);
		return -1;
	}
}

// ---------------------------------------------------------------- drop-in single-stream ABI

R8BSRC_DECL CR8BResampler r8b_create(double SrcSampleRate, double DstSampleRate, int MaxInLen,
	double ReqTransBand, enum ER8BResamplerRes Res)
{
	try
	{
		std::unique_ptr<Single> s(new Single());
		s->b.eng.reset(new Engine(build_topology(SrcSampleRate, DstSampleRate, ReqTransBand,
			res_atten((int) Res)), MaxInLen, 1, -1));
		s->out.resize((size_t) (s->b.eng->plan().max_out_len > 0 ?
			s->b.eng->plan().max_out_len : 1));
		g_err.clear();
		return s.release();
	}
	catch (const std::exception& e)
	{
		// the reference has no error path; a missing GPU must not go unnoticed
		set_err("r8b_create", e);
		fprintf(stderr, "r8bsrc-hip: %s\n", g_err.c_str());
		return nullptr;
	}
}

R8BSRC_DECL void r8b_delete(CR8BResampler rs) { delete (Single*) rs; }

R8BSRC_DECL int r8b_inlen(CR8BResampler rs, int ReqOutSamples)
{
	return ((Single*) rs)->b.eng->plan().input_required(ReqOutSamples);
}

R8BSRC_DECL void r8b_clear(CR8BResampler rs) { ((Single*) rs)->b.eng->clear(); }

R8BSRC_DECL int r8b_process(CR8BResampler rs, double* ip0, int l, double*& op0)
{
	Single* s = (Single*) rs;
	try
	{
		if (s->b.eng->plan().stages.empty())
		{
			op0 = ip0; // reference CDSPResampler.h:534-535
			return l;
		}
		op0 = s->out.data();
		return batch_process_host(&s->b, ip0, l, l, s->out.data(), (long long) s->out.size());
	}
	catch (const std::exception& e)
	{
		set_err("r8b_process", e);
		fprintf(stderr, "r8bsrc-hip: %s\n", g_err.c_str());
		op0 = s->out.data();
		return 0;
	}
}

// ---------------------------------------------------------------- designer / plan queries

R8BSRC_DECL int r8b_design_lpfilter(double ReqNormFreq, double ReqTransBand, double ReqAtten,
	double ReqGain, int* BlockLenBits, int* Latency, double* taps, int cap)
{
	const LpFilterRef fr = design_lp(ReqNormFreq, ReqTransBand, ReqAtten, ReqGain);
	const LpFilter& f = *fr;
	if (BlockLenBits) *BlockLenBits = f.block_len_bits;
	if (Latency) *Latency = f.fl2;
	if (taps)
		memcpy(taps, f.taps.data(), sizeof(double) * (size_t) (f.kernel_len < cap ? f.kernel_len : cap));
	return f.kernel_len;
}

R8BSRC_DECL int r8b_design_lpfilter_ex(double ReqNormFreq, double ReqTransBand, double ReqAtten,
	double ReqGain, int ReqPhase, int* BlockLenBits, int* Latency, double* LatencyFrac, double* taps,
	int cap)
{
	const LpFilterRef fr = design_lp(ReqNormFreq, ReqTransBand, ReqAtten, ReqGain, ReqPhase != 0);
	const LpFilter& f = *fr;
	if (BlockLenBits) *BlockLenBits = f.block_len_bits;
	if (Latency) *Latency = f.fl2;
	if (LatencyFrac) *LatencyFrac = f.lat_frac;
	if (taps)
		memcpy(taps, f.taps.data(), sizeof(double) * (size_t) (f.kernel_len < cap ? f.kernel_len : cap));
	return f.kernel_len;
}

#ifdef R8B_TEST_HOOKS
R8BSRC_DECL void r8b_design_set_lp_provider(r8b_lp_provider provider)
{
	set_lp_provider(reinterpret_cast<LpProvider>(provider));
}

R8BSRC_DECL long long r8b_batch_test_skip_silence(CR8BBatch b, long long n)
{
	try
	{
		Batch* const h = need(b);
		if (h->pass_frames != 0)
			throw std::runtime_error("the object has processed samples since creation / r8b_batch_clear()");
		const long long out = h->eng->test_skip_silence(n, nullptr);
		// (Src == Dst: no stage counts the frames, the handle does -- the dither's frame number)
		if (h->eng->plan().stages.empty()) h->pass_frames += out;
		return out;
	}
	catch (const std::exception& e)
	{
		set_err("r8b_batch_test_skip_silence", e);
		return -1;
	}
}
#endif

R8BSRC_DECL int r8b_design_fracbank(int FilterFracs, int ElementSize, int InterpPoints,
	double ReqAtten, int IsThird, int* FilterLen, int* Fracs, double* table, int cap)
{
	if (!((ElementSize == 1 && InterpPoints == 2) || (ElementSize == 3 && InterpPoints == 8)))
		return -1;
	const FracBankRef br = design_frac_bank(FilterFracs, ElementSize, InterpPoints, ReqAtten,
		IsThird != 0);
	const FracBank& b = *br;
	if (FilterLen) *FilterLen = b.filter_len;
	if (Fracs) *Fracs = b.fracs;
	const int n = (int) b.table.size();
	if (table) memcpy(table, b.table.data(), sizeof(double) * (size_t) (n < cap ? n : cap));
	return n;
}

R8BSRC_DECL void r8b_design_cache_counts(int* Filters, int* FracBanks, int* LaneTables)
{
	int c[3] = { 0, 0, 0 };
	design_cache_counts(c);
	if (Filters) *Filters = c[0];
	if (FracBanks) *FracBanks = c[1];
	if (LaneTables) *LaneTables = c[2];
}

R8BSRC_DECL int r8b_design_hbfilter(double ReqAtten, int SteepIndex, int IsThird, double* taps,
	double* att)
{
	const double* t;
	double a;
	const int n = select_hb_filter(ReqAtten, SteepIndex, IsThird != 0, &t, &a);
	if (taps) memcpy(taps, t, sizeof(double) * (size_t) n);
	if (att) *att = a;
	return n;
}

R8BSRC_DECL int r8b_design_whole_stepping(double SSampleRate, double DSampleRate, int* InStep,
	int* OutStep)
{
	int i = 0, o = 0;
	const bool ok = whole_stepping(SSampleRate, DSampleRate, &i, &o);
	if (InStep) *InStep = i;
	if (OutStep) *OutStep = o;
	return ok ? 1 : 0;
}

R8BSRC_DECL CR8BPlan r8b_plan_create(double SrcSampleRate, double DstSampleRate, int MaxInLen,
	double ReqTransBand, double ReqAtten)
{
	try
	{
		ChainPlan* p = new ChainPlan();
		p->init(build_topology(SrcSampleRate, DstSampleRate, ReqTransBand, ReqAtten), MaxInLen);
		return p;
	}
	catch (const std::exception& e)
	{
		set_err("r8b_plan_create", e);
		return nullptr;
	}
}

R8BSRC_DECL void r8b_plan_delete(CR8BPlan p) { delete (ChainPlan*) p; }
R8BSRC_DECL void r8b_plan_clear(CR8BPlan p) { ((ChainPlan*) p)->clear(); }

R8BSRC_DECL int r8b_plan_step(CR8BPlan p, int l)
{
	ChainPlan* c = (ChainPlan*) p;
	int n = l;
	for (StagePlan& s : c->stages)
	{
		long long a, b;
		s.step(n, &a, &b, nullptr);
		n = (int) (b - a);
	}
	return n;
}

R8BSRC_DECL int r8b_plan_max_out_len(CR8BPlan p)
{
	ChainPlan* c = (ChainPlan*) p;
	return c->stages.empty() ? c->max_in : c->max_out_len;
}

R8BSRC_DECL int r8b_plan_inlen(CR8BPlan p, int n) { return ((ChainPlan*) p)->input_required(n); }

R8BSRC_DECL int r8b_plan_inlen_before_outpos(CR8BPlan p, int pos)
{
	return ((ChainPlan*) p)->in_len_before_out_pos(pos);
}

R8BSRC_DECL int r8b_plan_describe(CR8BPlan p, char* buf, int cap)
{
	return copy_text(((ChainPlan*) p)->describe(), buf, cap);
}

} // extern "C"
