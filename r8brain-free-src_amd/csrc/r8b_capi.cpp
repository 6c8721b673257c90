// r8b_capi.cpp -- the C ABI of include/r8bsrc.h over r8bhip::Engine.
#include "../../include/r8bsrc.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "r8b_engine.h"
#include "r8b_meters.h"

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

} // namespace r8bhip

namespace {

thread_local std::string g_err;

void set_err(const char* where, const std::exception& e)
{
	g_err = std::string(where) + ": " + e.what();
}

// An entry's body under the C ABI's error rule: what it throws goes to r8b_last_error() behind the entry's name, and the
// entry returns `fail`
template<class Body>
auto guarded(const char* entry, Body body, decltype(body()) fail = -1) -> decltype(body())
{
	try
	{
		return body();
	}
	catch (const std::exception& e)
	{
		set_err(entry, e);
		return fail;
	}
}

struct Batch
{
	std::unique_ptr<Engine> eng;
	// staging for the host-pointer entry points
	double* d_in = nullptr;
	double* d_out = nullptr;
	long long in_cap = 0, out_cap = 0; // per-channel capacities
	// PCM egress finish (r8b_batch_set_dither) and the meters beside it (r8b_meters.h): settings of the handle, not of the
	// engine -- they are no engine option, enter no configuration hash and no checkpoint.  Each event of a stream's life
	// names the meters it concerns one after the other, in one place: clear(), meters_need_staging() and meter_launches()
	// below, r8b_batch_state_load, and admission, beginning and end (Finish) of a clip call in batch_resample_clips
	int dither_mode = 0, first_channel = 0;
	unsigned long long seed = 0;
	PeakMeters peak;
	TruePeakMeter tp;
	LoudnessMeter ld;
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
		for (ClipSlot& s : clip_slot)
		{
			dev_free(s.d_len);
			dev_free(s.d_mix);
			dev_event_destroy(s.done);
		}
	}
	// whether the stream has taken samples since creation / clear() (the clip entries' "fresh object" rule)
	bool streaming() const { return eng->plan().stages.empty() ? pass_frames != 0 : eng->plan().stages.front().m != 0; }
	void count_pass(int n)
	{
		if (n > 0 && eng->plan().stages.empty()) pass_frames += n;
	}
	// r8b_batch_clear: the stream starts again, and so does what the meters have measured
	void clear()
	{
		eng->clear();
		pass_frames = 0;
		peak.cleared(*eng);
		tp.cleared(*eng);
		ld.cleared();
	}
	// a meter that reads the staging rows, or rides in the finishing egress kernel that does (r8b_pcm.h)
	bool meters_need_staging() const { return peak.on || tp.on || ld.on; }
	// whether an egress into format fmt is dithered (integer formats; the float ones ignore the setting)
	bool dithers(int fmt) const { return dither_mode != 0 && pcm_io_dithers(fmt); }
	// the finish of an egress launch into P.fmt: the dither, keyed by the launch's first absolute frame, and the peak meters
	void egress_finish(PcmLaunch& P, long long frame0) const
	{
		if (dithers(P.fmt))
		{
			P.dither = dither_mode;
			P.seed = seed;
			P.first_channel = first_channel;
			P.frame0 = frame0;
		}
		peak.fill(P);
	}
	// n frames of rows [0, nch) of the output side's staging rows, as the meters' launches take them
	MeterRows staged_rows(int nch, long long n, void* stream) const { return MeterRows{d_out, out_cap, nch, n, stream}; }
	// the meters' launches beside an egress launch
	void meter_launches(const MeterRows& R)
	{
		tp.launch(R);
		ld.launch(R);
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

// The frames a call of l input frames yields: the plan's stages stepped one after the other.  The plan moves with it --
// a copy, to ask only
long long plan_advance(ChainPlan& plan, int l)
{
	long long n = l;
	for (StagePlan& sp : plan.stages)
	{
		long long a, b;
		sp.step((int) n, &a, &b, nullptr);
		n = b - a;
	}
	return n;
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
	if (pcm_io_bytes(in_fmt) == 0 || pcm_io_bytes(out_fmt) == 0) throw std::runtime_error("unknown PCM sample format");
	if (l < 0 || l > e.plan().max_in) throw std::runtime_error("input length exceeds MaxInLen");
	boundary_begin(e);
	if (l == 0) return 0;
	// Src == Dst has no stage to fuse into: both sides staged
	const bool pass = e.plan().stages.empty();
	// the loudness store must take what this call completes: refused here, before anything is enqueued
	// (the probe steps a copy of the plan: only for a meter that asks)
	h->ld.admit([&]
	{
		ChainPlan probe = e.plan();
		return plan_advance(probe, l);
	});
	// ... and so has a planar PCM side whose first / last stage is a compile-time-sized convolver (fp64 views only)
	// ... and so has every side in a one-byte format: the stage kernels' codec does not know them (r8b_pcm_codec.h)
	const bool stage_in = in_interleaved || pass || (in_fmt != kPcmF64 && !e.pcm_fused_in()) || pcm_io_bytes(in_fmt) == 1;
	// ... and so has every output side while dither or a meter is on: the finishing egress kernels do the dither and the
	// peak meters (r8b_pcm.h), the other meters read the staging rows
	const bool stage_out = out_interleaved || pass || h->dithers(out_fmt) || h->meters_need_staging() ||
		(out_fmt != kPcmF64 && !e.pcm_fused_out()) || pcm_io_bytes(out_fmt) == 1;
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
		h->egress_finish(P, frame0);
		boundary_launch(e, 1, P, stream);
		h->meter_launches(h->staged_rows(P.nch, n, stream));
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

// A block of a clip call's slot, enlarged to `want` elements when the slot is taken, i.e. behind its event: no kernel
// reads the block that is replaced
template<class T>
void slot_grow(T*& d, size_t& cap, size_t want)
{
	if (cap >= want) return;
	dev_free(d);
	d = nullptr;
	cap = 0;
	d = (T*) dev_alloc(want * sizeof(T));
	dev_sync(nullptr); // (dev_alloc zeroes on the null stream, which a non-blocking `stream` does not follow)
	cap = want;
}

// One side of a clip call, as the caller describes its buffer: the entries fill the first six fields, in the order of
// their own arguments
struct ClipSide
{
	const void* buf = nullptr;
	int fmt = 0, interleaved = 0;
	long long stride = 0;              // strided: row c (planar) or clip i (interleaved) starts at c / i times this
	const long long* off = nullptr;    // packed: clip i's region starts at element off[i] and the stride is ignored
	const long long* len = nullptr;    // one entry per clip
	int channels = 0;                  // of a clip in the buffer: batch_resample_clips fills in K, or Kin on a mixing input
	// (one channel per clip: a frame-major clip IS a row)
	bool frames() const { return interleaved && channels > 1; }
	// bases per clip (PcmLaunch::clip_base): one per row of a planar side, one per clip of an interleaved one
	int rows() const { return frames() ? 1 : channels; }
	void check_stride(long long longest, const char* text) const
	{
		if (off == nullptr && stride < longest * (frames() ? channels : 1)) throw std::runtime_error(text);
	}
	void check_offset(int clip, const char* text) const
	{
		if (off != nullptr && off[clip] < 0) throw std::runtime_error(text);
	}
	bool misaligned() const { return fmt == kPcmF64 && ((size_t) buf & 7) != 0; }
	// (one length per channel, the clip's: the masked row kernels read their row's, the tile kernels the clip's first)
	void push_lengths(std::vector<long long>& host, const std::vector<int>& order, int K) const
	{
		for (int clip : order) host.insert(host.end(), (size_t) K, len[clip]);
	}
	// a packed side: a planar side's row k of clip i starts k clip lengths behind the clip's offset; a strided side (of an
	// ordered call): clip i's rows or region where the stride puts them
	void push_bases(std::vector<long long>& host, const std::vector<int>& order) const
	{
		for (int clip : order)
			for (int k = 0; k < rows(); k++)
				host.push_back(off != nullptr ? off[clip] + k * len[clip] : ((long long) clip * rows() + k) * stride);
	}
	// the side's launch on nch staging rows of `cap` frames: lengths and bases (null: none) are DEVICE arrays
	PcmLaunch launch(int nch, int K, double* staging, long long cap, const long long* d_len, const long long* d_base) const
	{
		PcmLaunch L;
		L.nch = nch;
		L.interleaved = frames() ? 1 : 0;
		L.clip_channels = K;
		L.pcm = const_cast<void*>(buf);
		L.fmt = fmt;
		L.pcm_stride = stride;
		L.planar = staging;
		L.planar_stride = cap;
		L.clip_len = d_len;
		L.clip_base = d_base;
		return L;
	}
};

// A clip call (include/r8bsrc.h r8b_batch_resample_clips ... _sched; the entries fill it in)
struct ClipCall
{
	int K = 1;                    // clip_channels: clip i is object channels i K .. i K + K - 1
	int Kin = 0;                  // != 0: the input side holds Kin channels per clip and the ingest mixes them to K by `mix`
	const double* mix = nullptr;  // the K x Kin HOST matrix (the entry has checked Kin's range and the pointer)
	ClipSide in, out;
	int flags = 0;
	void* stream = nullptr;
};

// A batch of clips of unequal length in one call (include/r8bsrc.h r8b_batch_resample_clips): the loop a host would
// write around r8b_batch_process_pcm -- MaxInLen frames per step, zeros once the clips have ended, until the last
// output has come out (reference CDSPResampler.h:592-651, bench/r8bfreesrc.cpp:92-136) -- with both sides going through
// the staging rows and the masked row kernels of r8b_clip.h, which know every clip's length.
// K: clip i is channels i K .. i K + K - 1 and has one entry in each length array; a side is planar (row c at
// c * stride) or, with K > 1, may hold the clips frame-major (clip i at i * stride: r8b_clip_frames.h).
// Kin != 0 (r8b_batch_resample_clips_mix): the input side holds Kin channels per clip in either layout and the
// ingest mixes them down (or up) to the K object channels (r8b_clip_mix.h); the matrix travels as the lengths do,
// through a host and a device block of the call's slot.
// A side's off != nullptr (r8b_batch_resample_clips_packed): that side is packed -- a clip's region holds its channels at
// the clip's own length (r8b_clip_packed.h).  The kernels get one base per row of a planar side and one per clip of an
// interleaved one, worked out here and sent through the slot behind the lengths.
// flags (r8b_batch_resample_clips_sched; 0: none of this, the calls above as they always ran):
//   R8B_CLIPS_LONGEST_FIRST  clip order[g] rides in slot g = staging rows and object channels g K .. g K + K - 1
//     (clip_order: by output length, longest first).  Everything the kernels read per row or per clip -- lengths, bases --
//     is filled here in slot order, a strided side gets bases too (row or clip times the stride), and the egress learns
//     each row's channel in the caller's numbering (PcmLaunch::clip_chan: dither key, meters) and whether to store the
//     padding behind a base (PcmLaunch::clip_pad: a strided output); r8b_clip_sched.h.
//   R8B_CLIPS_DROP_FINISHED  a step's ingest and stages run channels [0, A) only (clip_active: the slots that still owe
//     outputs, as whole clips and whole channel pairs); a packed egress covers the same rows, a strided one every row --
//     a finished row's frames all lie at or past its length there, so it stores padding and loads nothing.
long long batch_resample_clips(Batch* h, ClipCall c)
{
	Engine& e = *h->eng;
	const int K = c.K;
	const bool mixing = c.Kin != 0;
	if ((c.flags & ~(R8B_CLIPS_DROP_FINISHED | R8B_CLIPS_LONGEST_FIRST)) != 0)
		throw std::runtime_error("flags holds an unknown bit");
	const bool drop = (c.flags & R8B_CLIPS_DROP_FINISHED) != 0, ordered = (c.flags & R8B_CLIPS_LONGEST_FIRST) != 0;
	if (pcm_io_bytes(c.in.fmt) == 0 || pcm_io_bytes(c.out.fmt) == 0) throw std::runtime_error("unknown PCM sample format");
	if (c.in.len == nullptr || c.out.len == nullptr) throw std::runtime_error("null length array");
	const int nch = e.channels();
	if (K < 1 || K > kClipChannelsMax) throw std::runtime_error("clip_channels must be 1 .. 64");
	if (nch % K != 0) throw std::runtime_error("clip_channels does not divide the object's channel count");
	const int nclips = nch / K;
	if (mixing)
		for (int j = 0; j < K * c.Kin; j++)
			if (!(c.mix[j] - c.mix[j] == 0.0)) throw std::runtime_error("mix holds a coefficient that is not finite");
	c.in.channels = mixing ? c.Kin : K;
	c.out.channels = K;
	long long max_in = 0, P = 0;
	for (int i = 0; i < nclips; i++)
	{
		if (c.in.len[i] < 0 || c.out.len[i] < 0) throw std::runtime_error("negative clip length");
		if (c.in.len[i] > max_in) max_in = c.in.len[i];
		if (c.out.len[i] > P) P = c.out.len[i];
	}
	if (h->streaming()) throw std::runtime_error("the object has processed samples since creation / r8b_batch_clear()");
	c.in.check_stride(max_in, "in_stride is smaller than the longest clip");
	c.out.check_stride(P, "out_stride is smaller than the longest output");
	for (int i = 0; i < nclips; i++)
	{
		c.in.check_offset(i, "in_offset holds a negative offset");
		c.out.check_offset(i, "out_offset holds a negative offset");
	}
	if (c.out.off != nullptr)
	{
		// two clips must not be written to the same elements (inputs may share theirs): the non-empty regions in order
		std::vector<std::pair<long long, long long>> reg;
		for (int i = 0; i < nclips; i++)
			if (c.out.len[i] > 0) reg.emplace_back(c.out.off[i], c.out.off[i] + c.out.len[i] * K);
		std::sort(reg.begin(), reg.end());
		for (size_t j = 1; j < reg.size(); j++)
			if (reg[j].first < reg[j - 1].second) throw std::runtime_error("out_offset: the regions of two clips overlap");
	}
	// the loudness store must take the longest clip's sub-blocks: refused here, before anything is enqueued
	h->ld.admit_clips(P);
	boundary_begin(e);
	// the loudness meter's call begins HERE, in front of the refusals below: a call they refuse has emptied the store and
	// left the clips' counts (observable, and kept).  The true-peak meter's begins where nothing refuses any more
	h->ld.clip_begin(K, c.out.len);
	if (P == 0) return 0;
	if (c.out.buf == nullptr || (c.in.buf == nullptr && max_in > 0)) throw std::runtime_error("null device pointer");
	if (c.in.misaligned() || c.out.misaligned()) throw std::runtime_error("fp64 buffers must be 8-byte aligned");
	DevGuard guard(e.device());
	h->need_staging();
	// the lengths: into the next slot, uploaded on `stream` in front of this call's kernels
	Batch::ClipSlot& slot = h->clip_slot[h->clip_next];
	h->clip_next = (h->clip_next + 1) % Batch::kClipSlots;
	if (slot.done == nullptr) slot.done = dev_event_create();
	// (the call made kClipSlots calls ago: waits only while all the slots are in flight)
	if (slot.used) dev_event_elapsed_ms(slot.done, slot.done);
	// the bases behind the lengths: a packed side has them, and both sides of an ordered call, whose rows' object channels
	// lie behind them in turn
	const size_t in_bases = c.in.off == nullptr && !ordered ? 0 : (size_t) nclips * c.in.rows();
	const size_t out_bases = c.out.off == nullptr && !ordered ? 0 : (size_t) nclips * c.out.rows();
	const size_t entries = (size_t) 2 * nch + in_bases + out_bases + (ordered ? nch : 0);
	// order[g]: the clip in slot g
	std::vector<int> order((size_t) nclips);
	clip_order(nclips, c.out.len, ordered, order.data());
	slot_grow(slot.d_len, slot.len_cap, entries);
	slot.host.clear();
	c.in.push_lengths(slot.host, order, K);
	c.out.push_lengths(slot.host, order, K);
	if (in_bases != 0) c.in.push_bases(slot.host, order);
	if (out_bases != 0) c.out.push_bases(slot.host, order);
	for (int r = 0; ordered && r < nch; r++) slot.host.push_back((long long) order[r / K] * K + r % K);
	dev_upload_async(slot.d_len, slot.host.data(), slot.host.size() * sizeof(long long), c.stream);
	slot.used = true;
	if (mixing)
	{
		const size_t count = (size_t) K * c.Kin;
		slot_grow(slot.d_mix, slot.mix_cap, count);
		slot.host_mix.assign(c.mix, c.mix + count);
		dev_upload_async(slot.d_mix, slot.host_mix.data(), count * sizeof(double), c.stream);
	}
	// whatever happens below, the object is left as after r8b_batch_clear() (but for the meters' values: the kernels may
	// still be in flight, and the caller reads them afterwards), and the slot knows when this call's last launch is through
	struct Finish
	{
		Batch* h;
		Batch::ClipSlot& slot;
		void* stream;
		~Finish()
		{
			h->eng->clear();
			h->pass_frames = 0;
			h->tp.clip_end();
			h->ld.clip_end();
			try { dev_event_record(slot.done, stream); }
			catch (const std::exception&) {}
		}
	} finish{h, slot, c.stream};
	const long long* const bases = slot.d_len + 2 * nch;
	const int l = (int) h->in_cap;
	PcmLaunch I = c.in.launch(nch, K, h->d_in, h->in_cap, slot.d_len, in_bases != 0 ? bases : nullptr);
	I.n = l;
	if (mixing)
	{
		I.mix_channels = c.Kin;
		I.mix = slot.d_mix;
	}
	PcmLaunch O = c.out.launch(nch, K, h->d_out, h->out_cap, slot.d_len + nch, out_bases != 0 ? bases + in_bases : nullptr);
	if (ordered)
	{
		O.clip_chan = bases + in_bases + out_bases;
		O.clip_pad = c.out.off == nullptr ? 1 : 0;
	}
	h->egress_finish(O, 0);
	h->tp.clip_begin();
	MeterRows R = h->staged_rows(nch, 0, c.stream);
	R.clip_len = O.clip_len;
	R.clip_chan = O.clip_chan;
	bool zeroed = false;
	// (outputs past P are never asked for: the loop ends with the last one, as the reference's oneshot() does)
	for (long long pos = 0, done = 0; done < P; pos += l)
	{
		// the channels this step runs: all of them, or those of the slots that still owe outputs
		const int A = drop ? clip_active(nclips, K, c.out.len, order.data(), done) : nch;
		if (pos < max_in)
		{
			I.in_frame0 = pos;
			I.nch = A;
			boundary_launch(e, 0, I, c.stream);
		}
		else if (!zeroed)
		{
			// every clip has ended: the staging rows are zeros from here on (A only shrinks)
			dev_zero(h->d_in, (size_t) h->in_cap * A * sizeof(double), c.stream);
			zeroed = true;
		}
		const int n = e.process(h->d_in, h->in_cap, l, h->d_out, h->out_cap, c.stream, A);
		e.bump(kClipSteps);
		e.bump(kClipChannelSteps, A);
		if (n > 0)
		{
			O.frame0 = done;
			O.n = n < P - done ? n : P - done;
			// (a side that stores padding covers every row: a finished row gets its zeros up to P)
			O.nch = c.out.off != nullptr ? A : nch;
			boundary_launch(e, 1, O, c.stream);
			// (rows [0, A): a dropped row's clip has ended, and its tail was metered by the step that held its last frame)
			R.nch = A;
			R.n = O.n;
			R.frame0 = done;
			h->meter_launches(R);
		}
		done += n;
	}
	return P;
}

// The three r8b_batch_create* entries: an object over the stages that stages() yields (it refuses what the entry refuses)
template<class Stages>
CR8BBatch batch_create(const char* entry, int MaxInLen, int nch, int device, double dst_rate, Stages stages)
{
	return guarded(entry, [&]() -> CR8BBatch
	{
		std::unique_ptr<Batch> b(new Batch());
		b->eng.reset(new Engine(stages(), MaxInLen, nch, device));
		b->ld.rate = dst_rate;
		g_err.clear();
		return b.release();
	}, nullptr);
}

// r8b_batch_resample_clips_packed and _sched: without a matrix nothing is mixed, and in_channels says so or agrees with
// clip_channels.  Returns ClipCall::Kin
int clip_mix_channels(int in_channels, int clip_channels, const double* mix)
{
	if (mix == nullptr)
	{
		if (in_channels != 0 && in_channels != clip_channels)
			throw std::runtime_error("in_channels must be 0 or clip_channels when mix is NULL");
		return 0;
	}
	if (in_channels < 1 || in_channels > kClipChannelsMax) throw std::runtime_error("in_channels must be 1 .. 64");
	return in_channels;
}

} // namespace

extern "C" {

R8BSRC_DECL const char* r8b_last_error(void) { return g_err.c_str(); }
R8BSRC_DECL const char* r8b_version(void) { return "r8bsrc-hip 0.1 (gfx950; tracks r8brain-free-src 7.1 semantics)"; }

// ---------------------------------------------------------------- batch object

R8BSRC_DECL CR8BBatch r8b_batch_create(double SrcSampleRate, double DstSampleRate, int MaxInLen,
	double ReqTransBand, double ReqAtten, int nch, int device)
{
	return batch_create("r8b_batch_create", MaxInLen, nch, device, DstSampleRate, [&]
	{
		return build_topology(SrcSampleRate, DstSampleRate, ReqTransBand, ReqAtten);
	});
}

R8BSRC_DECL CR8BBatch r8b_batch_create_ex(double SrcSampleRate, double DstSampleRate, int MaxInLen,
	double ReqTransBand, double ReqAtten, int ReqPhase, int nch, int device)
{
	return batch_create("r8b_batch_create_ex", MaxInLen, nch, device, DstSampleRate, [&]
	{
		if (ReqPhase != kLinearPhase && ReqPhase != kMinPhase)
			throw std::runtime_error("ReqPhase must be 0 (linear phase) or 1 (minimum phase)");
		return build_topology(SrcSampleRate, DstSampleRate, ReqTransBand, ReqAtten, ReqPhase);
	});
}

R8BSRC_DECL CR8BBatch r8b_batch_create_stage(int kind, double a, double b, double c, double d,
	int i0, int i1, int MaxInLen, int nch, int device)
{
	// (an object made of one stage has no destination rate)
	return batch_create("r8b_batch_create_stage", MaxInLen, nch, device, 0.0, [&]
	{
		if (kind < 0 || kind > 3) throw std::runtime_error("stage kind must be 0 (convolver), 1 "
			"(interpolator), 2 (half-band up) or 3 (half-band down)");
		StageDesc sd;
		sd.kind = (StageKind) kind;
		sd.a = a; sd.b = b; sd.c = c; sd.d = d; sd.i0 = i0; sd.i1 = i1;
		return std::vector<StageDesc>(1, sd);
	});
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
	return guarded("r8b_batch_process", [&]() -> int
	{
		Batch* const h = need(b);
		const int n = h->eng->process(d_in, in_stride, l, d_out, out_stride, stream);
		h->count_pass(n);
		return n;
	});
}

R8BSRC_DECL int r8b_batch_process_host(CR8BBatch b, const double* in, long long in_stride, int l,
	double* out, long long out_stride)
{
	return guarded("r8b_batch_process_host", [&] { return batch_process_host(need(b), in, in_stride, l, out, out_stride); });
}

R8BSRC_DECL int r8b_batch_process_pcm(CR8BBatch b, const void* d_in, int in_format,
	int in_interleaved, long long in_stride, int l, void* d_out, int out_format,
	int out_interleaved, long long out_stride, void* stream)
{
	return guarded("r8b_batch_process_pcm", [&]
	{
		return batch_process_pcm(need(b), d_in, in_format, in_interleaved, in_stride, l, d_out, out_format, out_interleaved,
			out_stride, stream);
	});
}

R8BSRC_DECL long long r8b_clip_out_len(double SrcSampleRate, double DstSampleRate, long long in_len)
{
	// reference bench/r8bfreesrc.cpp:92
	return (long long) ((double) in_len * DstSampleRate / SrcSampleRate);
}

R8BSRC_DECL long long r8b_batch_resample_clips(CR8BBatch b, const void* d_in, int in_format, long long in_stride,
	const long long* in_len, void* d_out, int out_format, long long out_stride, const long long* out_len, void* stream)
{
	return guarded("r8b_batch_resample_clips", [&]() -> long long
	{
		ClipCall c;
		c.in = ClipSide{d_in, in_format, 0, in_stride, nullptr, in_len};
		c.out = ClipSide{d_out, out_format, 0, out_stride, nullptr, out_len};
		c.stream = stream;
		return batch_resample_clips(need(b), c);
	});
}

R8BSRC_DECL long long r8b_batch_resample_clips_ex(CR8BBatch b, int clip_channels, const void* d_in, int in_format,
	int in_interleaved, long long in_stride, const long long* in_len, void* d_out, int out_format, int out_interleaved,
	long long out_stride, const long long* out_len, void* stream)
{
	return guarded("r8b_batch_resample_clips_ex", [&]() -> long long
	{
		ClipCall c;
		c.K = clip_channels;
		c.in = ClipSide{d_in, in_format, in_interleaved, in_stride, nullptr, in_len};
		c.out = ClipSide{d_out, out_format, out_interleaved, out_stride, nullptr, out_len};
		c.stream = stream;
		return batch_resample_clips(need(b), c);
	});
}

R8BSRC_DECL long long r8b_batch_resample_clips_mix(CR8BBatch b, int in_channels, int clip_channels, const double* mix,
	const void* d_in, int in_format, int in_interleaved, long long in_stride, const long long* in_len, void* d_out,
	int out_format, int out_interleaved, long long out_stride, const long long* out_len, void* stream)
{
	return guarded("r8b_batch_resample_clips_mix", [&]() -> long long
	{
		ClipCall c;
		if (in_channels < 1 || in_channels > kClipChannelsMax) throw std::runtime_error("in_channels must be 1 .. 64");
		if (mix == nullptr) throw std::runtime_error("mix is NULL");
		c.K = clip_channels;
		c.Kin = in_channels;
		c.mix = mix;
		c.in = ClipSide{d_in, in_format, in_interleaved, in_stride, nullptr, in_len};
		c.out = ClipSide{d_out, out_format, out_interleaved, out_stride, nullptr, out_len};
		c.stream = stream;
		return batch_resample_clips(need(b), c);
	});
}

R8BSRC_DECL long long r8b_batch_resample_clips_packed(CR8BBatch b, int in_channels, int clip_channels, const double* mix,
	const void* d_in, int in_format, int in_interleaved, long long in_stride, const long long* in_offset,
	const long long* in_len, void* d_out, int out_format, int out_interleaved, long long out_stride,
	const long long* out_offset, const long long* out_len, void* stream)
{
	return guarded("r8b_batch_resample_clips_packed", [&]() -> long long
	{
		ClipCall c;
		c.K = clip_channels;
		c.Kin = clip_mix_channels(in_channels, clip_channels, mix);
		c.mix = mix;
		c.in = ClipSide{d_in, in_format, in_interleaved, in_stride, in_offset, in_len};
		c.out = ClipSide{d_out, out_format, out_interleaved, out_stride, out_offset, out_len};
		c.stream = stream;
		return batch_resample_clips(need(b), c);
	});
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
	return guarded("r8b_batch_resample_clips_sched", [&]() -> long long
	{
		ClipCall c;
		c.K = clip_channels;
		c.Kin = clip_mix_channels(in_channels, clip_channels, mix);
		c.mix = mix;
		c.in = ClipSide{d_in, in_format, in_interleaved, in_stride, in_offset, in_len};
		c.out = ClipSide{d_out, out_format, out_interleaved, out_stride, out_offset, out_len};
		c.flags = flags;
		c.stream = stream;
		return batch_resample_clips(need(b), c);
	});
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
	return guarded("r8b_batch_set_dither", [&]() -> int
	{
		Batch* const h = need(b);
		if (mode != R8B_DITHER_NONE && mode != R8B_DITHER_TPDF)
			throw std::runtime_error("dither mode must be 0 (none) or 1 (TPDF)");
		if (first_channel < 0) throw std::runtime_error("first_channel must not be negative");
		h->dither_mode = mode;
		h->seed = seed;
		h->first_channel = first_channel;
		return 0;
	});
}

R8BSRC_DECL int r8b_batch_meter_enable(CR8BBatch b, int on)
{
	return guarded("r8b_batch_meter_enable", [&]() -> int
	{
		Batch* const h = need(b);
		h->peak.enable(*h->eng, on);
		return 0;
	});
}

R8BSRC_DECL int r8b_batch_meter_read(CR8BBatch b, double* peak, long long* clipped, long long* nonfinite, int reset,
	void* stream)
{
	return guarded("r8b_batch_meter_read", [&]() -> int
	{
		Batch* const h = need(b);
		h->peak.read(*h->eng, peak, clipped, nonfinite, reset, stream);
		return 0;
	});
}

R8BSRC_DECL int r8b_batch_true_peak_enable(CR8BBatch b, int on)
{
	return guarded("r8b_batch_true_peak_enable", [&]() -> int
	{
		Batch* const h = need(b);
		h->tp.enable(*h->eng, on, h->streaming());
		return 0;
	});
}

R8BSRC_DECL int r8b_batch_true_peak_read(CR8BBatch b, double* true_peak, int reset, void* stream)
{
	return guarded("r8b_batch_true_peak_read", [&]() -> int
	{
		Batch* const h = need(b);
		h->tp.read(*h->eng, true_peak, reset, stream);
		return 0;
	});
}

R8BSRC_DECL int r8b_loudness_design(double rate, double* coefs, double* handoff, long long* hop)
{
	return guarded("r8b_loudness_design", [&]() -> int
	{
		loudness_rate_check(rate);
		double c[10], phi[16];
		long long h;
		loudness_design(rate, c, phi, &h);
		if (coefs) memcpy(coefs, c, sizeof(c));
		if (handoff) memcpy(handoff, phi, sizeof(phi));
		if (hop) *hop = h;
		return 0;
	});
}

R8BSRC_DECL int r8b_batch_loudness_enable(CR8BBatch b, int on, long long capacity)
{
	return guarded("r8b_batch_loudness_enable", [&]() -> int
	{
		Batch* const h = need(b);
		h->ld.enable(*h->eng, on, capacity);
		return 0;
	});
}

R8BSRC_DECL long long r8b_batch_loudness_read(CR8BBatch b, double* sums, long long stride, long long* counts, int drain,
	void* stream)
{
	return guarded("r8b_batch_loudness_read", [&]() -> long long
	{
		Batch* const h = need(b);
		return h->ld.read(*h->eng, sums, stride, counts, drain, stream);
	});
}

R8BSRC_DECL int r8b_loudness_integrated(const double* sums, long long stride, const long long* counts, int nprog, int Kp,
	const double* weights, long long hop, double* lufs)
{
	return guarded("r8b_loudness_integrated", [&]() -> int
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
	});
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
	return guarded("r8b_batch_state_save", [&]
	{
		return (long long) need(b)->eng->save_state(buf, cap < 0 ? 0 : (size_t) cap, stream);
	});
}

R8BSRC_DECL int r8b_batch_state_load(CR8BBatch b, const void* buf, long long size, void* stream)
{
	return guarded("r8b_batch_state_load", [&]() -> int
	{
		Batch* const h = need(b);
		h->eng->load_state(buf, size < 0 ? 0 : (size_t) size, stream);
		// (the frames in front of the stream's next one are not the ones the meters saw)
		h->tp.history_lost();
		h->ld.history_lost();
		return 0;
	});
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
	return guarded("r8b_batch_stage_timing", [&]() -> int
	{
		std::string name;
		if (!need(b)->eng->stage_timing((size_t) stage, ms_sum, launches, &name,
			in_samples, out_samples)) return -1;
		copy_text(name, kernel, cap);
		return 0;
	});
}

R8BSRC_DECL int r8b_batch_stage_symbol(CR8BBatch b, int stage, char* symbol, int cap)
{
	return guarded("r8b_batch_stage_symbol", [&]() -> int
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
	});
}

// ---------------------------------------------------------------- drop-in single-stream ABI

R8BSRC_DECL CR8BResampler r8b_create(double SrcSampleRate, double DstSampleRate, int MaxInLen,
	double ReqTransBand, enum ER8BResamplerRes Res)
{
	const CR8BResampler rs = guarded("r8b_create", [&]() -> CR8BResampler
	{
		std::unique_ptr<Single> s(new Single());
		s->b.eng.reset(new Engine(build_topology(SrcSampleRate, DstSampleRate, ReqTransBand,
			res_atten((int) Res)), MaxInLen, 1, -1));
		s->out.resize((size_t) (s->b.eng->plan().max_out_len > 0 ?
			s->b.eng->plan().max_out_len : 1));
		g_err.clear();
		return s.release();
	}, nullptr);
	// the reference has no error path; a missing GPU must not go unnoticed
	if (rs == nullptr) fprintf(stderr, "r8bsrc-hip: %s\n", g_err.c_str());
	return rs;
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
	if (s->b.eng->plan().stages.empty())
	{
		op0 = ip0; // reference CDSPResampler.h:534-535
		return l;
	}
	op0 = s->out.data();
	const int n = guarded("r8b_process", [&] { return batch_process_host(&s->b, ip0, l, l, op0, (long long) s->out.size()); });
	// (the reference has no error path: no samples, and the reason on stderr)
	if (n < 0) fprintf(stderr, "r8bsrc-hip: %s\n", g_err.c_str());
	return n < 0 ? 0 : n;
}

// ---------------------------------------------------------------- designer / plan queries

R8BSRC_DECL int r8b_design_lpfilter(double ReqNormFreq, double ReqTransBand, double ReqAtten,
	double ReqGain, int* BlockLenBits, int* Latency, double* taps, int cap)
{
	// (linear phase, whose fractional latency is 0 and not asked for)
	return r8b_design_lpfilter_ex(ReqNormFreq, ReqTransBand, ReqAtten, ReqGain, 0, BlockLenBits, Latency, nullptr, taps, cap);
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
	return guarded("r8b_batch_test_skip_silence", [&]() -> long long
	{
		Batch* const h = need(b);
		if (h->pass_frames != 0)
			throw std::runtime_error("the object has processed samples since creation / r8b_batch_clear()");
		const long long out = h->eng->test_skip_silence(n, nullptr);
		// (Src == Dst: no stage counts the frames, the handle does -- the dither's frame number)
		if (h->eng->plan().stages.empty()) h->pass_frames += out;
		return out;
	});
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
	return guarded("r8b_plan_create", [&]() -> CR8BPlan
	{
		ChainPlan* p = new ChainPlan();
		p->init(build_topology(SrcSampleRate, DstSampleRate, ReqTransBand, ReqAtten), MaxInLen);
		return p;
	}, nullptr);
}

R8BSRC_DECL void r8b_plan_delete(CR8BPlan p) { delete (ChainPlan*) p; }
R8BSRC_DECL void r8b_plan_clear(CR8BPlan p) { ((ChainPlan*) p)->clear(); }

R8BSRC_DECL int r8b_plan_step(CR8BPlan p, int l) { return (int) plan_advance(*(ChainPlan*) p, l); }

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
