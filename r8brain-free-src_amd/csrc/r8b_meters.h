// r8b_meters.h -- the three meters of the PCM egress as the C ABI layer keeps them (host only; r8b_capi.cpp alone
// includes it): the peak / clip meters (r8b_batch_meter_*), the true-peak meter (r8b_batch_true_peak_*) and the loudness
// meter (r8b_batch_loudness_*).  All three are settings of the handle, not of the engine: no engine option, in no
// configuration hash and no checkpoint.
//
// A struct per meter owns all of it: the device block, the `on` flag, what the host knows of the device's state, the
// bodies of its enable and read entries, and what it does at each event of a stream's life.  Batch (r8b_capi.cpp) holds
// one of each and names them one after the other where the event happens, in one place per event; a meter that does
// nothing at an event has no method for it:
//
//                 the event                                      PeakMeters  TruePeakMeter  LoudnessMeter
//   cleared       r8b_batch_clear                                x           x              x
//   history_lost  r8b_batch_state_load                                       x              x
//   admit*        a call, before anything is enqueued                                       x (it alone refuses)
//   clip_begin    a clip call                                                x              x
//   clip_end      a clip call's end, whatever happened in it                 x              x
//   on            "the output side must be staged"               x           x              x
//   fill          the egress launch's own fields                 x
//   launch        beside an egress launch                                    x              x
//
// cleared and clip_end differ on purpose: clear() zeroes what the meters have measured, while a clip call leaves the object
// as after clear() BUT for the meters' values -- its kernels may still be in flight, and the caller reads them afterwards.
#ifndef R8B_METERS_H
#define R8B_METERS_H

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "r8b_devblock.h"
#include "r8b_engine.h"
// (the meters' constants, ld_frame for loudness_design, and the bodies of r8b_capi.cpp's serial host launch forms)
#ifndef R8B_HD
#define R8B_HD inline
#endif
#include "r8b_truepeak.h"
#include "r8b_loudness.h"

namespace r8bhip {

// (a meter's device block: a DevBlock, r8b_devblock.h -- null until the meter is first enabled)

// What a meter's launch beside an egress launch runs on: n frames of rows [0, nch) of the staging rows and, in a clip
// call, the egress launch's clip fields (TruePeakLaunch and LoudnessLaunch begin with the same)
struct MeterRows
{
	const double* rows;
	long long stride;
	int nch;
	long long n;
	void* stream;
	const long long* clip_len = nullptr;
	long long frame0 = 0;
	const long long* clip_chan = nullptr;
	bool in_clip_call() const { return clip_len != nullptr; }
	template<class Launch>
	Launch as() const
	{
		Launch T;
		T.rows = rows;
		T.stride = stride;
		T.nch = nch;
		T.n = n;
		T.clip_len = clip_len;
		T.frame0 = frame0;
		T.clip_chan = clip_chan;
		return T;
	}
};

// ---------------------------------------------------------------- peak | clipped | nonfinite
// The finishing egress kernels keep them (r8b_pcm.h): no launch of its own
struct PeakMeters
{
	bool on = false;
	DevBlock<unsigned long long> d; // peak | clipped | nonfinite, channels() entries each; allocated on first enable
	size_t bytes = 0;
	int nch = 0;
	void enable(Engine& e, int want)
	{
		if (want && d == nullptr)
		{
			DevGuard guard(e.device());
			nch = e.channels();
			bytes = (size_t) 3 * nch * sizeof(unsigned long long);
			d.alloc(bytes);
		}
		on = want != 0;
	}
	void read(Engine& e, double* peak, long long* clipped, long long* nonfinite, int reset, void* stream)
	{
		if (d == nullptr) throw std::runtime_error("the object's meters were never enabled");
		DevGuard guard(e.device());
		std::vector<unsigned long long> m((size_t) 3 * nch);
		dev_download(m.data(), d, bytes, stream); // (waits for `stream`)
		// (peak: the bit pattern of a non-negative double; the counts never reach 2^63)
		if (peak) memcpy(peak, m.data(), (size_t) nch * sizeof(double));
		if (clipped) memcpy(clipped, m.data() + nch, (size_t) nch * sizeof(long long));
		if (nonfinite) memcpy(nonfinite, m.data() + 2 * nch, (size_t) nch * sizeof(long long));
		if (reset) dev_zero(d, bytes, stream);
	}
	void cleared(Engine& e)
	{
		if (d == nullptr) return;
		DevGuard guard(e.device());
		dev_zero(d, bytes, nullptr);
	}
	void fill(PcmLaunch& P) const
	{
		if (!on) return;
		P.m_peak = d;
		P.m_clipped = P.m_peak + nch;
		P.m_nonfinite = P.m_clipped + nch;
	}
};

// ---------------------------------------------------------------- true peak (r8b_truepeak.h)
// d: channels() values, then two history arrays of kTpHistStride doubles per channel, taken in turn -- cur is the one the
// next launch reads, live whether it holds the stream's last frames (false: they read as zeros); the y of the next skip
// frames are not metered (the history refills)
struct TruePeakMeter
{
	bool on = false, live = false;
	DevBlock<double> d;
	size_t bytes = 0;
	int nch = 0, cur = 0, skip = 0;
	// streaming: the stream has taken samples since creation / clear()
	void enable(Engine& e, int want, bool streaming)
	{
		if (want && d == nullptr)
		{
			DevGuard guard(e.device());
			nch = e.channels();
			bytes = (size_t) (1 + 2 * kTpHistStride) * nch * sizeof(double);
			d.alloc(bytes);
		}
		// (switched on in mid-stream: the frames that passed meanwhile are not in the history)
		if (want && !on && streaming) history_lost();
		on = want != 0;
	}
	void read(Engine& e, double* true_peak, int reset, void* stream)
	{
		if (d == nullptr) throw std::runtime_error("the object's true-peak meter was never enabled");
		DevGuard guard(e.device());
		const size_t values = (size_t) nch * sizeof(double);
		// (the bit pattern of a non-negative double)
		std::vector<double> v((size_t) nch);
		dev_download(v.data(), d, values, stream); // (waits for `stream`)
		if (true_peak) memcpy(true_peak, v.data(), values);
		if (reset) dev_zero(d, values, stream);
	}
	// values and history
	void cleared(Engine& e)
	{
		if (d)
		{
			DevGuard guard(e.device());
			dev_zero(d, bytes, nullptr);
		}
		live = false;
		skip = 0;
	}
	// the history is gone (a checkpoint was loaded, the meter was off for a while): zeros, and the next 11 frames only refill it
	void history_lost()
	{
		live = false;
		skip = kTpHist;
	}
	// zero history at the start of a clip call (the object is fresh), carried from step to step
	void clip_begin()
	{
		live = false;
		skip = 0;
	}
	void clip_end() { live = false; }
	void launch(const MeterRows& R)
	{
		if (!on) return;
		TruePeakLaunch T = R.as<TruePeakLaunch>();
		double* const hist = d + nch;
		const size_t one = (size_t) kTpHistStride * nch;
		T.skip = skip < R.n ? skip : (int) R.n;
		T.hist_in = live ? hist + one * cur : nullptr;
		T.hist_out = hist + one * (cur ^ 1);
		T.values = reinterpret_cast<unsigned long long*>(d.p);
		launch_true_peak(T, R.stream);
		cur ^= 1;
		live = true;
		skip -= T.skip;
	}
};

// ---------------------------------------------------------------- loudness (r8b_loudness.h)
// The meter's constants for the destination rate fs (include/r8bsrc.h "loudness"): the ten coefficients in plain fp64,
// the hand-off matrix by the recurrence itself, the sub-block's frames
inline void loudness_design(double fs, double* coef, double* phi, long long* hop)
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

// (the shelf is unstable once the rate approaches twice 1682 Hz; a sub-block must fit the kernels' int)
inline void loudness_rate_check(double rate)
{
	if (!(rate >= 8000.0 && rate <= 1e10))
		throw std::runtime_error("the loudness meter needs a destination rate of 8000 Hz or more");
}

// d: kLdStateStride doubles of state per row, then cap sums per channel.  The host knows everything but the values: m
// meter frames have run (whole segments), pending more wait in the state; slot 0 of the store is sub-block store0;
// count[c] slots of channel c are filled (one number for all channels but after a clip call, `clip`, whose store the next
// metered call empties).  fresh: the device state reads as zeros
struct LoudnessMeter
{
	bool on = false, fresh = true, clip = false;
	DevBlock<double> d;
	size_t bytes = 0;
	double rate = 0.0; // the object's destination rate (0: an object made of one stage has none)
	int nch = 0, pending = 0;
	long long cap = 0, hop = 0, m = 0, store0 = 0;
	std::vector<long long> count;
	double coef[10], phi[16];
	void enable(Engine& e, int want, long long capacity)
	{
		if (want)
		{
			loudness_rate_check(rate);
			if (capacity < 1 || capacity > (1LL << 40)) throw std::runtime_error("capacity must be at least 1 sub-block");
			if (d == nullptr || capacity != cap)
			{
				DevGuard guard(e.device());
				nch = e.channels();
				bytes = ((size_t) kLdStateStride + (size_t) capacity) * nch * sizeof(double);
				d.alloc(bytes);
				cap = capacity;
				count.assign((size_t) nch, 0);
				clip = false;
				on = false;
			}
			loudness_design(rate, coef, phi, &hop);
			// (switched on: meter frame 0 is the next call's first frame)
			if (!on) restart();
		}
		on = want != 0;
	}
	long long read(Engine& e, double* sums, long long stride, long long* counts, int drain, void* stream)
	{
		if (d == nullptr) throw std::runtime_error("the object's loudness meter was never enabled");
		long long most = 0;
		for (int c = 0; c < nch; c++) most = std::max(most, count[c]);
		if (sums != nullptr && stride < most) throw std::runtime_error("stride is smaller than the largest count");
		DevGuard guard(e.device());
		std::vector<double> v((size_t) cap * nch);
		dev_download(v.data(), d + (size_t) kLdStateStride * nch, v.size() * sizeof(double), stream); // (waits for `stream`)
		for (int c = 0; c < nch; c++)
		{
			if (counts) counts[c] = count[c];
			if (sums) memcpy(sums + c * stride, v.data() + (size_t) c * cap, (size_t) count[c] * sizeof(double));
		}
		if (drain) empty();
		return most;
	}
	// the meter starts again at meter frame 0; what the store holds stays in front of what comes
	void restart()
	{
		fresh = true;
		pending = 0;
		m = 0;
		store0 = clip || count.empty() ? 0 : -count[0];
	}
	// the store is empty from here on: slot 0 is the next sub-block to complete
	void empty()
	{
		std::fill(count.begin(), count.end(), 0);
		clip = false;
		store0 = hop > 0 ? m / hop : 0;
	}
	// store and state
	void cleared()
	{
		clip = false;
		restart();
		empty();
	}
	void history_lost() { restart(); }
	// a streaming call of frames() output frames (asked only while the meter is on): the store must take the sub-blocks
	// it completes
	template<class Frames>
	void admit(Frames frames) const
	{
		if (!on) return;
		const long long n = frames();
		const long long after = (m + pending + n) / kLdSeg * kLdSeg;
		const long long filled = after / hop - (clip ? m / hop : store0);
		if (filled > cap)
			throw std::runtime_error("the loudness store holds " + std::to_string(cap) + " sub-blocks per channel and this call "
				"would complete the " + std::to_string(filled) + "th: read with drain first");
	}
	// a clip call whose longest output has P frames: the store must take that clip's sub-blocks
	void admit_clips(long long P) const
	{
		if (!on) return;
		if (P / hop > cap)
			throw std::runtime_error("the loudness store holds " + std::to_string(cap) + " sub-blocks per channel and the longest "
				"clip has " + std::to_string(P / hop));
	}
	// state and store start empty at a clip call; what a clip of K channels will have stored is known now
	void clip_begin(int K, const long long* out_len)
	{
		if (!on) return;
		cleared();
		clip = true;
		for (int c = 0; c < nch; c++) count[c] = out_len[c / K] / hop;
	}
	void clip_end() { restart(); }
	void launch(const MeterRows& R)
	{
		if (!on) return;
		// (a streaming call behind a clip call starts from an empty store)
		const bool streaming = !R.in_clip_call();
		if (streaming && clip) empty();
		LoudnessLaunch T = R.as<LoudnessLaunch>();
		T.pending = pending;
		T.fresh = fresh ? 1 : 0;
		T.m0 = m;
		T.hop = hop;
		T.store0 = store0;
		T.capacity = cap;
		T.state = d;
		T.sums = d + (size_t) kLdStateStride * nch;
		memcpy(T.coef, coef, sizeof(coef));
		memcpy(T.phi, phi, sizeof(phi));
		launch_loudness(T, R.stream);
		const long long total = pending + R.n;
		m += total / kLdSeg * kLdSeg;
		pending = (int) (total % kLdSeg);
		fresh = false;
		// (what admit() let in: the whole sub-blocks of the stream so far, less those drained)
		if (streaming) std::fill(count.begin(), count.end(), m / hop - store0);
	}
};

} // namespace r8bhip

#endif
