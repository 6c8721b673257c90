/*
 * include/r8bsrc.h -- C ABI of libr8bsrc_hip.so, the MI355X-native batched sample-rate converter.
 *
 * Part 1 re-declares, symbol for symbol, what the reference's DLL exports
 * (reference DLL/r8bsrc.h:31-132, implemented there by DLL/r8bsrc.cpp:67-107), so that a program
 * linked against the reference's r8bsrc library links against this one unchanged.
 * Part 2 is additive: an N-channel batch object whose process() takes DEVICE (HBM) pointers --
 * this is the entry point the throughput numbers are quoted on.  Every signature uses plain
 * pointers and sizes only (no torch types, no C++ types).
 *
 * All functions are thread-compatible the same way the reference is (DLL/r8bsrc.h, README
 * "one object per stream"): distinct objects may be used from distinct threads, one object must
 * not be used concurrently.
 */
#ifndef R8BSRC_HIP_INCLUDED
#define R8BSRC_HIP_INCLUDED

#ifndef R8BSRC_DECL
	#define R8BSRC_DECL __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * Part 1: drop-in symbols (reference DLL/r8bsrc.h)
 * ------------------------------------------------------------------------------------------- */

/* reference DLL/r8bsrc.h:31 */
typedef void* CR8BResampler;

/* reference DLL/r8bsrc.h:37-43; ReqAtten 136.45 / 109.56 / 180.15 dB
 * (reference CDSPResampler.h:746,777,807 via DLL/r8bsrc.cpp:67-85). */
enum ER8BResamplerRes
{
	r8brr16 = 0,
	r8brr16IR = 1,
	r8brr24 = 2
};

/* replaces reference DLL/r8bsrc.h:68-70 (r8b_create).  Returns NULL (after printing the reason to
 * stderr) when no MI355X/HIP device is usable: there is no CPU fallback. */
R8BSRC_DECL CR8BResampler r8b_create(double SrcSampleRate, double DstSampleRate, int MaxInLen,
	double ReqTransBand, enum ER8BResamplerRes Res);

/* replaces reference DLL/r8bsrc.h:79 */
R8BSRC_DECL void r8b_delete(CR8BResampler rs);

/* replaces reference DLL/r8bsrc.h:92 (CDSPResampler::getInputRequiredForOutput,
 * CDSPResampler.h:476-484) */
R8BSRC_DECL int r8b_inlen(CR8BResampler rs, int ReqOutSamples);

/* replaces reference DLL/r8bsrc.h:102 */
R8BSRC_DECL void r8b_clear(CR8BResampler rs);

/* replaces reference DLL/r8bsrc.h:131-132.  The reference declares `double*& op0`; at ABI level
 * that is a `double**` (DLL/r8bsrc.pas:31-32 binds it as `var op0: PR8BDouble`).  `ip0` and `*op0`
 * are HOST pointers, exactly like the reference: `*op0` points into a buffer owned by the object,
 * valid until the next call on it (CDSPResampler.h:546-552); if Src == Dst, `*op0 = ip0`. */
#ifdef __cplusplus
R8BSRC_DECL int r8b_process(CR8BResampler rs, double* ip0, int l, double*& op0);
#else
R8BSRC_DECL int r8b_process(CR8BResampler rs, double* ip0, int l, double** op0);
#endif

/* ---------------------------------------------------------------------------------------------
 * Part 2: N-channel batch object (additive; no counterpart in the reference, whose callers loop
 * "for each channel: process(same length)" -- example.cpp:63-67, bench/r8bfreesrc.cpp:120-124)
 * ------------------------------------------------------------------------------------------- */

typedef void* CR8BBatch;

/* Creates `nch` independent linear-phase resamplers that share one schedule, on HIP device
 * `device` (-1 = current).  ReqAtten is the reference constructor's ReqAtten in dB
 * (CDSPResampler.h:117-120).  NULL + message in r8b_last_error() on failure.
 *
 * Channel independence and accuracy.  The output of every channel equals the reference's for that channel's samples
 * within RMS 1e-15 / peak 1e-13 OF THAT CHANNEL'S OWN LEVEL (for full-scale +-1.0 noise: the absolute figures; measured
 * RMS 2-4e-16, the reference's own noise between two of its builds), and is bitwise independent of how the stream is
 * cut into calls.  Channels 2c and 2c+1 are convolved as the real and imaginary part of one complex transform (the
 * filter kernels are real); per transform block the quieter of the two is brought to its partner's binary order of
 * magnitude by an exact power of two and taken back afterwards, so a channel at -240 dBFS beside a full-scale partner
 * keeps its error at 1e-16 of its own level, as in the reference's one-object-per-channel use (README.md:52-55).  A
 * channel whose samples are all zero comes out as exact zeros whatever its partner carries (silence is detected per
 * transform block).  An Inf / NaN stays in its own channel: per transform block, a channel whose input window holds a
 * sample with exponent field 2047 goes into the transform as +0.0, so its partner's output is bitwise what it is beside
 * an all-zero channel, and every output of that channel from that block is a quiet NaN -- stored, parked or interpolated
 * alike; the later stages carry it through their filters as the reference's do.  The decision depends on the block's
 * window alone, so NaN positions too are independent of how the stream is cut into calls and survive checkpoints (a
 * NaN's sign and payload bits are not specified: where a half-band stage combines two NaNs, either may come out).  Out
 * of scope: finite inputs so large that the transform overflows (|x| >~ 1e300; the reference overflows there too).
 * "pair_conv" = 0 (r8b_batch_set_option, before the first sample) selects the one-channel kernels (slower).
 *
 * Block lengths.  Conversions whose REFERENCE block is 32768 points (a radix-3 ratio with a transition band of
 * 0.5 ... 0.6 %: 8 507 - 13 633 taps) run on 16384-point blocks of the same filter where overlap-save does not depend
 * on the block length (ratios 3/1, 1/3, 2/3), and on the REFERENCE'S OWN 32768-point block where the convolver also
 * decimates by 2 or 4 in the spectrum (ratios 3/2, 3/4: the residue of truncating a block's spectrum, -219 dB of the
 * signal, depends on the block length -- CDSPBlockConvolver.h:329-344); all of them meet the tolerance above (until
 * round 6 the two decimating ratios ran on 16384-point blocks and met 1e-13 / 1e-10 only).  Per-call output counts,
 * latency queries and chunk invariance are the reference's in every case (tests/cases.py REBLOCK_CASES, DESIGN.md
 * section 6).  Minimum phase (r8b_batch_create_ex): see DESIGN.md section 6 -- the bound there is the reference's own
 * run-to-run noise of its cepstral designer, the kernels meet 1e-15 on the reference's taps.
 * One sample the reference leaves undefined (a ONE-tap half-band up-sampler, >= 32x up-sampling below 55 dB: the
 * stream's first odd output reads an unwritten ring slot, CDSPHBUpsampler.h:606-693) is the filter's value here.
 *
 * Stream length.  Every stream of a chain -- its input, each stage's output -- is addressed by its absolute position
 * since creation / r8b_batch_clear(), a 64-bit count on the host and in the kernels; the dither's frame number is the
 * last stage's.  Exercised: each of those streams across 2^31 and 2^32 samples while signal flows, and at 2^40 + 12345
 * input samples (45 days at 2.8224 MHz; up to 2^46 samples at the end of a 64x chain), with per-call counts equal to
 * the oracle's and samples within the tolerance above; checkpoint and clear() past 2^32; dither bit-exact across output
 * frame 2^32 (tests/test_time_axis.py, both tiers; tests/cxx_time_axis.cpp under the signed-overflow sanitizer).  No
 * limit was found; by construction the plan's closed forms hold while (samples of a stream) x (the whole-step
 * interpolator's step, at most a few hundred) stays below 2^63, i.e. beyond 2^52 samples of any stream.  Not covered:
 * chains with a non-whole-step (polynomial) interpolator and minimum-phase chains at such positions (the first keeps a
 * per-output position counter the test hook cannot fast-forward, the second has no independent reference there). */
R8BSRC_DECL CR8BBatch r8b_batch_create(double SrcSampleRate, double DstSampleRate, int MaxInLen,
	double ReqTransBand, double ReqAtten, int nch, int device);

R8BSRC_DECL void r8b_batch_delete(CR8BBatch b);
R8BSRC_DECL void r8b_batch_clear(CR8BBatch b);
R8BSRC_DECL int r8b_batch_channels(CR8BBatch b);
/* ordinal of the HIP device the object lives on (device = -1 at creation: the device that was
   current then).  Every entry point runs on that device and leaves the caller's current device as
   it found it. */
R8BSRC_DECL int r8b_batch_device(CR8BBatch b);

/* CDSPResampler::getMaxOutLen(0) for the MaxInLen given at creation (CDSPResampler.h:502-519):
 * the minimum per-channel capacity of the output buffer. */
R8BSRC_DECL int r8b_batch_max_out_len(CR8BBatch b);
/* The chain's residual fractional latency in OUTPUT samples: r8b::CDSPResampler::getLatencyFrac() (reference
 * CDSPResampler.h:491-494: the LatencyFrac the last stage reports, :688).  0.0 for linear-phase objects; for
 * fprMinPhase (r8b_batch_create_ex) what a caller that compensates latency has to add to getLatency() = 0. */
R8BSRC_DECL double r8b_batch_latency_frac(CR8BBatch b);
/* CDSPResampler::getInputRequiredForOutput / getInLenBeforeOutPos (CDSPResampler.h:476-484,406) */
R8BSRC_DECL int r8b_batch_inlen(CR8BBatch b, int ReqOutSamples);
R8BSRC_DECL int r8b_batch_inlen_before_outpos(CR8BBatch b, int OutPos);

/* One process() step for all channels.  d_in / d_out are DEVICE pointers, channel-major:
 * channel c's samples start at d_in + c*in_stride (doubles), l <= MaxInLen samples each;
 * channel c's output is written at d_out + c*out_stride (out_stride >= r8b_batch_max_out_len).
 * `stream` is a hipStream_t (NULL = default stream); the call only enqueues work on it.
 * Any 8-byte aligned rows work; rows that start on 16-byte boundaries (even strides, better multiples of 8
 * samples = 64 bytes) let the last stage store pairs of outputs as 16 bytes.  Fastest of all (optional): rows on a
 * 64-byte pitch and d_out advanced by (outputs this object has produced so far) mod 8 samples, so that output j of
 * the stream always lands at a column congruent to j mod 8 -- the fused kernels' 64-byte store pieces are then
 * whole aligned segments in every call (worth 3-4 % on 44100 -> 96000).
 * Returns the number of output samples produced per channel (identical for all channels and equal
 * to what the reference's process() returns for the same call sequence), or -1 on error. */
R8BSRC_DECL int r8b_batch_process(CR8BBatch b, const double* d_in, long long in_stride, int l,
	double* d_out, long long out_stride, void* stream);

/* Convenience: same with HOST buffers (copies through the device, synchronous). */
R8BSRC_DECL int r8b_batch_process_host(CR8BBatch b, const double* in, long long in_stride, int l,
	double* out, long long out_stride);

/* PCM boundary next to the hot path (the reference's command-line tool does
 * this on the host through CWaveFile, call sites bench/r8bfreesrc.cpp:103,134): one process()
 * step whose input and output are DEVICE buffers of PCM samples, converted by ingest / egress
 * kernels on `stream`, so that 2-4 bytes per sample cross PCIe and the HBM edge instead of 8.
 *   interleaved != 0: frame-major, sample (frame f, channel c) is element f*stride + c
 *                     (stride >= channel count; the usual WAV layout has stride == channels)
 *   interleaved == 0: planar, element c*stride + f
 * Strides are in samples.  Integer formats decode as value / 2^(bits-1) and encode as
 * round-to-nearest-even of v * 2^(bits-1), saturated -- plain by default, with TPDF dither added before the rounding
 * when r8b_batch_set_dither() asks for it (specification below); R8B_PCM_S24 is packed
 * 3-byte little-endian.  THIS CONVENTION IS THIS LIBRARY'S DEFINITION: the reference's converter (CWaveFile, from the
 * author's libvox) is not part of the reference sources, so its scale (2^(bits-1) vs 2^(bits-1) - 1), rounding and
 * dither cannot be pinned to it; the codec is bit-exact against its own specification (tests/test_pcm.py) and the fp64
 * core between the two conversions is pinned to the reference.  Returns the output frames produced, or -1 on error.
 *
 * The one-byte formats -- WAV's remaining encodings: unsigned 8-bit PCM (format tag 1 at 8 bits), A-law (tag 6) and
 * mu-law (tag 7) -- on either side of every entry of the boundary, in either layout.  Like the integer convention this
 * is this library's definition; `>>` is arithmetic, seg(m, base) is the number of k in 0 .. 7 with m > (base << k) - 1.
 *   R8B_PCM_U8    decode (b - 128) / 128.  Encode q = rint(v * 128 + d), saturated to [-128, 127], NaN -> 0, the stored
 *                 byte q + 128.  An integer format in every respect, at scale 128: TPDF dither d as specified below (the
 *                 format that needs it most), `clipped` by the integer rule, the encoded zero 0x80.
 *   R8B_PCM_ULAW  ITU-T G.711 over a 16-bit linear value, scale 32768.  Decode T[b] / 32768 with T the standard 16-bit
 *   R8B_PCM_ALAW  expansion (mu-law reaches +-32124, A-law +-32256).  Encode s = the S16 encode of v WITHOUT dither
 *                 (rint(v * 32768), saturated, NaN -> 0), then the standard compression of s.  Dither is ignored as by the
 *                 float formats (the bytes are the same with it on or off), `clipped` is the undithered S16 rule, peak
 *                 and nonfinite as ever.  Encoded zeros: 0xFF (mu-law), 0xD5 (A-law).
 *     mu-law decode  u = ~b & 255;  t = (((u & 15) << 3) + 0x84) << ((u >> 4) & 7);  value = (u & 0x80) ? 0x84 - t : t - 0x84
 *     A-law decode   a = b ^ 0x55, e = (a >> 4) & 7, m = a & 15;  t = e == 0 ? (m << 4) + 8 : ((m << 4) + 0x108) << (e - 1);
 *                    value = (a & 0x80) ? t : -t
 *     mu-law encode  p = s >> 2, neg = p < 0;  m = min(|p|, 8159) + 0x21, e = seg(m, 0x40);
 *                    u = e >= 8 ? 0x7F : (e << 4) | ((m >> (e + 1)) & 15);  byte = u ^ (neg ? 0x7F : 0xFF)
 *     A-law encode   p = s >> 3, neg = p < 0;  m = neg ? -p - 1 : p, e = seg(m, 0x20);
 *                    a = e >= 8 ? 0x7F : (e << 4) | ((e < 2 ? m >> 1 : m >> e) & 15);  byte = a ^ (neg ? 0x55 : 0xD5)
 *   These are the tables of CPython's audioop at width 2 (tests/golden/g711.npz holds all four; all 256 codes and all
 *   65536 inputs agree).  The one code that does not survive a round trip is mu-law 0x7F, the negative zero: it decodes
 *   as 0 and encodes as 0xFF.  The device computes both directions arithmetically (the segment by count-leading-zeros).
 *   Cost: the stage kernels do not know these formats (their per-sample format test would grow by two segment
 *   searches), so a side in one of them ALWAYS goes through the staging rows, planar sides included -- one extra pass
 *   over that side's fp64 rows, counted in "pcm_staged_sides" like a planar side at a compile-time-sized convolver.
 * Every value that names none of the eight formats is refused ("unknown PCM sample format"), and r8b_pcm_sample_bytes
 * returns 0 for it. */
enum r8b_pcm_format
{
	R8B_PCM_F64 = 0,
	R8B_PCM_F32 = 1,
	R8B_PCM_S16 = 2,
	R8B_PCM_S24 = 3,
	R8B_PCM_S32 = 4,
	R8B_PCM_U8 = 16,
	R8B_PCM_ULAW = 17,
	R8B_PCM_ALAW = 18
};
R8BSRC_DECL int r8b_batch_process_pcm(CR8BBatch b, const void* d_in, int in_format,
	int in_interleaved, long long in_stride, int l, void* d_out, int out_format,
	int out_interleaved, long long out_stride, void* stream);
R8BSRC_DECL int r8b_pcm_sample_bytes(int format);

/* TPDF dither of the integer formats U8 / S16 / S24 / S32 (F32 / F64 / ULAW / ALAW outputs ignore it and stay
 * byte-identical; U8: scale = 128).  The
 * dither of a sample is a pure function of (seed, channel, absolute output frame) -- no generator runs from sample to
 * sample -- so the output stays bitwise independent of how the stream is cut into calls, survives checkpoints, and
 * shards of a batch reproduce the whole.  With scale = 2^(bits-1) and all integer arithmetic in 64-bit unsigned
 * words with wrap-around:
 *   mix(z):  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 *   k   = mix(seed ^ ((first_channel + c) * 0xD1B54A32D192ED03))
 *   z   = mix(k + j * 0x9E3779B97F4A7C15)
 *   d   = (double(z >> 32) - double(z & 0xFFFFFFFF)) * 2^-32          triangular in (-1, 1) LSB, exact in fp64
 *   q   = rint(v * scale + d), saturated to [-scale, scale - 1]; NaN -> 0
 * c is the channel's index in this object, j the absolute output frame of the stream since creation or
 * r8b_batch_clear(): the last stage's count of outputs emitted, which the checkpoint blob already carries (blob
 * format, r8b_batch_state_size() and the configuration check do not change; load the blob into an object with the
 * same r8b_batch_set_dither() settings).  A pass-through object (Src == Dst, no stages) counts its frames in the
 * handle itself: r8b_batch_clear() resets that count and a blob does NOT carry it.  Silence stays silent in fp64 (zero
 * input gives exact zeros), so a dithered silent stream is rint(d).  Noise shaping and output gain are not offered.
 *   mode 0 = none (default), 1 = TPDF as specified; first_channel = number of this object's channel 0 in the
 *   dither key (a shard of a larger batch passes its offset; 0 otherwise).  May change between calls.
 * Returns 0, or -1 (unknown mode, negative first_channel; r8b_last_error()). */
enum r8b_dither_mode
{
	R8B_DITHER_NONE = 0,
	R8B_DITHER_TPDF = 1
};
R8BSRC_DECL int r8b_batch_set_dither(CR8BBatch b, int mode, unsigned long long seed, int first_channel);

/* Per-channel meters of the r8b_batch_process_pcm egress, accumulated over calls until read with reset:
 *   peak       max |v| of the fp64 output value before dither; NaN skipped, +Inf allowed
 *   clipped    integer formats: samples whose rounded (dithered) value fell outside [-scale, scale - 1] before
 *              saturation (ULAW / ALAW: of the undithered 16-bit value); float formats: samples with |v| > 1.0
 *   nonfinite  samples whose exponent field is 2047 (Inf or NaN)
 * Meters are instrumentation, not stream state: r8b_batch_clear() zeroes them (on the default stream: like the rest
 * of r8b_batch_clear() it expects the stream the process calls were enqueued on to be idle -- a finishing kernel still
 * in flight on a non-blocking stream would add to the meters after they were zeroed), checkpoints do not carry them, and
 * enabling allocates three device arrays of one entry per channel (kept, and the counts with them, while disabled).
 * While dither or meters are on, the output side of every call goes through the staging rows and the finishing egress
 * kernels, also a planar side the last stage would otherwise encode itself (counted in "pcm_staged_sides").
 * r8b_batch_meter_read waits for `stream`; any of the three arrays (channel-count entries each) may be NULL;
 * reset != 0 zeroes the meters after reading.  -1 when the object's meters were never enabled. */
R8BSRC_DECL int r8b_batch_meter_enable(CR8BBatch b, int on);
R8BSRC_DECL int r8b_batch_meter_read(CR8BBatch b, double* peak, long long* clipped, long long* nonfinite, int reset,
	void* stream);

/* True peak: the per-channel maximum of the 4x interpolated output, the quantity delivery specifications limit (EBU
 * R 128, ATSC A/85, -1 dBTP).  Band-limiting rings: a stream whose samples all stay below full scale can reconstruct
 * above it, and `peak` above does not see that.  The library's own definition, bit for bit:
 *   x[j]  the fp64 output value of frame j of a channel before dither and encoding -- the value `peak` sees; frames
 *         before the start of the stream are +0.0.
 *   g     48 taps, four phases of 12: g[i] = sinc((i - 24) / 4) * I0(8 sqrt(1 - ((i - 24) / 24)^2)) / I0(8), i = 0 .. 47,
 *         a Kaiser-windowed Nyquist filter, exactly symmetric.  tools/gen_true_peak.py computes it; the literals it
 *         wrote into csrc/r8b_truepeak.h (the same bits: tests/golden/true_peak_taps.json) ARE the definition, as the
 *         G.711 tables are.  All 36 coefficients of the phases 1 .. 3 are non-zero, the smallest is 2.6e-4.
 *   y     phase 0 is no filter: y[4 j] = x[j - 6] exactly (the prototype's residues of 1e-17 there are dropped), so
 *         +-Inf passes as itself.  For p = 1, 2, 3: acc = g[p] * x[j] (one multiplication), then
 *         acc = fma(g[4 t + p], x[j - t], acc) for t = 1 .. 11 in that order; y[4 j + p] = acc.
 *   meter max |y| over the y covered so far, NaN results skipped, +Inf allowed; kept as the bit pattern of a
 *         non-negative double like `peak`, 0.0 at first.  A maximum does not depend on the order: the value is bitwise
 *         determined by the stream.
 * r8b_batch_process_pcm: after N output frames the meter has covered y[0 .. 4 N).  The interpolator is causal, so the
 *   meter LAGS the stream by 6 frames: the last 6 frames of a stream enter through phase 0 only after 6 more frames.
 *   11 frames per channel are carried from call to call, so the value is bitwise independent of how the stream is cut
 *   into calls.  r8b_batch_clear() zeroes value and history (on the default stream, under the meters' idle-stream
 *   condition above); reading with reset zeroes the value only.  Checkpoints do not carry the meter (blob format,
 *   r8b_batch_state_size() and the configuration check are unchanged): r8b_batch_state_load() drops the history, and the
 *   next 11 frames only refill it -- their y are not metered, because a zeroed history in mid-stream would be a step, and a
 *   step over-reads by the interpolator's overshoot.  Enabling the meter on a stream that has taken samples does the same.
 * r8b_batch_resample_clips* (all five): the history is zero at the start of the call; a clip's x is its output frames
 *   [0, out_len) followed by zeros, and the meter covers the WHOLE convolution, frames j in [0, out_len + 11) -- the tail
 *   comes out without another step, so for clip calls true_peak >= peak holds bitwise.  An out_len that cuts a clip short
 *   is metered as delivered, its edge included.  The value is kept by the clip's own object channel in the caller's
 *   numbering, whatever slot it rode in; rows of dropped or finished clips add nothing; the call does not zero the
 *   value (as with the meters).
 * Src == Dst objects are metered the same way.  r8b_batch_process / _host are not metered.
 * Accuracy (tools/gen_true_peak.py prints the figures): stationary tones up to 0.45 fs over-read by at most 0.002 dB;
 *   the under-read is that of any 4x grid, at most 0.44 dB at 0.4 fs -- the size of BS.1770's own 4x interpolator.
 * r8b_batch_true_peak_enable: on != 0 allocates the device arrays, zeroed -- one value and two histories of 12 doubles
 *   per channel (two: a launch writes the one its successor reads while its own is still being read) -- and keeps them,
 *   and the value with them, while disabled.  Independent of r8b_batch_meter_enable.  While it is on, the output side of
 *   every PCM call goes through the staging rows, also a planar side the last stage would otherwise encode itself
 *   (counted in "pcm_staged_sides"), and a kernel of its own (k_truepeak) runs beside the egress kernel, which stays the
 *   one it was: the finishing kernels still run only for dither or meters.  While it is off nothing differs.
 * r8b_batch_true_peak_read waits for `stream` and fills channels() doubles, linear amplitudes like `peak` (NULL: reads
 *   nothing); reset != 0 zeroes the values after reading.  -1 when the meter was never enabled. */
R8BSRC_DECL int r8b_batch_true_peak_enable(CR8BBatch b, int on);
R8BSRC_DECL int r8b_batch_true_peak_read(CR8BBatch b, double* true_peak, int reset, void* stream);

/* Loudness: the K-weighted energy of every channel per 100 ms sub-block, the quantity ITU-R BS.1770 builds programme
 * loudness (LUFS; EBU R 128, ATSC A/85) from, and a host function that gates and integrates it.  K-weighting is two
 * biquads, a recurrence; it is DEFINED here in segments of 64 frames with a linear hand-off between them, so that the
 * segments run side by side and the sums are still bitwise determined by the stream and bitwise independent of how the
 * stream is cut into calls.  (A segmented run's sub-block energies differ from an 80-bit reference by 2e-14 relative, a
 * plain sample-by-sample fp64 recurrence by 4e-15.)  The library's own definition, bit for bit:
 *   x[m]   the fp64 output value of a channel before dither and encoding -- the value `peak` and the true-peak meter see.
 *          A sample whose exponent field is 2047 (Inf, NaN) enters as +0.0: `nonfinite` reports it, and one NaN would
 *          poison a recurrence for ever.  m is the METER frame: 0 at enable, at r8b_batch_clear(), at
 *          r8b_batch_state_load() and at the start of every clip call -- not the stream's absolute position.
 *   coefficients for the destination rate fs, computed on the host in plain fp64 with tan and pow (the re-derivation of
 *          the BS.1770-4 48 kHz tables that libebur128 made common):
 *          shelf      f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196; K = tan(pi f0 / fs),
 *                     Vh = 10^(G/20), Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2;
 *                     b = ((Vh + Vb K/Q + K^2)/a0, 2 (K^2 - Vh)/a0, (Vh - Vb K/Q + K^2)/a0),
 *                     a1 = 2 (K^2 - 1)/a0, a2 = (1 - K/Q + K^2)/a0;
 *          high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773, K and a0 alike; b = (1, -2, 1), a1, a2 alike.
 *          At 48000 Hz: shelf b 1.5351248595869702, -2.6916961894063807, 1.19839281085285, a -1.6906592931824103,
 *          0.7324807742158501; high-pass a -1.9900474548339797, 0.9900722503662099 -- the standard's table.  The shelf is
 *          unstable once fs approaches twice 1682 Hz: a rate below 8000 is refused.
 *   stage  with state (p, q):  y = fma(b0, x, p);  p' = fma(-a1, y, fma(b1, x, q));  q' = fma(-a2, y, b2 * x).
 *          A frame is the shelf on x, then the high-pass on the shelf's y; its result is z.  A channel's state is
 *          S = (p1, q1, p2, q2); R(S, x[0 .. n)) names the z and the final state of that run.
 *   segments  of M = 64 meter frames.  S_0 = 0.  The z of segment k are those of R(S_k, segment) (that run's final state
 *          is dropped); Z_k is the final state of R(0, segment); the hand-off, for each component i:
 *          S_{k+1}[i] = fma(Phi[i][3], S_k[3], fma(Phi[i][2], S_k[2], fma(Phi[i][1], S_k[1], fma(Phi[i][0], S_k[0], Z_k[i])))).
 *          Column j of Phi is the final state of R(e_j, 64 zeros): computed by the recurrence itself, so its bits are
 *          defined.  (The entries that couple the high-pass's state into the shelf's are exactly 0; all sixteen products
 *          are formed.)
 *   energies  H = (long long)(fs / 10 + 0.5) frames is the sub-block.  For each segment and each sub-block it overlaps
 *          (at most two: H >= 800 > M) the piece is e = 0.0, then e = fma(z, z, e) over the segment's frames inside that
 *          sub-block, in frame order.  A sub-block's sum starts at 0.0 and takes its pieces in ascending order by plain
 *          additions; it is stored once the piece that holds its last frame is in.  What is stored is the SUM, not the
 *          mean.
 * r8b_batch_process_pcm: only whole segments run; up to 63 pending frames per channel are carried to the next call with S
 *   and the open sum, so the stored sums are bitwise independent of how the stream is cut, and the meter lags the
 *   stream by fewer than 64 frames.  All channels have the same number of completed sub-blocks, and the host knows it
 *   without asking the device.
 * r8b_batch_resample_clips* (all five): state and store start empty at the call; a clip's x is its delivered frames
 *   [0, out_len[c]); the step that holds a clip's last frame finishes it -- its last segment is filled with zeros and
 *   run --, and floor(out_len[c] / H) sub-blocks are stored for the clip's own object channel in the caller's numbering,
 *   whatever slot it rode in; rows of dropped or finished clips add nothing.  A clip call's store stays readable until
 *   the next metered call, which empties it.
 * Capacity: the store holds `capacity` sub-blocks per channel.  A call that would complete more than fit is refused
 *   before anything is enqueued: -1, r8b_last_error(), nothing changed.  Reading with drain != 0 empties the store.
 * Lifecycle, as the true-peak meter's: independent of the other meters; the arrays are kept while disabled (enabling
 *   with another capacity allocates anew, empty); r8b_batch_clear() empties the store and restarts the meter,
 *   r8b_batch_state_load() and enabling a disabled meter restart it and keep the store (new sub-blocks go behind the
 *   kept ones); blobs and r8b_batch_state_size() are unchanged.  While it is on, the output side of every PCM call goes
 *   through the staging rows (counted in "pcm_staged_sides") and a kernel of its own (k_loudness) runs beside the egress
 *   kernel; while it is off nothing differs.  r8b_batch_process / _host are not metered.
 * r8b_loudness_design (host only): the constants for `rate` -- coefs: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2;
 *   handoff: Phi[i][j] at handoff[4 i + j]; hop: H.  Any pointer may be NULL.  -1 for a rate below 8000.
 * r8b_batch_loudness_enable: on != 0 allocates (capacity >= 1 sub-blocks per channel; 600 is a minute) and switches on;
 *   -1 with a message when the object's destination rate is below 8000 (or unknown: r8b_batch_create_stage).
 * r8b_batch_loudness_read waits for `stream`, fills counts[c] and sums[c * stride + i], i < counts[c] (either may be
 *   NULL; stride >= the largest count); returns the largest count, -1 when the meter was never enabled.
 * r8b_loudness_integrated (host only): programmes are runs of Kp consecutive channels with weights w (NULL: all 1.0;
 *   BS.1770 gives the surround channels 1.41).  A gating block is 4 consecutive sub-blocks, hopped by one:
 *   G_j = sum_i w_i (s_i[j] + .. + s_i[j+3]) / (4 hop), l_j = -0.691 + 10 log10 G_j.  Absolute gate l_j > -70; relative
 *   gate 10 LU below the loudness of the mean of the absolutely gated G_j; lufs[p] = -0.691 + 10 log10 of the mean G_j
 *   that pass both, -HUGE_VAL if none does.  A programme's block count is the smallest of its channels' counts.
 * Momentary (4 sub-blocks) and short-term (30) loudness are plain sums over the same array and are left to the caller.
 * Loudness range, output gain and noise shaping are out of scope. */
R8BSRC_DECL int r8b_loudness_design(double rate, double* coefs, double* handoff, long long* hop);
R8BSRC_DECL int r8b_batch_loudness_enable(CR8BBatch b, int on, long long capacity);
R8BSRC_DECL long long r8b_batch_loudness_read(CR8BBatch b, double* sums, long long stride, long long* counts, int drain,
	void* stream);
R8BSRC_DECL int r8b_loudness_integrated(const double* sums, long long stride, const long long* counts, int nprog, int Kp,
	const double* weights, long long hop, double* lufs);

/* A batch of clips of unequal length in one call: clip c goes through channel c of the object.  What a host does
 * around r8b_batch_process_pcm today -- pad every clip to the longest, loop MaxInLen frames at a time and keep
 * feeding zeros until the last output has come out (the reference's oneshot(), CDSPResampler.h:592-651; its tool,
 * bench/r8bfreesrc.cpp:92-136), cut every row back to its length -- happens here, on device buffers.
 *
 * r8b_clip_out_len: the frames a clip of in_len frames yields, (long long) (in_len * Dst / Src) in double arithmetic,
 * the reference tool's rule (bench/r8bfreesrc.cpp:92).  Host only.
 *
 * r8b_batch_resample_clips: d_in / d_out are DEVICE buffers, planar: clip c is row c, frame j at element c*stride + j,
 * in any r8b_pcm_format.  in_len / out_len are HOST arrays of channels() entries, each >= 0; they may be freed or
 * changed as soon as the call returns.  Row c of the output receives frames [0, out_len[c]) of the stream "clip c
 * followed by zeros" -- an out_len below r8b_clip_out_len cuts the clip short, one above it takes the filter's tail
 * and then zeros -- and encoded zeros in [out_len[c], P), P = max(out_len).  Nothing at or beyond P is written; frames
 * of d_in at or beyond in_len[c] are never read, whatever they hold.  Requires in_stride >= max(in_len) and
 * out_stride >= P.  Returns P, or -1 (r8b_last_error()).
 *   - The object must be fresh: no samples processed since creation or r8b_batch_clear(); otherwise -1, and nothing
 *     has changed.  On return its stream state is that of r8b_batch_clear() again, so calls may follow one another;
 *     the meters alone are not zeroed (the kernels may still be in flight; r8b_batch_meter_read afterwards reads this
 *     call's clips).
 *   - Everything is enqueued on `stream`: steps of MaxInLen frames until P outputs exist, each an ingest kernel (while
 *     some clip still has frames; afterwards the staging rows are zeroed once), the stages, an egress kernel cut at P.
 *     The call does not wait for `stream`.
 *   - Dither and meters apply as in r8b_batch_process_pcm: a frame's dither index j is its frame number in the clip;
 *     the meters see frames j < out_len[c] only; the padding zeros are neither dithered nor counted.
 *   - Src == Dst (no stages): converts and masks -- min(in_len[c], out_len[c]) frames copied, zeros up to out_len[c]
 *     (dithered like any silence), encoded zeros up to P.
 *   - P == 0 returns 0 and launches nothing; in_len[c] == 0 is a silent row.
 * The lengths on the device: a call's kernels read them after the call has returned, so one device array that the
 * next call overwrites would not do, and a synchronous upload on the null stream does not order against a
 * non-blocking `stream` either.  The object keeps FOUR device arrays and takes them in turn; a call copies its
 * lengths into a host block of the slot, uploads that block asynchronously ON `stream` in front of its kernels, and
 * records an event on `stream` behind its last launch.  A slot is taken again only after its event has passed: calls
 * enqueued back to back on one stream, with different lengths and no synchronisation between them, are each right,
 * and the only wait there ever is is the fifth call's for the first while four are still in flight.  (Like every
 * other entry of an object, the calls belong on ONE stream: the stream state is not ordered across streams.)
 * Cost: both sides ALWAYS go through the object's staging rows -- an F64 -> F64 batch pays two passes over the data
 * that r8b_batch_process on the caller's rows does not; any other format in front of / behind a compile-time-sized
 * convolver pays what r8b_batch_process_pcm already pays there (its "pcm_staged_sides"), the masked kernels replacing
 * the plain staging kernels one for one.  Every clip rides to the end of the longest one: a batch of similar
 * lengths wastes little, one long clip among short ones makes the short ones resample silence.
 *
 * r8b_batch_resample_clips_ex: the same call for clips of clip_channels = K channels each, 1 <= K <= 64, channels() a
 * multiple of K: clip i goes through channels i K .. i K + K - 1 of the object, in_len / out_len hold channels() / K
 * entries, one per clip.  Each side chooses its layout:
 *   interleaved (WAV layout; a decoder's buffer): clip i is frame-major, sample (frame f, channel k) at element
 *     i*stride + f*K + k; strides in samples; requires in_stride >= max(in_len)*K / out_stride >= P*K.  A clip's base
 *     needs its sample's own alignment only (F64: 8 bytes), so odd strides are fine.
 *   planar: the layout above, channel k of clip i being row i K + k at element (i K + k)*stride + f.
 * Interleaved S16 in and planar F32 out is the data-loader case.  Everything else is r8b_batch_resample_clips, which
 * is this call with K = 1 and planar sides: the dither key of a sample is (seed, first_channel + i K + k, frame in the
 * clip), the meters are per object channel and see frames below out_len[i] only, clip i's padding is encoded zeros in
 * elements [out_len[i]*K, P*K) of its region, nothing at or past element P*K of a region is written and no sample of
 * a frame >= in_len[i] is read.  -1 (nothing changed) also for K < 1, K > 64, K not dividing channels() and a stride
 * too small for its layout.  An interleaved side goes through tile kernels of its own (a tile of a clip's consecutive
 * samples through LDS: csrc/r8b_clip_frames.h), a planar side through the masked row kernels.
 * Not offered: reading F64 rows in place; K > 64;
 * helpers for sharded batches (a shard is an object: give it its rows and lengths).
 *
 * r8b_batch_resample_clips_mix: r8b_batch_resample_clips_ex with a channel mix in its ingest -- "decode, mix stereo (or
 * 5.1) down to mono, resample" in one call.  A mix is linear, so in front of the resampler it gives the audio a mix
 * behind it gives, and the stages run on K instead of Kin channels per clip; the ingest kernel, which passes every
 * sample anyway, does it without another pass over memory (csrc/r8b_clip_mix.h).  Everything not stated here is _ex:
 * the fresh-object rule and the state afterwards, P and the padding, dither keys, meters (per OBJECT channel), the
 * four slots, "enqueues only", Src == Dst, and the whole output side.
 *   clip_channels = K, 1 <= K <= 64, dividing channels(): clip i goes through object channels i K .. i K + K - 1.
 *   in_channels = Kin, 1 <= Kin <= 64: the channels of a clip in the caller's INPUT buffer.
 *   mix: HOST array of K x Kin doubles, row-major: mix[m*Kin + k] is the gain of input channel k in object channel m
 *     of every clip.  Every entry finite.  It may be freed or changed as soon as the call returns.
 *   input, interleaved: sample (frame f, channel k) of clip i at element i*in_stride + f*Kin + k; requires
 *     in_stride >= max(in_len)*Kin (Kin == 1: a row).  Planar: channel k of clip i is row i Kin + k, at element
 *     (i*Kin + k)*in_stride + f; requires in_stride >= max(in_len).  No sample of a frame >= in_len[i] is read.
 * The sample that enters object channel m at frame f is defined bit for bit: over the k with mix[m*Kin + k] != 0.0,
 * in ascending order, acc = mix[k0] * x[k0] (one fp64 multiply), then acc = fma(mix[k], x[k], acc) for each further
 * k, x[k] the decoded sample of input channel k.  A coefficient of +-0.0 contributes NOTHING: a row [1 0] selects
 * channel 0, bitwise the sample, whatever channel 1 holds (Inf and NaN included); a row of zeros gives +0.0 and that
 * object channel comes out as exact silence.  The identity matrix with Kin == K is _ex.
 * -1 (nothing changed; the message names the argument) for in_channels outside 1 .. 64, mix == NULL, a coefficient
 * that is not finite, an in_stride too small for Kin and its layout, and everything _ex refuses.
 * The matrix on the device: up to 32 KB, so it does not travel in the kernel arguments.  Each of the four slots owns a
 * device block for it, allocated or enlarged when the slot is taken (that is, behind its event), filled through a
 * host block of the slot and uploaded asynchronously on `stream` in front of the call's kernels, as the lengths are:
 * calls enqueued back to back with different matrices and no synchronisation each read their own.
 * Not offered: a mix on the OUTPUT side; a matrix per clip; Kin or K above 64.
 *
 * r8b_batch_resample_clips_packed: r8b_batch_resample_clips_mix / _ex for clips PACKED END TO END -- one buffer and an
 * offsets array, as a loader holds its decoded clips (torch jagged layouts, cu_seqlens) and as a consumer of packed
 * sequences wants them back.  The calls above address clip i at i*stride, so every clip takes the room of the longest
 * one in the pinned buffer, over PCIe and in HBM, and the egress stores zeros up to P that such a consumer throws away;
 * packed, a batch costs the sum of its lengths and nothing is read or written outside a clip's own region.  The
 * resampler between the two sides is the same; the ingest and egress kernels are the strided ones with another
 * addressing rule (csrc/r8b_clip_packed.h), so a clip's samples are the strided call's bit for bit.
 *   in_offset / out_offset: HOST arrays of channels() / K entries, one per clip, each >= 0: where the clip's region
 *     starts, in samples of that side's format counted from d_in / d_out.  They may be freed or changed as soon as the
 *     call returns.
 *   in_offset == NULL / out_offset == NULL: that side is strided exactly as in _mix / _ex, and its stride and the
 *     check on it apply.  With both NULL the call IS _mix (_ex when mix == NULL): the same code path, kernels and bytes.
 *   offset array given: that side is packed and its stride is ignored.  Clip i with Kc channels (Kc = in_channels on
 *     an input side with a mix, else clip_channels) and n = in_len[i] / out_len[i] frames occupies the n*Kc elements
 *     from offset[i]:
 *       interleaved: sample (frame f, channel k) at element offset[i] + f*Kc + k;
 *       planar: at element offset[i] + k*n + f -- the clip's channels one behind the other at the clip's OWN length,
 *         as a [Kc, n] tensor lies in memory.
 *     A base needs its sample's own alignment only: any element offset, odd ones for S16 and any multiple of 3 bytes
 *     for S24 included (F64: d_in / d_out 8-byte aligned, as ever).
 *   mix == NULL: no mix; in_channels must then be 0 or equal to clip_channels.  Otherwise as in _mix.
 *   output side, packed: elements [out_offset[i], out_offset[i] + out_len[i]*K) are written, for every clip, and
 *     nothing else -- no padding anywhere.  The return value is still P = max(out_len).
 *   input side, packed: no sample outside a clip's in_len[i]*Kc elements is read.  Input regions MAY overlap or
 *     coincide (windows of one recording; one clip resampled into several rows).  A clip of length 0 has a region of
 *     no elements, and its offset is not looked at beyond >= 0.
 * Everything else is _ex / _mix: the fresh-object rule and the state afterwards, the dither key (seed, first_channel +
 * i K + k, frame in the clip), meters per object channel over frames < out_len[i], "enqueues only", Src == Dst, and
 * P == 0 returns 0 and launches nothing.
 * -1 (nothing changed, nothing launched; the message names the argument) for everything _mix / _ex refuse on the
 * sides they apply to, a negative offset, two packed OUTPUT regions of non-zero size that overlap (the regions are
 * sorted on the host: at most 65535 clips), and mix == NULL with in_channels neither 0 nor clip_channels.
 * The bases on the device travel as the lengths and the matrix do: a host block and a device block of the call's slot,
 * enlarged only when the slot is taken (behind its event), uploaded asynchronously on `stream` in front of the call's
 * kernels -- one base per ROW of a planar side (offset[i] + k*len[i], worked out on the host), one per clip of an
 * interleaved side, so that a kernel does one uniform load and no multiply by a per-clip length.  Calls enqueued back to
 * back with different offsets and no synchronisation each read their own.
 * Cost against the strided call: see profiles/clip_packed_ab.txt.
 *
 * r8b_clip_pack_offsets: host only.  offset[i] = the exclusive running sum of len[j]*channels, each clip's base rounded
 * up to a multiple of `align` elements when align > 1 (align = 1: clips end to end).  Returns the elements the buffer
 * needs -- the end of the last clip --, or -1 for nclips < 0, a negative length, channels < 1 or align < 1.
 * Still not offered: torch nested tensors as such (pass their buffer and offsets); a matrix per clip.
 *
 * r8b_batch_resample_clips_sched: r8b_batch_resample_clips_packed with `flags` (enum r8b_clip_flags) that let a batch of
 * unequal clips pay for the sum of its lengths in the STAGES too, not only in its buffers: by default every clip rides
 * through every step, to the end of the longest one.
 *   flags == 0 IS _packed: the same code path, kernels and bytes.  A bit other than the two below: -1, nothing changed,
 *     nothing launched.
 *   R8B_CLIPS_LONGEST_FIRST: clip order[g] rides in slot g, i.e. in object channels g K .. g K + K - 1, where order[] is
 *     the clips sorted by out_len descending, equal lengths by ascending index (a stable sort); without the flag the
 *     identity.  r8b_clip_schedule (host only) writes exactly this order into order[nclips] and returns 0, or -1 for
 *     nclips < 0, a negative length, a NULL array or an unknown flag bit.  Buffers, lengths and offsets stay in the
 *     CALLER's order on both sides: the call permutes what its kernels read (csrc/r8b_clip_sched.h).
 *   R8B_CLIPS_DROP_FINISHED: with `done` the outputs produced before a step (0 before the first), slot g is live while
 *     out_len[order[g]] > done; hi = 1 + the largest live g; A = hi*K, and if A is odd and hi < nclips, A += K (whole
 *     clips and whole channel pairs).  The step's ingest and stages run channels [0, A) only.  A never grows within a
 *     call.  The kernel forms stay those chosen for the OBJECT (its channel count, or "form_channels"), not for A.
 *     Dropping is per step of MaxInLen frames: a clip leaves with the step in which its last output comes out, so a
 *     small MaxInLen drops finer and launches more.  Without LONGEST_FIRST a long clip at the END of the batch keeps
 *     every slot in front of it running: the two flags belong together unless the caller has sorted already.
 * What is promised:
 *   DROP_FINISHED alone: every output byte and every meter is that of the flags == 0 call -- both layouts, both
 *     addressings, padding, mix, dither, Src == Dst.  A finished channel's rings and park buffers are simply not
 *     advanced, and nothing reads them before the call's closing clear().
 *   LONGEST_FIRST, with or without DROP_FINISHED: clip i's samples are those of the plain call on a fresh object that is
 *     GIVEN the clips in the order order[].  Clip i then shares its pair transform with another partner than in the
 *     unsorted call, so its samples are not bitwise the unsorted call's: they agree with it as any two channel
 *     placements do, within the per-channel accuracy stated at the top of this header.
 *   The dither key and the meters stay by the clip's OWN object channel i K + k in the caller's numbering, whatever slot
 *     the clip rode in: r8b_batch_meter_read is in the caller's order.
 *   A Src == Dst object has no pair transform: with any flags its bytes and meters equal the flags == 0 call's.
 *   Output padding on a strided side is unchanged: encoded zeros up to P in every row, dropped rows included.
 *   Everything else is _packed: the fresh-object rule and the state afterwards, the four slots (the rows' channels travel
 *     behind the bases in the slot's one upload), "enqueues only", and every refusal.
 * Counters (r8b_batch_stat): "clip_steps" -- process steps made by the clip calls, flagged or not; "clip_channel_steps"
 * -- the sum of A over those steps (A = channels() without DROP_FINISHED).  clip_channel_steps / (clip_steps *
 * channels()) is the share of stage work a call had left.  Measured cost: profiles/clip_sched_ab.txt.
 * Not offered: the flags on by default; dropping clips that are not a prefix of the slots; a ratio per clip. */
enum r8b_clip_flags { R8B_CLIPS_DROP_FINISHED = 1, R8B_CLIPS_LONGEST_FIRST = 2 };
R8BSRC_DECL long long r8b_clip_out_len(double SrcSampleRate, double DstSampleRate, long long in_len);
R8BSRC_DECL long long r8b_batch_resample_clips(CR8BBatch b, const void* d_in, int in_format, long long in_stride,
	const long long* in_len, void* d_out, int out_format, long long out_stride, const long long* out_len, void* stream);
R8BSRC_DECL long long r8b_batch_resample_clips_ex(CR8BBatch b, int clip_channels,
	const void* d_in, int in_format, int in_interleaved, long long in_stride, const long long* in_len,
	void* d_out, int out_format, int out_interleaved, long long out_stride, const long long* out_len, void* stream);
R8BSRC_DECL long long r8b_batch_resample_clips_mix(CR8BBatch b, int in_channels, int clip_channels, const double* mix,
	const void* d_in, int in_format, int in_interleaved, long long in_stride, const long long* in_len,
	void* d_out, int out_format, int out_interleaved, long long out_stride, const long long* out_len, void* stream);
R8BSRC_DECL long long r8b_batch_resample_clips_packed(CR8BBatch b, int in_channels, int clip_channels, const double* mix,
	const void* d_in, int in_format, int in_interleaved, long long in_stride,
	const long long* in_offset, const long long* in_len,
	void* d_out, int out_format, int out_interleaved, long long out_stride,
	const long long* out_offset, const long long* out_len, void* stream);
R8BSRC_DECL long long r8b_clip_pack_offsets(int nclips, const long long* len, int channels, int align, long long* offset);
R8BSRC_DECL long long r8b_batch_resample_clips_sched(CR8BBatch b, int in_channels, int clip_channels, const double* mix,
	const void* d_in, int in_format, int in_interleaved, long long in_stride,
	const long long* in_offset, const long long* in_len,
	void* d_out, int out_format, int out_interleaved, long long out_stride,
	const long long* out_offset, const long long* out_len, int flags, void* stream);
R8BSRC_DECL int r8b_clip_schedule(int nclips, const long long* out_len, int flags, int* order);

/* Checkpoint / resume of the streaming state of all channels (the reference
 * keeps this state inside each CDSPProcessor and offers only clear()).  The blob is host memory:
 * the schedule's counters plus every history ring and the park buffer (outputs a call's last block
 * has computed for the next call).  r8b_batch_state_size() is a constant of the object; save returns
 * the bytes written; load accepts only a blob saved by an object created with the same parameters and
 * options (checked as a whole before anything changes), after which the stream continues
 * bit-identically.  Blobs are not canonical: ring and buffer positions that no later call reads keep
 * whatever earlier calls left there, so two blobs of the same stream position taken after different ways
 * of cutting the stream into calls may differ in bytes (never in the stream that follows).  Both wait
 * for `stream` (the stream the process calls were enqueued on).  Return -1 on error. */
R8BSRC_DECL long long r8b_batch_state_size(CR8BBatch b);
R8BSRC_DECL long long r8b_batch_state_save(CR8BBatch b, void* buf, long long cap, void* stream);
R8BSRC_DECL int r8b_batch_state_load(CR8BBatch b, const void* buf, long long size, void* stream);

/* The same with the phase response of the low-pass filters selectable (reference CDSPResampler.h:117-120,
 * EDSPFilterPhaseResponse CDSPFIRFilter.h:28-45): ReqPhase 0 = fprLinearPhase, 1 = fprMinPhase.  A
 * minimum-phase chain carries fractional latencies from stage to stage like the reference does; its convolvers
 * run on the pair kernel with a complex kernel spectrum, the interpolator behind them unfused.  Samples agree
 * with the reference's to 1e-15 when both use the same taps (tests feed the reference's through
 * r8b_design_set_lp_provider of a test build); with the taps of THIS library's designer the streams differ by 3e-7 ... 6e-5 RMS
 * (-48 dB for 1/3-band filters at 180 dB), because the cepstral transform's result depends on the rounding noise
 * of the FFT that computes it. */
R8BSRC_DECL CR8BBatch r8b_batch_create_ex(double SrcSampleRate, double DstSampleRate, int MaxInLen,
	double ReqTransBand, double ReqAtten, int ReqPhase, int nch, int device);

/* Single DSP stage as a batch object (the reference's CDSPProcessor boundary,
 * CDSPProcessor.h:64-127), used by the stage-level parity tests:
 *   kind 0: CDSPBlockConvolver(getLPFilter(a=ReqNormFreq, b=ReqTransBand, c=ReqAtten, linear,
 *           d=ReqGain), i0=UpFactor, i1=DownFactor)           (CDSPBlockConvolver.h:62)
 *   kind 1: CDSPFracInterpolator(a=SrcRate, b=DstRate, c=ReqAtten, i0=IsThird)
 *                                                              (CDSPFracInterpolator.h:713)
 *   kind 2: CDSPHBUpsampler(a=ReqAtten, i0=SteepIndex, i1=IsThird)   (CDSPHBUpsampler.h:572)
 *   kind 3: CDSPHBDownsampler(a=ReqAtten, i0=SteepIndex, i1=IsThird) (CDSPHBDownsampler.h:47) */
R8BSRC_DECL CR8BBatch r8b_batch_create_stage(int kind, double a, double b, double c, double d,
	int i0, int i1, int MaxInLen, int nch, int device);

/* Number of stages and a printable description of the chain (what the reference prints through
 * R8BCONSOLE, r8bconf.h:31-42).  Returns the full length; writes at most cap-1 chars. */
R8BSRC_DECL int r8b_batch_describe(CR8BBatch b, char* buf, int cap);

/* Kernel tuning/instrumentation knob: name/value pairs understood by the engine
 * ("fuse", "conv_threads", ...).  Returns 0 if the knob exists.  Knobs that change where a stream's state lives
 * ("fuse", "fuse_hb", "fuse_hbd", "fold_tail", "fast_conv", "pair_conv", "pair_two", "pair_split", "pair_solo", "align_groups", "park", "fuse_latency")
 * or how a stream is rounded ("solo_fuse", "up3_poly", "half", "half_fused", "quad", "form_channels") are
 * refused (-1) once samples have been processed, until r8b_batch_clear().  "half" / "half_fused" (default 1: objects whose
 * largest call holds at least 512 workgroups of the stage -- channel pairs x overlap-save blocks --; 2: every object; 0: never): the half-array forms of the 2x up-sampling, 2x decimating and fused
 * 2048 -> 4096-point pair kernels -- the full-array kernels' arithmetic with three or four workgroups
 * per CU instead of two; results agree with theirs to rounding (RMS 4e-17), the choice is a constant of the object.  "park" (default 1): every overlap-save
 * block is computed once -- the block that holds a call's last output keeps what it holds of the next call in a
 * per-channel park buffer (or writes it ahead into the next stage's ring) instead of being computed again by the next
 * call; 0 restores the recomputation.  The output stream is bit for bit the same either way.  "form_channels" (default
 * 0: the object's own channel count): the channel count the choices made by the object's size are made for -- the
 * half-array forms above, the walk form, the half-band cascade's tile, runs of half-band decimators as one kernel, the
 * channel groups of "poly_groups".  A shard of a larger batch sets it to the batch's total channel count (before the
 * first sample, like the options above) and then runs the kernels the unsharded object runs: its rows are bit for bit
 * the unsharded object's (include/r8b/BatchSharded.h). */
R8BSRC_DECL int r8b_batch_set_option(CR8BBatch b, const char* name, int value);

/* Instrumentation: with option "timing" = 1 every stage launch is bracketed by HIP events on the
 * caller's stream.  r8b_batch_stage_timing waits for the pending events of `stage` and returns
 * the accumulated kernel milliseconds and launch count since the previous query (then resets),
 * the per-channel input/output sample counts those launches covered, and the kernel's name.
 * 0 on success. */
R8BSRC_DECL int r8b_batch_stage_count(CR8BBatch b);
/* Instrumentation: a counter of the engine since creation (-1: unknown name).  "conv_blocks": overlap-save blocks
 * per channel the compile-time-sized convolver kernels were launched for (the reference computes every block once,
 * CDSPBlockConvolver.h:283-350; so does this library where a call's last block parks what it holds of the next
 * call); "park_calls": calls that took outputs from the park buffer; "park_only_calls": calls served from it alone;
 * "pcm_staged_sides": planar PCM sides of r8b_batch_process_pcm calls that had to go through the staging rows (the
 * first / last stage's kernel is built for fp64 rows only); "walk_blocks": blocks per channel that ran on the walk
 * form of the fused pair kernel; "tail_launches": calls whose history copy (the input's tail for the next call,
 * CDSPBlockConvolver.h:296-305) needed a launch of its own -- no convolver kept it and no half-band launch carried it;
 * "hbc_tile_8192": launches of the up-sampling half-band cascade on 8192-output tiles (else 4096 or less: option
 * "hbc_tile", 0 = by batch size); "clip_steps" / "clip_channel_steps": the process steps of the clip calls and the
 * channels they ran, summed (r8b_batch_resample_clips_sched); "poly_front": launches of the tiled polynomial
 * interpolator that fetched samples and bank entries together (a tile's span within 200 samples; else the two-step
 * fetch). */
R8BSRC_DECL long long r8b_batch_stat(CR8BBatch b, const char* name);
R8BSRC_DECL int r8b_batch_stage_timing(CR8BBatch b, int stage, double* ms_sum, int* launches,
	long long* in_samples, long long* out_samples, char* kernel, int cap);
/* The device symbol of `stage`'s most recent launch made with "timing" = 1, as rocprofv3 prints it without namespace
 * and argument list ("k_convp_walk<11, 1, 4, 24>"; r8b_batch_stage_timing's `kernel` is the engine's label for the
 * stage's form, e.g. "k_convp_whole" = convolver + interpolator in one launch).  "" before the first such launch.
 * Two pseudo-stages name the PCM boundary's kernels (r8b_batch_process_pcm and the r8b_batch_resample_clips entries):
 * R8B_STAGE_PCM_IN the most recent ingest launch ("k_clip_packed_rows_in"), R8B_STAGE_PCM_OUT the most recent egress
 * launch ("k_clip_sched_frames_out<false, true, true>"), each of the most recent such call made with "timing" = 1;
 * "" before the first one and after a call whose side needed no launch (a planar side that the first / last stage
 * converts itself; no sample in or out).
 * 0 on success. */
enum r8b_pseudo_stage { R8B_STAGE_PCM_IN = -1, R8B_STAGE_PCM_OUT = -2 };
R8BSRC_DECL int r8b_batch_stage_symbol(CR8BBatch b, int stage, char* symbol, int cap);

/* Last error message of the calling thread ("" if none). */
R8BSRC_DECL const char* r8b_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Part 3: host-side designer/plan queries (no device needed).  These expose the read-only
 * coefficient sets the kernels consume so that they can be compared with the reference's
 * (CDSPFIRFilter.h:220-537, CDSPFracInterpolator.h:61-189, CDSPHBUpsampler.h:47-552).
 * ------------------------------------------------------------------------------------------- */

/* Low-pass taps h[0..KernelLen) (zero-phase filter, centre at KernelLen/2, DC gain ReqGain).
 * Returns KernelLen; fills at most cap taps; *BlockLenBits and *Latency like
 * CDSPFIRFilter::getBlockLenBits/getLatency (CDSPFIRFilter.h:139-164). */
R8BSRC_DECL int r8b_design_lpfilter(double ReqNormFreq, double ReqTransBand, double ReqAtten,
	double ReqGain, int* BlockLenBits, int* Latency, double* taps, int cap);

/* The same with the phase response selectable (0 = fprLinearPhase, 1 = fprMinPhase; reference
 * CDSPFIRFilter.h:28-45).  Minimum phase: causal taps h[0..KernelLen-1]; *Latency / *LatencyFrac =
 * integer and fractional part of the group delay at DC (CDSPFIRFilter.h:476-484). */
R8BSRC_DECL int r8b_design_lpfilter_ex(double ReqNormFreq, double ReqTransBand, double ReqAtten,
	double ReqGain, int ReqPhase, int* BlockLenBits, int* Latency, double* LatencyFrac, double* taps,
	int cap);

#ifdef R8B_TEST_HOOKS
/* PARITY-TEST HOOK -- NOT part of the shipped library: libr8bsrc_hip.so neither exports this symbol nor contains its
 * code; only builds made with -DR8B_TEST_HOOKS do (tests/emul, tests/_build/libr8bsrc_hip_testhooks.so).  A
 * provider may supply the taps of a low-pass filter in place of the designer: it is asked on every designer cache miss
 * (cache unlocked) with the filter's parameters and returns the number of taps it wrote (<= cap; 0 = "not mine", the
 * designer runs), their group-delay split *Latency / *LatencyFrac and *BlockLenBits.  tests/ use it to feed the
 * REFERENCE's own minimum-phase taps (recovered from CDSPFIRFilter::getKernelBlock) through the kernels, which
 * separates kernel parity (1e-15) from the conditioning of the cepstral minimum-phase transform
 * (CDSPRealFFT.h:681-785), whose output depends on the rounding noise of the particular FFT used.  Filters obtained
 * under a provider are cached apart from designed ones; NULL removes it. */
typedef int (*r8b_lp_provider)(double ReqNormFreq, double ReqTransBand, double ReqAtten, double ReqGain,
	int ReqPhase, double* taps, int cap, int* Latency, double* LatencyFrac, int* BlockLenBits);
R8BSRC_DECL void r8b_design_set_lp_provider(r8b_lp_provider provider);

/* TIME-AXIS TEST HOOK -- test builds only, like the one above.  Leaves the object in the state it would have after
 * being fed n zero samples through process calls whose outputs are discarded (however the n samples are cut into calls:
 * the stream is bitwise chunk invariant), and returns the number of output samples those calls would have returned.
 * No kernel runs and the host cost does not depend on n: every stage's counters move by their closed forms, the egress
 * frame number the dither key reads moves with the last stage's; rings, park buffers and meters hold what a fresh
 * object's hold (all-zero input leaves every ring zero).  Everything else that bears a stream position -- block
 * indices, history-copy ranges, span rows, parked ranges -- is worked out per call from those counters.  tests/
 * test_time_axis.py uses it to put streams at positions 2^31, 2^32 and 2^40, which cost 4e9 samples and more to reach
 * by feeding.  Refused (-1, r8b_last_error): an object fed since creation or r8b_batch_clear(); n < 0; a chain that
 * holds a non-whole-step (polynomial) interpolator -- its position counter is a loop over the outputs, re-based per
 * call, so there is no closed form to step, and that kernel's rpos0 at large positions is not covered by this hook. */
R8BSRC_DECL long long r8b_batch_test_skip_silence(CR8BBatch b, long long n);
#endif

/* Fractional-delay bank (CDSPFracDelayFilterBank): rows 0..FilterFracs, FilterLen*ElementSize
 * doubles each, natural (unshuffled) element order.  FilterFracs = -1 selects the default
 * (CDSPFracInterpolator.h:79-84).  Returns the total number of doubles. */
R8BSRC_DECL int r8b_design_fracbank(int FilterFracs, int ElementSize, int InterpPoints,
	double ReqAtten, int IsThird, int* FilterLen, int* Fracs, double* table, int cap);

/* Half-band taps (CDSPHBUpsampler::getHBFilter / getHBFilterThird).  Returns the tap count. */
R8BSRC_DECL int r8b_design_hbfilter(double ReqAtten, int SteepIndex, int IsThird, double* taps,
	double* att);

/* getWholeStepping (CDSPFracInterpolator.h:644-673). */
R8BSRC_DECL int r8b_design_whole_stepping(double SSampleRate, double DSampleRate, int* InStep,
	int* OutStep);

/* The designer's caches are bounded like the reference's (r8bconf.h:90 R8B_FILTER_CACHE_MAX 96, :103
 * R8B_FRACBANK_CACHE_MAX 12; CDSPFIRFilter.h:598-694, CDSPFracInterpolator.h:516): least recently used entries that no
 * live object holds are dropped once a cache is full, so a host that sweeps ratios does not grow without limit; what a
 * live resampler uses stays alive with it.  Writes the number of entries held right now: low-pass filters,
 * fractional-delay banks, lane tables of the fused interpolator (one per ratio, at most 96). */
R8BSRC_DECL void r8b_design_cache_counts(int* Filters, int* FracBanks, int* LaneTables);

/* Host-only schedule object: the integer bookkeeping of a resampler without any device work.
 * r8b_plan_step feeds l input samples and returns how many output samples the reference's
 * process() returns for that call. */
typedef void* CR8BPlan;
R8BSRC_DECL CR8BPlan r8b_plan_create(double SrcSampleRate, double DstSampleRate, int MaxInLen,
	double ReqTransBand, double ReqAtten);
R8BSRC_DECL void r8b_plan_delete(CR8BPlan p);
R8BSRC_DECL void r8b_plan_clear(CR8BPlan p);
R8BSRC_DECL int r8b_plan_step(CR8BPlan p, int l);
R8BSRC_DECL int r8b_plan_max_out_len(CR8BPlan p);
R8BSRC_DECL int r8b_plan_inlen(CR8BPlan p, int ReqOutSamples);
R8BSRC_DECL int r8b_plan_inlen_before_outpos(CR8BPlan p, int OutPos);
R8BSRC_DECL int r8b_plan_describe(CR8BPlan p, char* buf, int cap);

R8BSRC_DECL const char* r8b_version(void);

#ifdef __cplusplus
}
#endif

#endif /* R8BSRC_HIP_INCLUDED */
