// r8b_pcm_codec.h -- PCM sample codec shared by the stage kernels (src_load / dst_store on planar
// caller buffers) and the transposing ingest/egress kernels (r8b_pcm.h).  Conventions: see
// r8b_pcm.h and include/r8bsrc.h.  The includer defines R8B_HD.
#ifndef R8B_PCM_CODEC_H
#define R8B_PCM_CODEC_H

#include <math.h>

#include <type_traits>

#include "r8b_launch.h"

namespace r8bhip {

R8B_HD int pcm_bytes(int fmt)
{
	switch (fmt)
	{
	case kPcmF64: return 8;
	case kPcmF32: return 4;
	case kPcmS16: return 2;
	case kPcmS24: return 3;
	case kPcmS32: return 4;
	}
	return 0;
}

R8B_HD double pcm_decode(const unsigned char* p, int fmt)
{
	switch (fmt)
	{
	case kPcmF64: return *reinterpret_cast<const double*>(p);
	case kPcmF32: return (double) *reinterpret_cast<const float*>(p);
	case kPcmS16: return (double) *reinterpret_cast<const short*>(p) * (1.0 / 32768.0);
	case kPcmS24:
	{
		// packed little-endian, no alignment: three byte loads
		int v = (int) p[0] | ((int) p[1] << 8) | ((int) (signed char) p[2] << 16);
		return (double) v * (1.0 / 8388608.0);
	}
	case kPcmS32: return (double) *reinterpret_cast<const int*>(p) * (1.0 / 2147483648.0);
	}
	return 0.0;
}

R8B_HD double pcm_quantize(double v, double scale)
{
	double q = rint(v * scale); // round half to even in both the HIP and the host build
	if (!(q >= -scale)) q = q != q ? 0.0 : -scale;
	if (q > scale - 1.0) q = scale - 1.0;
	return q;
}

R8B_HD void pcm_encode(unsigned char* p, int fmt, double v)
{
	switch (fmt)
	{
	case kPcmF64: *reinterpret_cast<double*>(p) = v; break;
	case kPcmF32: *reinterpret_cast<float*>(p) = (float) v; break;
	case kPcmS16: *reinterpret_cast<short*>(p) = (short) (int) pcm_quantize(v, 32768.0); break;
	case kPcmS24:
	{
		const int q = (int) pcm_quantize(v, 8388608.0);
		p[0] = (unsigned char) (q & 255);
		p[1] = (unsigned char) ((q >> 8) & 255);
		p[2] = (unsigned char) ((q >> 16) & 255);
		break;
	}
	case kPcmS32: *reinterpret_cast<int*>(p) = (int) (long long) pcm_quantize(v, 2147483648.0); break;
	}
}

// ------------------------------------------------------------------ dither and meters (the finishing egress kernels)
// TPDF dither as a pure function of (seed, channel, absolute output frame): include/r8bsrc.h states it, the tests
// restate it in numpy.  All arithmetic in 64-bit unsigned integers with wrap-around.
R8B_HD unsigned long long pcm_mix(unsigned long long z)
{
	z ^= z >> 30;
	z *= 0xBF58476D1CE4E5B9ULL;
	z ^= z >> 27;
	z *= 0x94D049BB133111EBULL;
	z ^= z >> 31;
	return z;
}

// the channel's key: computed once per row, not per sample
R8B_HD unsigned long long pcm_dither_key(unsigned long long seed, long long ch)
{
	return pcm_mix(seed ^ ((unsigned long long) ch * 0xD1B54A32D192ED03ULL));
}

// difference of two uniform 32-bit integers, scaled to (-1, 1) LSB: triangular, every step exact in fp64
R8B_HD double pcm_dither_keyed(unsigned long long key, long long j)
{
	const unsigned long long z = pcm_mix(key + (unsigned long long) j * 0x9E3779B97F4A7C15ULL);
	return ((double) (unsigned) (z >> 32) - (double) (unsigned) (z & 0xFFFFFFFFULL)) * (1.0 / 4294967296.0);
}

R8B_HD double pcm_dither(unsigned long long seed, long long ch, long long j)
{
	return pcm_dither_keyed(pcm_dither_key(seed, ch), j);
}

// 2^(bits - 1) of an integer format, 0 for the float formats
R8B_HD double pcm_scale(int fmt)
{
	switch (fmt)
	{
	case kPcmS16: return 32768.0;
	case kPcmS24: return 8388608.0;
	case kPcmS32: return 2147483648.0;
	}
	return 0.0;
}

// pcm_quantize with `d` LSB of dither added before rounding; *clipped: the rounded value lay outside
// [-scale, scale - 1] before saturation (NaN: not clipped, encodes as 0).
// scale is a power of two, so v * scale is exact (or overflows to the infinity the fused form rounds to as well): the
// device's contracted fma(v, scale, d) and the host's separate multiply and add (-ffp-contract=off) give the same bits.
R8B_HD double pcm_quantize_dithered(double v, double scale, double d, int* clipped)
{
	double q = rint(v * scale + d);
	*clipped = (q < -scale) | (q > scale - 1.0);
	if (!(q >= -scale)) q = q != q ? 0.0 : -scale;
	if (q > scale - 1.0) q = scale - 1.0;
	return q;
}

// stores a value pcm_quantize / pcm_quantize_dithered returned (integer formats only)
R8B_HD void pcm_store_quantized(unsigned char* p, int fmt, double q)
{
	switch (fmt)
	{
	case kPcmS16: *reinterpret_cast<short*>(p) = (short) (int) q; break;
	case kPcmS24:
	{
		const int i = (int) q;
		p[0] = (unsigned char) (i & 255);
		p[1] = (unsigned char) ((i >> 8) & 255);
		p[2] = (unsigned char) ((i >> 16) & 255);
		break;
	}
	case kPcmS32: *reinterpret_cast<int*>(p) = (int) (long long) q; break;
	}
}

// pcm_encode with dither d (0.0: none -- the bytes are pcm_encode's then); the float formats ignore d.  Returns whether
// the sample clipped: integer formats as pcm_quantize_dithered says, float formats |v| > 1
R8B_HD int pcm_encode_dithered(unsigned char* p, int fmt, double v, double d)
{
	const double scale = pcm_scale(fmt);
	if (scale == 0.0)
	{
		pcm_encode(p, fmt, v);
		return fabs(v) > 1.0;
	}
	int clipped;
	pcm_store_quantized(p, fmt, pcm_quantize_dithered(v, scale, d, &clipped));
	return clipped;
}

// What a thread has seen of one channel's samples (the fp64 values before dither).  peak: bit pattern of the largest
// |v| -- non-negative doubles order as integers; NaN (above the pattern of +Inf) skipped
struct PcmMeter
{
	unsigned long long peak = 0;
	unsigned clipped = 0, nonfinite = 0;
};

R8B_HD void pcm_meter_note(PcmMeter& m, double v, int clipped)
{
	unsigned long long b;
	__builtin_memcpy(&b, &v, 8);
	b &= 0x7FFFFFFFFFFFFFFFULL;
	if (b <= 0x7FF0000000000000ULL && b > m.peak) m.peak = b;
	m.nonfinite += b >= 0x7FF0000000000000ULL; // exponent field 2047
	m.clipped += (unsigned) clipped;
}

// ------------------------------------------------------------------ boundary codec (the ingest / egress kernels alone)
// Everything above knows the five formats a stage kernel may meet in a SrcView / DstView and stays as it is: src_load /
// dst_store decide the format per sample at run time, and every case costs the kernels bench.py times.  The one-byte
// formats -- kPcmU8, kPcmUlaw, kPcmAlaw (include/r8bsrc.h states them) -- exist only here, on top: the pcm_io_* functions
// take all eight formats and hand the five old ones to the functions above.  r8b_pcm.h and r8b_clip*.h call these.
// (pcm_io_bytes, pcm_io_dithers: r8b_launch.h, for the host side too)

// the scale a sample is rounded at on its way out: pcm_scale, 128 for U8, and G.711's 16-bit linear value; 0: a float format
R8B_HD double pcm_io_scale(int fmt)
{
	return fmt == kPcmU8 ? 128.0 : fmt == kPcmUlaw || fmt == kPcmAlaw ? 32768.0 : pcm_scale(fmt);
}

// f(std::integral_constant<int, FMT>) for the run-time format: the switch in front of every phase that is compiled per format
template<class F>
R8B_HD void pcm_io_instance(int fmt, F f)
{
	switch (fmt)
	{
	case kPcmF64: f(std::integral_constant<int, kPcmF64>()); break;
	case kPcmF32: f(std::integral_constant<int, kPcmF32>()); break;
	case kPcmS16: f(std::integral_constant<int, kPcmS16>()); break;
	case kPcmS24: f(std::integral_constant<int, kPcmS24>()); break;
	case kPcmS32: f(std::integral_constant<int, kPcmS32>()); break;
	case kPcmU8: f(std::integral_constant<int, kPcmU8>()); break;
	case kPcmUlaw: f(std::integral_constant<int, kPcmUlaw>()); break;
	case kPcmAlaw: f(std::integral_constant<int, kPcmAlaw>()); break;
	}
}

// ITU-T G.711 over a 16-bit linear value, arithmetically (include/r8bsrc.h states each line; tests/golden/g711.npz holds
// the four tables).  g711_seg(m, lb): the number of k in 0 .. 7 with m >= (1 << lb) << k, for m >= 0 -- the position of
// m's highest bit above bit lb - 1, by count-leading-zeros (the low bits set: no case for m < 1 << lb)
R8B_HD int g711_seg(int m, int lb)
{
	const int e = 32 - lb - __builtin_clz((unsigned) m | ((1u << lb) - 1u));
	return e > 8 ? 8 : e;
}

R8B_HD int g711_ulaw_decode(unsigned b)
{
	const unsigned u = ~b & 255u;
	const int t = (int) ((((u & 15u) << 3) + 0x84u) << ((u >> 4) & 7u));
	return (u & 0x80u) != 0 ? 0x84 - t : t - 0x84;
}

R8B_HD int g711_alaw_decode(unsigned b)
{
	const unsigned a = (b ^ 0x55u) & 255u, e = (a >> 4) & 7u, m = a & 15u;
	const int t = (int) (((m << 4) + (e == 0 ? 8u : 0x108u)) << (e == 0 ? 0u : e - 1u));
	return (a & 0x80u) != 0 ? t : -t;
}

// s: a 16-bit linear value, -32768 .. 32767
R8B_HD unsigned g711_ulaw_encode(int s)
{
	const int p = s >> 2;
	const bool neg = p < 0;
	int m = neg ? -p : p;
	m = (m > 8159 ? 8159 : m) + 0x21;
	const int e = g711_seg(m, 6);
	const unsigned u = e >= 8 ? 0x7Fu : (unsigned) ((e << 4) | ((m >> (e + 1)) & 15));
	return u ^ (neg ? 0x7Fu : 0xFFu);
}

R8B_HD unsigned g711_alaw_encode(int s)
{
	const int p = s >> 3;
	const bool neg = p < 0;
	const int m = neg ? -p - 1 : p;
	const int e = g711_seg(m, 5);
	const unsigned a = e >= 8 ? 0x7Fu : (unsigned) ((e << 4) | ((e < 2 ? m >> 1 : m >> e) & 15));
	return a ^ (neg ? 0x55u : 0xD5u);
}

// one byte of a one-byte format -> the sample
R8B_HD double pcm8_decode(unsigned b, int fmt)
{
	switch (fmt)
	{
	case kPcmU8: return (double) ((int) b - 128) * (1.0 / 128.0);
	case kPcmUlaw: return (double) g711_ulaw_decode(b) * (1.0 / 32768.0);
	case kPcmAlaw: return (double) g711_alaw_decode(b) * (1.0 / 32768.0);
	}
	return 0.0;
}

// a value pcm_quantize / pcm_quantize_dithered returned at pcm_io_scale(fmt) -> the byte of a one-byte format
R8B_HD unsigned pcm8_byte(int fmt, double q)
{
	switch (fmt)
	{
	case kPcmU8: return (unsigned) ((int) q + 128);
	case kPcmUlaw: return g711_ulaw_encode((int) q);
	case kPcmAlaw: return g711_alaw_encode((int) q);
	}
	return 0;
}

// the sample with dither d -> the byte of a one-byte format (G.711: d is ignored); *clipped as pcm_quantize_dithered says
R8B_HD unsigned pcm8_encode(int fmt, double v, double d, int* clipped)
{
	return pcm8_byte(fmt, pcm_quantize_dithered(v, pcm_io_scale(fmt), fmt == kPcmU8 ? d : 0.0, clipped));
}

R8B_HD double pcm_io_decode(const unsigned char* p, int fmt)
{
	return pcm_io_bytes(fmt) == 1 ? pcm8_decode(p[0], fmt) : pcm_decode(p, fmt);
}

R8B_HD void pcm_io_store_quantized(unsigned char* p, int fmt, double q)
{
	if (pcm_io_bytes(fmt) == 1) p[0] = (unsigned char) pcm8_byte(fmt, q);
	else pcm_store_quantized(p, fmt, q);
}

R8B_HD int pcm_io_encode_dithered(unsigned char* p, int fmt, double v, double d)
{
	if (pcm_io_bytes(fmt) != 1) return pcm_encode_dithered(p, fmt, v, d);
	int clipped;
	p[0] = (unsigned char) pcm8_encode(fmt, v, d, &clipped);
	return clipped;
}

R8B_HD void pcm_io_encode(unsigned char* p, int fmt, double v)
{
	if (pcm_io_bytes(fmt) == 1) pcm_io_encode_dithered(p, fmt, v, 0.0);
	else pcm_encode(p, fmt, v);
}

} // namespace r8bhip

#endif
