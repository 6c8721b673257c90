// tests/cxx_clip_packed.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone driver of r8b_batch_resample_clips_packed over the
// host emulation (tests/emul/Makefile, target `asan`: the emulation's sources and this file compiled with
// -fsanitize=address,undefined into one program, which is then run).  "Device" memory is the heap here, so every packed
// buffer is a malloc block of EXACTLY the size r8b_clip_pack_offsets returns: the first clip's base is the block's first
// byte and the last clip ends with the block, and a load or store of the packed phases (r8b_clip_packed.h) outside a
// clip's region lands in a redzone.  Each case is also compared with the strided call on padded buffers, region by
// region.  Exit status 0: every case ran clean and equal.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/r8bsrc.h"

namespace {

const int kBytes[5] = {8, 4, 2, 3, 4};

struct Case
{
	const char* name;
	int Kin, K; // Kin = 0: no mix
	int in_fmt, in_il, out_fmt, out_il;
	int dither;
};

// sample s of an input buffer in format fmt: noise on the 16-bit grid
void put(unsigned char* p, int fmt, unsigned& state)
{
	state = state * 1664525u + 1013904223u;
	const int q = (int) (state >> 16) - 32768;
	switch (fmt)
	{
	case R8B_PCM_F64: { const double v = q / 32768.0; memcpy(p, &v, 8); break; }
	case R8B_PCM_F32: { const float v = (float) (q / 32768.0); memcpy(p, &v, 4); break; }
	case R8B_PCM_S16: { const short v = (short) q; memcpy(p, &v, 2); break; }
	case R8B_PCM_S24: p[0] = 0; p[1] = (unsigned char) (q & 255); p[2] = (unsigned char) ((q >> 8) & 255); break;
	default: { const int v = q * 65536; memcpy(p, &v, 4); break; }
	}
}

int run(const Case& c)
{
	const int nch = 6, nclips = nch / c.K, Kc = c.Kin ? c.Kin : c.K;
	const long long all_len[6] = {1999, 0, 4500, 1, 2000, 6001};
	std::vector<long long> in_len(all_len, all_len + nclips), out_len(nclips), in_off(nclips), out_off(nclips);
	long long max_in = 0, P = 0;
	for (int i = 0; i < nclips; i++)
	{
		out_len[i] = r8b_clip_out_len(44100.0, 48000.0, in_len[i]);
		if (in_len[i] > max_in) max_in = in_len[i];
		if (out_len[i] > P) P = out_len[i];
	}
	const long long in_total = r8b_clip_pack_offsets(nclips, in_len.data(), Kc, 1, in_off.data());
	const long long out_total = r8b_clip_pack_offsets(nclips, out_len.data(), c.K, 1, out_off.data());
	const int Bi = kBytes[c.in_fmt], Bo = kBytes[c.out_fmt];
	// packed: exactly-sized blocks; padded: clip i at i * stride (interleaved) or its rows at (i * Kc + k) * stride
	unsigned char* pin = (unsigned char*) malloc((size_t) in_total * Bi);
	unsigned char* pout = (unsigned char*) malloc((size_t) out_total * Bo);
	const long long in_stride = max_in * (c.in_il ? Kc : 1), out_stride = P * (c.out_il ? c.K : 1);
	std::vector<unsigned char> sin((size_t) nclips * Kc * max_in * Bi, 0x7F), sout((size_t) nch * P * Bo, 0xA5);
	memset(pout, 0xA5, (size_t) out_total * Bo);
	unsigned state = 12345u;
	for (int i = 0; i < nclips; i++)
		for (long long f = 0; f < in_len[i]; f++)
			for (int k = 0; k < Kc; k++)
			{
				const long long pe = in_off[i] + (c.in_il ? f * Kc + k : k * in_len[i] + f);
				const long long se = c.in_il ? i * in_stride + f * Kc + k : ((long long) i * Kc + k) * in_stride + f;
				put(pin + pe * Bi, c.in_fmt, state);
				memcpy(sin.data() + se * Bi, pin + pe * Bi, (size_t) Bi);
			}
	std::vector<double> mix;
	for (int j = 0; j < c.K * c.Kin; j++) mix.push_back(((j * 7 + 3) % 17 - 8) / 8.0);
	int bad = 0;
	unsigned char* outs[2] = {pout, sout.data()};
	double peaks[2][6];
	for (int packed = 1; packed >= 0; packed--)
	{
		CR8BBatch b = r8b_batch_create(44100.0, 48000.0, 2000, 2.0, 136.45, nch, 0);
		if (b == nullptr) { printf("%s: create: %s\n", c.name, r8b_last_error()); return 1; }
		if (c.dither) r8b_batch_set_dither(b, R8B_DITHER_TPDF, 0x5EEDull, 5);
		r8b_batch_meter_enable(b, 1);
		const long long p = r8b_batch_resample_clips_packed(b, c.Kin, c.K, c.Kin ? mix.data() : nullptr,
			packed ? (const void*) pin : (const void*) sin.data(), c.in_fmt, c.in_il, in_stride,
			packed ? in_off.data() : nullptr, in_len.data(), outs[1 - packed], c.out_fmt, c.out_il, out_stride,
			packed ? out_off.data() : nullptr, out_len.data(), nullptr);
		if (p != P) { printf("%s: returned %lld, not %lld: %s\n", c.name, p, P, r8b_last_error()); bad = 1; }
		long long clipped[6], nonfinite[6];
		if (r8b_batch_meter_read(b, peaks[packed], clipped, nonfinite, 0, nullptr) != 0) bad = 1;
		r8b_batch_delete(b);
	}
	if (memcmp(peaks[0], peaks[1], sizeof(peaks[0])) != 0) { printf("%s: the meters differ\n", c.name); bad = 1; }
	for (int i = 0; i < nclips && !bad; i++)
		for (long long f = 0; f < out_len[i] && !bad; f++)
			for (int k = 0; k < c.K; k++)
			{
				const long long pe = out_off[i] + (c.out_il ? f * c.K + k : k * out_len[i] + f);
				const long long se = c.out_il ? i * out_stride + f * c.K + k : ((long long) i * c.K + k) * out_stride + f;
				if (memcmp(pout + pe * Bo, sout.data() + se * Bo, (size_t) Bo) != 0)
				{
					printf("%s: clip %d frame %lld channel %d differs from the strided call\n", c.name, i, f, k);
					bad = 1;
					break;
				}
			}
	free(pin);
	free(pout);
	printf("%-28s %s (%lld + %lld elements)\n", c.name, bad ? "FAILED" : "ok", in_total, out_total);
	return bad;
}

} // namespace

int main()
{
	const Case cases[] = {
		{"rows S16 -> F32", 0, 1, R8B_PCM_S16, 0, R8B_PCM_F32, 0, 0},
		{"rows K=2 F64 -> S16 dither", 0, 2, R8B_PCM_F64, 0, R8B_PCM_S16, 0, 1},
		{"tiles K=2 S24 -> S24 dither", 0, 2, R8B_PCM_S24, 1, R8B_PCM_S24, 1, 1},
		{"tiles K=3 F32 -> rows S32", 0, 3, R8B_PCM_F32, 1, R8B_PCM_S32, 0, 0},
		{"rows K=3 S32 -> tiles F64", 0, 3, R8B_PCM_S32, 0, R8B_PCM_F64, 1, 0},
		{"mix 2 -> 1 tiles S16 -> F32", 2, 1, R8B_PCM_S16, 1, R8B_PCM_F32, 0, 0},
		{"mix 3 -> 2 rows F32 -> tiles", 3, 2, R8B_PCM_F32, 0, R8B_PCM_F64, 1, 0},
		{"mix 1 -> 2 rows S24 -> rows", 1, 2, R8B_PCM_S24, 0, R8B_PCM_S24, 0, 0},
	};
	int bad = 0;
	for (const Case& c : cases) bad |= run(c);
	return bad;
}
