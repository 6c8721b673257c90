// tests/cxx_clip_sched.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone driver of r8b_batch_resample_clips_sched over the
// host emulation (tests/emul/Makefile, target `asan`: the emulation's sources and this file compiled with
// -fsanitize=address,undefined into one program, which is then run).  "Device" memory is the heap here and every
// buffer is a malloc block of EXACTLY the size its layout needs -- a packed one what r8b_clip_pack_offsets returns, a
// strided one rows x stride with the stride at its minimum -- so a load or store of the scheduled forms
// (r8b_clip_sched.h: bases for strided sides, padding behind a base, rows a dropping step leaves out) outside the
// buffers lands in a redzone.  Per case and addressing:
//   DROP_FINISHED against flags 0: the whole output block and the meters, byte for byte;
//   DROP_FINISHED | LONGEST_FIRST against flags 0 on a second object GIVEN the clips in r8b_clip_schedule's order:
//     every clip's valid frames and the meters of its channels, byte for byte.
// Exit status 0: every case ran clean and equal.
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

// one call's buffers for the clips in the order perm[] (perm[g]: the clip in position g)
struct Run
{
	std::vector<long long> in_len, out_len, in_off, out_off;
	long long in_stride = 0, out_stride = 0, P = 0;
	unsigned char* in = nullptr;
	unsigned char* out = nullptr;
	size_t out_bytes = 0;
	double peak[6];
	long long clipped[6], nonfinite[6];
	~Run()
	{
		free(in);
		free(out);
	}
	// element of (clip at position g, frame f, channel k) on a side of Kc channels per clip
	static long long at(bool packed, bool il, const std::vector<long long>& off, const std::vector<long long>& len,
		long long stride, int Kc, int g, long long f, int k)
	{
		if (packed) return off[g] + (il ? f * Kc + k : k * len[g] + f);
		return il ? g * stride + f * Kc + k : ((long long) g * Kc + k) * stride + f;
	}
};

// clip c's samples are a function of c alone, whatever position it is given
void fill(Run& r, const Case& c, bool packed, const int* perm, int nclips, const long long* all_in, const long long* all_out)
{
	const int Kc = c.Kin ? c.Kin : c.K, Bi = kBytes[c.in_fmt], Bo = kBytes[c.out_fmt];
	long long max_in = 0;
	for (int g = 0; g < nclips; g++)
	{
		r.in_len.push_back(all_in[perm[g]]);
		r.out_len.push_back(all_out[perm[g]]);
		if (r.in_len[g] > max_in) max_in = r.in_len[g];
		if (r.out_len[g] > r.P) r.P = r.out_len[g];
	}
	r.in_off.resize(nclips);
	r.out_off.resize(nclips);
	long long in_total = r8b_clip_pack_offsets(nclips, r.in_len.data(), Kc, 1, r.in_off.data());
	long long out_total = r8b_clip_pack_offsets(nclips, r.out_len.data(), c.K, 1, r.out_off.data());
	r.in_stride = max_in * (c.in_il ? Kc : 1);
	r.out_stride = r.P * (c.out_il ? c.K : 1);
	if (!packed)
	{
		in_total = (c.in_il ? nclips : nclips * Kc) * r.in_stride;
		out_total = (c.out_il ? nclips : nclips * c.K) * r.out_stride;
	}
	r.in = (unsigned char*) malloc((size_t) in_total * Bi + 1);
	r.out_bytes = (size_t) out_total * Bo;
	r.out = (unsigned char*) malloc(r.out_bytes + 1);
	memset(r.in, 0x7F, (size_t) in_total * Bi);
	memset(r.out, 0xA5, r.out_bytes);
	for (int g = 0; g < nclips; g++)
	{
		unsigned state = 12345u + 977u * (unsigned) perm[g];
		for (long long f = 0; f < r.in_len[g]; f++)
			for (int k = 0; k < Kc; k++)
				put(r.in + Run::at(packed, c.in_il, r.in_off, r.in_len, r.in_stride, Kc, g, f, k) * Bi, c.in_fmt, state);
	}
}

int call(Run& r, const Case& c, bool packed, int flags, const std::vector<double>& mix, int nch)
{
	CR8BBatch b = r8b_batch_create(44100.0, 48000.0, 2000, 2.0, 136.45, nch, 0);
	if (b == nullptr) { printf("%s: create: %s\n", c.name, r8b_last_error()); return 1; }
	if (c.dither) r8b_batch_set_dither(b, R8B_DITHER_TPDF, 0x5EEDull, 5);
	r8b_batch_meter_enable(b, 1);
	int bad = 0;
	const long long p = r8b_batch_resample_clips_sched(b, c.Kin, c.K, c.Kin ? mix.data() : nullptr, r.in, c.in_fmt, c.in_il,
		r.in_stride, packed ? r.in_off.data() : nullptr, r.in_len.data(), r.out, c.out_fmt, c.out_il, r.out_stride,
		packed ? r.out_off.data() : nullptr, r.out_len.data(), flags, nullptr);
	if (p != r.P) { printf("%s: returned %lld, not %lld: %s\n", c.name, p, r.P, r8b_last_error()); bad = 1; }
	if (r8b_batch_meter_read(b, r.peak, r.clipped, r.nonfinite, 0, nullptr) != 0) bad = 1;
	const long long steps = r8b_batch_stat(b, "clip_steps"), chs = r8b_batch_stat(b, "clip_channel_steps");
	if (steps <= 0 || chs > steps * nch || ((flags & R8B_CLIPS_DROP_FINISHED) == 0 && chs != steps * nch))
	{
		printf("%s: counters %lld / %lld\n", c.name, steps, chs);
		bad = 1;
	}
	r8b_batch_delete(b);
	return bad;
}

int run(const Case& c, bool packed)
{
	const int nch = 6, nclips = nch / c.K;
	// (longest last: the unordered dropping call can drop nothing, the ordered one nearly everything)
	const long long all_in[6] = {1999, 0, 4500, 1, 2000, 6001};
	long long all_out[6];
	for (int i = 0; i < nclips; i++) all_out[i] = r8b_clip_out_len(44100.0, 48000.0, all_in[i]);
	// (so that the unordered dropping call drops something too: the last clip cut short)
	all_out[nclips - 1] = nclips > 1 ? 700 : all_out[0];
	std::vector<double> mix;
	for (int j = 0; j < c.K * c.Kin; j++) mix.push_back(((j * 7 + 3) % 17 - 8) / 8.0);
	int ident[6] = {0, 1, 2, 3, 4, 5}, order[6];
	if (r8b_clip_schedule(nclips, all_out, R8B_CLIPS_LONGEST_FIRST, order) != 0) return 1;
	int bad = 0;
	Run plain, drop, sched, given;
	fill(plain, c, packed, ident, nclips, all_in, all_out);
	fill(drop, c, packed, ident, nclips, all_in, all_out);
	fill(sched, c, packed, ident, nclips, all_in, all_out);
	fill(given, c, packed, order, nclips, all_in, all_out);
	bad |= call(plain, c, packed, 0, mix, nch);
	bad |= call(drop, c, packed, R8B_CLIPS_DROP_FINISHED, mix, nch);
	bad |= call(sched, c, packed, R8B_CLIPS_DROP_FINISHED | R8B_CLIPS_LONGEST_FIRST, mix, nch);
	bad |= call(given, c, packed, 0, mix, nch);
	if (!bad && (memcmp(plain.out, drop.out, plain.out_bytes) != 0 || memcmp(plain.peak, drop.peak, sizeof(plain.peak)) != 0 ||
		memcmp(plain.clipped, drop.clipped, sizeof(plain.clipped)) != 0))
	{
		printf("%s: the dropping call differs from flags 0\n", c.name);
		bad = 1;
	}
	const int Bo = kBytes[c.out_fmt];
	for (int g = 0; g < nclips && !bad; g++)
	{
		const int i = order[g];
		for (int k = 0; k < c.K && !bad; k++)
		{
			if (memcmp(&sched.peak[i * c.K + k], &given.peak[g * c.K + k], sizeof(double)) != 0 && !c.dither)
			{
				printf("%s: clip %d channel %d: the meters differ\n", c.name, i, k);
				bad = 1;
			}
			for (long long f = 0; f < all_out[i] && !bad && !c.dither; f++)
			{
				const long long se = Run::at(packed, c.out_il, sched.out_off, sched.out_len, sched.out_stride, c.K, i, f, k);
				const long long ge = Run::at(packed, c.out_il, given.out_off, given.out_len, given.out_stride, c.K, g, f, k);
				if (memcmp(sched.out + se * Bo, given.out + ge * Bo, (size_t) Bo) != 0)
				{
					printf("%s: clip %d frame %lld channel %d differs from the call given the order\n", c.name, i, f, k);
					bad = 1;
				}
			}
		}
	}
	// the padding of a strided output under order and drop: whatever is no valid frame equals the plain call's byte
	for (int i = 0; i < nclips && !bad && !packed; i++)
		for (int k = 0; k < c.K && !bad; k++)
			for (long long f = all_out[i]; f < plain.P; f++)
			{
				const long long e = Run::at(false, c.out_il, plain.out_off, plain.out_len, plain.out_stride, c.K, i, f, k);
				if (memcmp(sched.out + e * Bo, plain.out + e * Bo, (size_t) Bo) != 0)
				{
					printf("%s: clip %d frame %lld channel %d: padding differs\n", c.name, i, f, k);
					bad = 1;
					break;
				}
			}
	printf("%-30s %-7s %s\n", c.name, packed ? "packed" : "strided", bad ? "FAILED" : "ok");
	return bad;
}

} // namespace

int main()
{
	// (a dithered case compares drop against flags 0 only: under order the keys are by the caller's channel while the
	// call GIVEN the order keys by position -- tests/test_clip_sched.py checks dither under order on a Src == Dst object)
	const Case cases[] = {
		{"rows S16 -> F32", 0, 1, R8B_PCM_S16, 0, R8B_PCM_F32, 0, 0},
		{"rows K=2 F64 -> S16 dither", 0, 2, R8B_PCM_F64, 0, R8B_PCM_S16, 0, 1},
		{"tiles K=2 S24 -> S24", 0, 2, R8B_PCM_S24, 1, R8B_PCM_S24, 1, 0},
		{"tiles K=3 F32 -> rows S32", 0, 3, R8B_PCM_F32, 1, R8B_PCM_S32, 0, 0},
		{"rows K=3 S32 -> tiles F64", 0, 3, R8B_PCM_S32, 0, R8B_PCM_F64, 1, 0},
		{"mix 2 -> 1 tiles S16 -> F32", 2, 1, R8B_PCM_S16, 1, R8B_PCM_F32, 0, 0},
		{"mix 3 -> 2 rows F32 -> tiles", 3, 2, R8B_PCM_F32, 0, R8B_PCM_F64, 1, 0},
		{"tiles K=2 S16 -> S24 dither", 0, 2, R8B_PCM_S16, 1, R8B_PCM_S24, 1, 1},
	};
	int bad = 0;
	for (const Case& c : cases)
	{
		bad |= run(c, true);
		bad |= run(c, false);
	}
	return bad;
}
