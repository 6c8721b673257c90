// tests/cxx_true_peak.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone driver of the true-peak meter (include/r8bsrc.h
// "true peak") over the host emulation: the emulation's sources and this file compiled with -fsanitize=address,undefined
// into ONE program (tests/test_true_peak.py builds and runs it; no library, nothing preloaded).  "Device" memory is the
// heap here, and every caller buffer is a malloc block of EXACTLY the size its layout needs, so a load of the meter's body
// outside the staging rows, the histories or the value arrays, or a store outside them, lands in a redzone.
//   streams  Src == Dst and 44100 -> 88200, 3 channels, calls of 1, 5, 11, 12, 13, TF - 1, TF, TF + 1, 2 TF + 3 frames
//            (TF: the kernel's tile, argv[1]), planar and interleaved F64 out, the meter read after every call
//   clips    lengths 0, 1, 10, 11, 12 and ends at a step's last output and in a step's first frame, and at a tile's edge:
//            r8b_batch_resample_clips (strided), _packed, _ex (two channels, interleaved), _sched with both flags behind
//            44100 -> 88200
// The values are compared bitwise with this file's own chain -- one multiplication and eleven std::fma per phase, the taps
// from tests/golden/true_peak_taps.json (argv[2]) -- over the call's F64 output.  Exit status 0 and "OK": all equal.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/r8bsrc.h"

namespace {

double G[3][12];
int failures = 0;

bool load_taps(const char* path)
{
	FILE* f = fopen(path, "rb");
	if (!f) return false;
	std::string s;
	char buf[4096];
	size_t n;
	while ((n = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
	fclose(f);
	int count = 0;
	for (size_t i = s.find("\"g\""); i != std::string::npos && i + 1 < s.size() && count < 36; i++)
		if (s[i] == '"' && (s.compare(i + 1, 2, "0x") == 0 || s.compare(i + 1, 3, "-0x") == 0))
		{
			G[count / 12][count % 12] = strtod(s.c_str() + i + 1, nullptr);
			count++;
		}
	return count == 36;
}

// max |y| over frames [skip, n (+ 11 with tail)) of x[0 .. n) behind hist[0 .. 11) (null: zeros), NaN skipped
double reference(const double* x, long long n, const double* hist, int skip, bool tail)
{
	std::vector<double> z(11 + (size_t) n + 11, 0.0);
	for (int k = 0; k < 11 && hist; k++) z[(size_t) k] = hist[k];
	for (long long f = 0; f < n; f++) z[(size_t) (11 + f)] = x[f];
	double m = 0.0;
	for (long long j = skip; j < n + (tail ? 11 : 0); j++)
	{
		const double* w = z.data() + 11 + j; // w[-t] = x[j - t]
		double a = std::fabs(w[-6]);
		if (a > m) m = a;
		for (int p = 0; p < 3; p++)
		{
			double acc = G[p][0] * w[0];
			for (int t = 1; t < 12; t++) acc = std::fma(G[p][t], w[-t], acc);
			a = std::fabs(acc);
			if (a > m) m = a;
		}
	}
	return m;
}

void expect_bits(const char* what, int k, int c, double got, double want)
{
	if (memcmp(&got, &want, 8) == 0) return;
	failures++;
	printf("FAIL %s, call %d, channel %d: reads %a, the chain gives %a\n", what, k, c, got, want);
}

double noise(unsigned& state)
{
	state = state * 1664525u + 1013904223u;
	return ((int) (state >> 8) - (1 << 23)) / (double) (1 << 23) * 0.999;
}

double* block(size_t doubles)
{
	double* p = (double*) malloc(doubles ? doubles * sizeof(double) : 1);
	if (!p) abort();
	return p;
}

void stream_case(const char* what, double dst, int maxin, const std::vector<int>& cuts, bool out_il)
{
	const int nch = 3;
	CR8BBatch b = r8b_batch_create(44100.0, dst, maxin, 2.0, 136.45, nch, -1);
	if (!b || r8b_batch_true_peak_enable(b, 1) != 0) { printf("FAIL %s: %s\n", what, r8b_last_error()); failures++; return; }
	const int cap = r8b_batch_max_out_len(b);
	std::vector<double> hist((size_t) nch * 11, 0.0), want((size_t) nch, 0.0), got((size_t) nch);
	unsigned state = 12345u;
	for (size_t k = 0; k < cuts.size(); k++)
	{
		const int l = cuts[k];
		double* in = block((size_t) nch * l);
		for (long long i = 0; i < (long long) nch * l; i++) in[i] = noise(state);
		// (planar rows cap apart: the last row ends with the block; interleaved frames: the entry's own bound is n <= cap)
		double* out = block((size_t) nch * cap);
		const int n = r8b_batch_process_pcm(b, in, R8B_PCM_F64, 0, l, l, out, R8B_PCM_F64, out_il, out_il ? nch : cap, nullptr);
		if (n < 0 || r8b_batch_true_peak_read(b, got.data(), 0, nullptr) != 0)
		{
			printf("FAIL %s: %s\n", what, r8b_last_error());
			failures++;
		}
		for (int c = 0; c < nch && n >= 0; c++)
		{
			std::vector<double> row((size_t) n);
			for (int f = 0; f < n; f++) row[(size_t) f] = out_il ? out[(size_t) f * nch + c] : out[(size_t) c * cap + f];
			const double v = reference(row.data(), n, hist.data() + 11 * c, 0, false);
			if (v > want[(size_t) c]) want[(size_t) c] = v;
			expect_bits(what, (int) k, c, got[(size_t) c], want[(size_t) c]);
			std::vector<double> z(hist.begin() + 11 * c, hist.begin() + 11 * c + 11);
			z.insert(z.end(), row.begin(), row.end());
			std::copy(z.end() - 11, z.end(), hist.begin() + 11 * c);
		}
		free(in);
		free(out);
	}
	r8b_batch_delete(b);
}

// K channels per clip, both sides laid out alike: strided planar (K = 1), strided interleaved, or packed (planar inside
// a region); entry 0: r8b_batch_resample_clips, 1: _ex, 2: _packed, 3: _sched with `flags`
void clip_case(const char* what, double dst, int maxin, int K, const std::vector<long long>& in_len, int entry, int flags)
{
	const int nclips = (int) in_len.size(), nch = nclips * K;
	CR8BBatch b = r8b_batch_create(44100.0, dst, maxin, 2.0, 136.45, nch, -1);
	if (!b || r8b_batch_true_peak_enable(b, 1) != 0) { printf("FAIL %s: %s\n", what, r8b_last_error()); failures++; return; }
	const bool il = entry == 1 && K > 1, packed = entry >= 2;
	std::vector<long long> out_len, in_off, out_off;
	long long max_in = 0, P = 0, in_total = 0, out_total = 0;
	for (long long n : in_len)
	{
		out_len.push_back(dst == 44100.0 ? n : r8b_clip_out_len(44100.0, dst, n));
		in_off.push_back(in_total);
		out_off.push_back(out_total);
		in_total += n * K;
		out_total += out_len.back() * K;
		if (n > max_in) max_in = n;
		if (out_len.back() > P) P = out_len.back();
	}
	const long long in_stride = il ? max_in * K : max_in, out_stride = il ? P * K : P;
	if (!packed)
	{
		in_total = in_stride * (il ? nclips : nch);
		out_total = out_stride * (il ? nclips : nch);
	}
	double* in = block((size_t) in_total);
	double* out = block((size_t) out_total);
	unsigned state = 777u;
	for (long long i = 0; i < in_total; i++) in[i] = noise(state);
	auto at = [&](const std::vector<long long>& off, const std::vector<long long>& len, long long stride, int i, long long f, int k)
	{
		if (packed) return off[(size_t) i] + k * len[(size_t) i] + f;
		return il ? i * stride + f * K + k : ((long long) i * K + k) * stride + f;
	};
	// a clip's last frame is its largest: it shows in the tail alone (Src == Dst: the output is the input)
	for (int i = 0; i < nclips; i++)
		for (int k = 0; k < K && in_len[(size_t) i] > 0; k++) in[at(in_off, in_len, in_stride, i, in_len[(size_t) i] - 1, k)] = 2.0 + i;
	for (int round = 0; round < 2; round++)
	{
		long long p;
		if (entry == 0)
			p = r8b_batch_resample_clips(b, in, R8B_PCM_F64, in_stride, in_len.data(), out, R8B_PCM_F64, out_stride, out_len.data(), nullptr);
		else if (entry == 1)
			p = r8b_batch_resample_clips_ex(b, K, in, R8B_PCM_F64, il, in_stride, in_len.data(), out, R8B_PCM_F64, il, out_stride,
				out_len.data(), nullptr);
		else if (entry == 2)
			p = r8b_batch_resample_clips_packed(b, 0, K, nullptr, in, R8B_PCM_F64, 0, 0, in_off.data(), in_len.data(), out, R8B_PCM_F64, 0,
				0, out_off.data(), out_len.data(), nullptr);
		else
			p = r8b_batch_resample_clips_sched(b, 0, K, nullptr, in, R8B_PCM_F64, 0, 0, in_off.data(), in_len.data(), out, R8B_PCM_F64, 0,
				0, out_off.data(), out_len.data(), flags, nullptr);
		std::vector<double> got((size_t) nch);
		if (p != P || r8b_batch_true_peak_read(b, got.data(), 1, nullptr) != 0)
		{
			printf("FAIL %s: %lld, %s\n", what, p, r8b_last_error());
			failures++;
			break;
		}
		for (int c = 0; c < nch; c++)
		{
			const int i = c / K;
			std::vector<double> row((size_t) out_len[(size_t) i]);
			for (long long f = 0; f < out_len[(size_t) i]; f++) row[(size_t) f] = out[at(out_off, out_len, out_stride, i, f, c % K)];
			expect_bits(what, round, c, got[(size_t) c], reference(row.data(), (long long) row.size(), nullptr, 0, true));
		}
		// the second call, quiet: nothing of the first call's loud ends is left in the history
		for (long long i = 0; i < in_total; i++) in[i] *= 1e-3;
	}
	free(in);
	free(out);
	r8b_batch_delete(b);
}

} // namespace

int main(int argc, char** argv)
{
	if (argc < 3 || !load_taps(argv[2]))
	{
		printf("usage: cxx_true_peak TILE tests/golden/true_peak_taps.json\n");
		return 2;
	}
	const int TF = atoi(argv[1]);
	const std::vector<int> cuts = {1, 5, 11, 12, 13, TF - 1, TF, TF + 1, 2 * TF + 3};
	stream_case("Src == Dst, planar", 44100.0, 2 * TF + 3, cuts, false);
	stream_case("Src == Dst, interleaved", 44100.0, 2 * TF + 3, cuts, true);
	const int L = TF + TF / 16;
	stream_case("44100 -> 88200, planar", 88200.0, L, {L, 1, 5, 11, 12, 13, L, L - 1}, false);
	stream_case("44100 -> 88200, interleaved", 88200.0, L, {L, L, 700}, true);
	const std::vector<long long> lens = {0, 1, 10, 11, 12, 100, 101, 137};
	clip_case("clips, strided", 44100.0, 50, 1, lens, 0, 0);
	clip_case("clips, packed", 44100.0, 50, 1, lens, 2, 0);
	clip_case("clips, two channels interleaved", 44100.0, 50, 2, {12, 100, 101, 1}, 1, 0);
	clip_case("clips, packed, two channels", 44100.0, 50, 2, {12, 100, 101, 0}, 2, 0);
	clip_case("clips at a tile's edge", 44100.0, TF / 2 + 1, 1, {TF, TF + 1, TF - 1, TF - 8, TF + 11, 2 * TF}, 0, 0);
	clip_case("clips, 44100 -> 88200, drop | longest first", 88200.0, 256, 1, {300, 0, 700, 128, 701, 5}, 3,
		R8B_CLIPS_DROP_FINISHED | R8B_CLIPS_LONGEST_FIRST);
	printf("%d failed\n%s\n", failures, failures ? "FAILED" : "OK");
	return failures ? 1 : 0;
}
