// tests/cxx_loudness.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone driver of the loudness meter (include/r8bsrc.h
// "loudness") over the host emulation: the emulation's sources and this file compiled with -fsanitize=address,undefined
// into ONE program (tests/test_loudness.py builds and runs it; no library, nothing preloaded).  "Device" memory is the
// heap here, and every caller buffer is a malloc block of EXACTLY the size its layout needs, so a load of the meter's body
// outside the staging rows, the state or the store, or a store outside them, lands in a redzone.
//   streams  8000 -> 8000 and 16000 -> 8000, 2 channels, cut at 1, 63, 64, 65, H - 1, H, H + 1, T - 1, T, T + 1 frames
//            (T: the kernel's tile, argv[1]; H = 800) and the rest; the store read into blocks of counts x channels
//   clips    lengths 0, 1, 63, 64, H - 1, H, 2 H + 100, 3 H + 37: r8b_batch_resample_clips (strided), _packed, _ex (two
//            channels, interleaved), _sched with both flags behind 16000 -> 8000; twice on one object
// The sums are compared bitwise with this file's own restatement of the definition -- std::fma, the constants from
// r8b_loudness_design -- over the call's F64 output.  Exit status 0 and "OK": all equal.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/r8bsrc.h"

namespace {

const int M = 64;
const long long H = 800;
int failures = 0;
double coef[10], phi[16];

double frame(double x, double* s)
{
	const double* c = coef;
	const double y = std::fma(c[0], x, s[0]);
	s[0] = std::fma(-c[3], y, std::fma(c[1], x, s[1]));
	s[1] = std::fma(-c[4], y, c[2] * x);
	const double z = std::fma(c[5], y, s[2]);
	s[2] = std::fma(-c[8], z, std::fma(c[6], y, s[3]));
	s[3] = std::fma(-c[9], z, c[7] * y);
	return z;
}

// the sums of the sub-blocks x[0 .. n) completes: a stream's whole segments; a clip's last segment filled with zeros, and
// n / H sub-blocks
std::vector<double> reference(const double* x, long long n, bool clip)
{
	const long long nseg = clip ? (n + M - 1) / M : n / M;
	std::vector<double> sums;
	double S[4] = {0, 0, 0, 0}, A = 0.0;
	for (long long k = 0; k < nseg; k++)
	{
		double seg[M], s[4], Z[4] = {0, 0, 0, 0}, e[2] = {0.0, 0.0};
		for (int j = 0; j < M; j++)
		{
			const long long f = k * M + j;
			seg[j] = f < n && std::isfinite(x[f]) ? x[f] : 0.0;
		}
		memcpy(s, S, sizeof s);
		const long long b0 = k * M / H;
		for (int j = 0; j < M; j++)
		{
			const double z = frame(seg[j], s);
			double& piece = e[(k * M + j) / H - b0];
			piece = std::fma(z, z, piece);
		}
		for (int j = 0; j < M; j++) frame(seg[j], Z);
		double N[4];
		for (int i = 0; i < 4; i++)
			N[i] = std::fma(phi[4 * i + 3], S[3], std::fma(phi[4 * i + 2], S[2], std::fma(phi[4 * i + 1], S[1], std::fma(phi[4 * i], S[0], Z[i]))));
		memcpy(S, N, sizeof S);
		A = A + e[0];
		if ((b0 + 1) * H <= (k + 1) * M)
		{
			sums.push_back(A);
			A = 0.0;
			if ((b0 + 1) * H < (k + 1) * M) A = A + e[1];
		}
	}
	if (clip) sums.resize((size_t) (n / H));
	return sums;
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

// the object's store against the reference over rows[c]
void check_store(const char* what, CR8BBatch b, const std::vector<std::vector<double>>& rows, bool clip)
{
	const int nch = (int) rows.size();
	long long* counts = (long long*) malloc(sizeof(long long) * (size_t) nch);
	const long long most = r8b_batch_loudness_read(b, nullptr, 0, counts, 0, nullptr);
	if (most < 0) { printf("FAIL %s: %s\n", what, r8b_last_error()); failures++; free(counts); return; }
	double* sums = block((size_t) (most * nch));
	if (r8b_batch_loudness_read(b, sums, most, counts, 0, nullptr) != most) { printf("FAIL %s: the second read\n", what); failures++; }
	for (int c = 0; c < nch; c++)
	{
		const std::vector<double> want = reference(rows[(size_t) c].data(), (long long) rows[(size_t) c].size(), clip);
		if (counts[c] != (long long) want.size() || (want.size() && memcmp(sums + c * most, want.data(), want.size() * 8) != 0))
		{
			failures++;
			printf("FAIL %s, channel %d: %lld sub-blocks, the reference has %zu, or their bits differ\n", what, c, counts[c], want.size());
		}
	}
	free(sums);
	free(counts);
}

void stream_case(const char* what, double src, int maxin, long long total, const std::vector<int>& cuts)
{
	const int nch = 2;
	CR8BBatch b = r8b_batch_create(src, 8000.0, maxin, 2.0, 136.45, nch, -1);
	if (!b || r8b_batch_loudness_enable(b, 1, 600) != 0) { printf("FAIL %s: %s\n", what, r8b_last_error()); failures++; return; }
	const int cap = r8b_batch_max_out_len(b);
	std::vector<std::vector<double>> rows((size_t) nch);
	unsigned state = 4321u;
	std::vector<int> calls(cuts);
	long long used = 0;
	for (int l : cuts) used += l;
	while (used < total)
	{
		calls.push_back((int) (total - used < maxin ? total - used : maxin));
		used += calls.back();
	}
	for (int l : calls)
	{
		double* in = block((size_t) nch * l);
		for (long long i = 0; i < (long long) nch * l; i++) in[i] = noise(state);
		double* out = block((size_t) nch * cap);
		const int n = r8b_batch_process_pcm(b, in, R8B_PCM_F64, 0, l, l, out, R8B_PCM_F64, 0, cap, nullptr);
		if (n < 0) { printf("FAIL %s: %s\n", what, r8b_last_error()); failures++; }
		for (int c = 0; c < nch && n > 0; c++) rows[(size_t) c].insert(rows[(size_t) c].end(), out + (size_t) c * cap, out + (size_t) c * cap + n);
		free(in);
		free(out);
	}
	check_store(what, b, rows, false);
	r8b_batch_delete(b);
}

// K channels per clip, both sides laid out alike: strided planar (K = 1), strided interleaved, or packed (planar inside
// a region); entry 0: r8b_batch_resample_clips, 1: _ex, 2: _packed, 3: _sched with `flags`
void clip_case(const char* what, double src, int maxin, int K, const std::vector<long long>& in_len, int entry, int flags)
{
	const int nclips = (int) in_len.size(), nch = nclips * K;
	CR8BBatch b = r8b_batch_create(src, 8000.0, maxin, 2.0, 136.45, nch, -1);
	if (!b || r8b_batch_loudness_enable(b, 1, 8) != 0) { printf("FAIL %s: %s\n", what, r8b_last_error()); failures++; return; }
	const bool il = entry == 1 && K > 1, packed = entry >= 2;
	std::vector<long long> out_len, in_off, out_off;
	long long max_in = 0, P = 0, in_total = 0, out_total = 0;
	for (long long n : in_len)
	{
		out_len.push_back(src == 8000.0 ? n : r8b_clip_out_len(src, 8000.0, n));
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
	unsigned state = 999u;
	for (long long i = 0; i < in_total; i++) in[i] = noise(state);
	auto at = [&](const std::vector<long long>& off, const std::vector<long long>& len, long long stride, int i, long long f, int k)
	{
		if (packed) return off[(size_t) i] + k * len[(size_t) i] + f;
		return il ? i * stride + f * K + k : ((long long) i * K + k) * stride + f;
	};
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
		if (p != P)
		{
			printf("FAIL %s: %lld, %s\n", what, p, r8b_last_error());
			failures++;
			break;
		}
		std::vector<std::vector<double>> rows((size_t) nch);
		for (int c = 0; c < nch; c++)
			for (long long f = 0; f < out_len[(size_t) (c / K)]; f++)
				rows[(size_t) c].push_back(out[at(out_off, out_len, out_stride, c / K, f, c % K)]);
		check_store(what, b, rows, true);
		// the second call, other samples: state and store start empty
		for (long long i = 0; i < in_total; i++) in[i] *= -0.5;
	}
	free(in);
	free(out);
	r8b_batch_delete(b);
}

} // namespace

int main(int argc, char** argv)
{
	long long hop = 0;
	if (argc < 2 || r8b_loudness_design(8000.0, coef, phi, &hop) != 0 || hop != H)
	{
		printf("usage: cxx_loudness TILE\n");
		return 2;
	}
	const int T = atoi(argv[1]);
	const std::vector<int> cuts = {1, 63, 64, 65, (int) H - 1, (int) H, (int) H + 1, T - 1, T, T + 1};
	long long total = 333;
	for (int l : cuts) total += l;
	stream_case("8000 -> 8000, cut", 8000.0, T + 1, total, cuts);
	stream_case("8000 -> 8000, whole calls", 8000.0, T + 1, total, {});
	stream_case("16000 -> 8000, cut", 16000.0, T + 1, total, cuts);
	const std::vector<long long> lens = {0, 1, 63, 64, H - 1, H, 2 * H + 100, 3 * H + 37};
	clip_case("clips, strided", 8000.0, 500, 1, lens, 0, 0);
	clip_case("clips, packed", 8000.0, 500, 1, lens, 2, 0);
	clip_case("clips, two channels interleaved", 8000.0, 500, 2, {H, 3 * H + 37, 2 * H + 100, 65}, 1, 0);
	clip_case("clips, packed, two channels", 8000.0, 500, 2, {H, 3 * H + 37, 2 * H + 100, 0}, 2, 0);
	clip_case("clips, 16000 -> 8000, drop | longest first", 16000.0, 1000, 1, {2 * H + 77, 0, 6 * H + 130, 300, 4 * H + 2, 5 * H}, 3,
		R8B_CLIPS_DROP_FINISHED | R8B_CLIPS_LONGEST_FIRST);
	printf("%d failed\n%s\n", failures, failures ? "FAILED" : "OK");
	return failures ? 1 : 0;
}
