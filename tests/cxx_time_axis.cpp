// tests/cxx_time_axis.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone driver of the batch object at stream positions past
// 2^31 and 2^32 over the host emulation (tests/emul/Makefile, target `ubsan`: the emulation's sources and this file
// compiled with -fsanitize=signed-integer-overflow,shift -fno-sanitize-recover into one program, which is then run).
// The test builds' r8b_batch_test_skip_silence puts an object just in front of a boundary, noise then carries a stream
// across it: once the chain's INPUT, once its OUTPUT, for 44100 -> 96000 (fused pair kernel, parked outputs),
// 44100 -> 2822400 (half-band cascade, carried history copy) and 2822400 -> 176400 (decimating cascade), three channels.
// Every host-side position computation of the engine, the plan and the emulated kernels runs with the values of those
// positions; a signed overflow or an out-of-range shift among them ends the program with a report.  (The unsigned
// wrap of SrcBlock::b_lo is intended: the unsigned check stays off.)  tests/test_time_axis.py compares the samples;
// this program only asks that they are finite, that the counts add up and that the boundary was crossed.
// Exit status 0: every case ran clean.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../include/r8bsrc.h" // (compiled with -DR8B_TEST_HOOKS: the hook's declaration)

namespace {

struct Chain
{
	double src, dst;
	int maxin;
};

const int kCh = 3;

int run(const Chain& c, long long B, bool output_side)
{
	CR8BBatch b = r8b_batch_create(c.src, c.dst, c.maxin, 2.0, 180.15, kCh, 0);
	if (b == nullptr) { printf("create: %s\n", r8b_last_error()); return 1; }
	const long long lat = r8b_batch_inlen_before_outpos(b, 0);
	// the boundary falls two calls behind the point where outputs start to flow
	const long long at = output_side ? (long long) std::floor((double) B * c.src / c.dst) + lat : B;
	const long long T = at - lat - 2 * c.maxin;
	long long out_pos = r8b_batch_test_skip_silence(b, T);
	if (out_pos < 0) { printf("skip: %s\n", r8b_last_error()); return 1; }
	long long in_pos = T;
	const long long in0 = in_pos, out0 = out_pos;
	const int cap = r8b_batch_max_out_len(b);
	std::vector<double> x((size_t) kCh * c.maxin), y((size_t) kCh * (cap > 0 ? cap : 1));
	unsigned state = 12345u;
	const int lens[6] = { c.maxin, c.maxin / 3 + 1, 1, c.maxin - 7, 17, c.maxin };
	double level = 0.0;
	for (int i = 0; in_pos < at + 2 * c.maxin; i++)
	{
		const int l = lens[i % 6];
		for (int ch = 0; ch < kCh; ch++)
			for (int k = 0; k < l; k++)
			{
				state = state * 1664525u + 1013904223u;
				x[(size_t) ch * l + k] = (double) (state >> 8) / 8388608.0 - 1.0;
			}
		const int n = r8b_batch_process_host(b, x.data(), l, l, y.data(), cap);
		if (n < 0) { printf("process: %s\n", r8b_last_error()); return 1; }
		for (int ch = 0; ch < kCh; ch++)
			for (int k = 0; k < n; k++)
			{
				const double v = y[(size_t) ch * cap + k];
				if (!(std::fabs(v) < 16.0)) { printf("output %g at %lld\n", v, out_pos + k); return 1; }
				if (std::fabs(v) > level) level = std::fabs(v);
			}
		in_pos += l;
		out_pos += n;
	}
	r8b_batch_delete(b);
	const bool crossed = output_side ? out0 < B && out_pos > B : in0 < B && in_pos > B;
	// (the counts: what went in, at the chain's ratio, less what the latency still holds)
	const double want = (double) (in_pos - lat) * c.dst / c.src;
	const bool counts = std::fabs((double) out_pos - want) <= 4.0 * c.dst / c.src + 4.0;
	printf("%g -> %g, %s across 2^%d: inputs %lld .. %lld, outputs %lld .. %lld, peak %.3f%s%s%s\n", c.src, c.dst,
		output_side ? "output" : "input", B == (1LL << 31) ? 31 : 32, in0, in_pos, out0, out_pos, level,
		crossed ? "" : " NOT CROSSED", counts ? "" : " COUNTS", level > 0.1 ? "" : " SILENT");
	return crossed && counts && level > 0.1 ? 0 : 1;
}

} // namespace

int main()
{
	const Chain chains[3] = { { 44100.0, 96000.0, 4096 }, { 44100.0, 2822400.0, 1024 }, { 2822400.0, 176400.0, 4096 } };
	int bad = 0;
	for (const Chain& c : chains)
		for (int bits = 31; bits <= 32; bits++)
			for (int side = 0; side < 2; side++)
				bad += run(c, 1LL << bits, side != 0);
	printf(bad ? "FAILED\n" : "OK\n");
	return bad ? 1 : 0;
}
