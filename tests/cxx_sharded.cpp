// tests/cxx_sharded.cpp -- compiled (hipcc) and run by tests/test_gpu_parity.py::test_cxx_batch_sharded: the C++ multi-device
// helper include/r8b/BatchSharded.h on the one GPU of the test box -- 11 channels over three shards on device 0 (4 + 4 + 3:
// whole pairs, the last shard ending in a channel without a partner), each on a stream of its own, against ONE object over all 11 channels:
// bitwise equal, call by call, ragged call lengths; then 130 channels over two shards that fall below the half-array
// threshold while the whole batch is above it (the shards run the batch's kernels: option form_channels), with the same
// device symbol per stage.  Exit code 0 and "OK" = equal.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/r8b/BatchSharded.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
	fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 10; } } while (0)

static double splitmix(uint64_t& s)
{
	uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
	z ^= z >> 31;
	return (double) (z >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
}

// one batch of nch channels through BatchSharded over `devices` and through ONE object, call by call: bitwise equal rows,
// the same per-call counts and the same device symbol per stage.  Returns 0 when equal.
static int run_case(int nch, int L, const std::vector<int>& lens, const std::vector<int>& devices, uint64_t seed)
{
	r8b::BatchSharded sh(44100.0, 96000.0, L, 2.0, 180.15, nch, devices);
	CR8BBatch all = r8b_batch_create(44100.0, 96000.0, L, 2.0, 180.15, nch, 0);
	if (all == nullptr) return 2;
	r8b_batch_set_option(all, "timing", 1);
	for (int g = 0; g < sh.shards(); g++)
		if (sh.handle(g)) r8b_batch_set_option(sh.handle(g), "timing", 1);
	const int cap = sh.getMaxOutLen();
	if (cap != r8b_batch_max_out_len(all)) return 4;
	std::vector<hipStream_t> st((size_t) sh.shards() + 1);
	for (hipStream_t& s : st) CHECK(hipStreamCreate(&s));
	double *d_in, *d_out, *d_out2;
	CHECK(hipMalloc(&d_in, sizeof(double) * L * nch));
	CHECK(hipMalloc(&d_out, sizeof(double) * cap * nch));
	CHECK(hipMalloc(&d_out2, sizeof(double) * cap * nch));
	std::vector<double> in((size_t) L * nch), a((size_t) cap * nch), b((size_t) cap * nch);
	long long total = 0;
	for (int l : lens)
	{
		for (int ch = 0; ch < nch; ch++)
			for (int i = 0; i < l; i++) in[(size_t) ch * L + i] = splitmix(seed);
		CHECK(hipMemcpy(d_in, in.data(), sizeof(double) * L * nch, hipMemcpyHostToDevice));
		CHECK(hipMemset(d_out, 0xff, sizeof(double) * cap * nch));
		CHECK(hipMemset(d_out2, 0xff, sizeof(double) * cap * nch));
		int n = -1;
		for (int g = 0; g < sh.shards(); g++)
		{
			const int c0 = sh.first_channel(g);
			const int m = sh.process(g, d_in + (size_t) c0 * L, L, l, d_out + (size_t) c0 * cap, cap, st[(size_t) g]);
			if (n >= 0 && m != n) return 5;
			n = m;
		}
		const int n2 = r8b_batch_process(all, d_in, L, l, d_out2, cap, st.back());
		if (n2 != n) return 6;
		for (hipStream_t s : st) CHECK(hipStreamSynchronize(s));
		CHECK(hipMemcpy(a.data(), d_out, sizeof(double) * cap * nch, hipMemcpyDeviceToHost));
		CHECK(hipMemcpy(b.data(), d_out2, sizeof(double) * cap * nch, hipMemcpyDeviceToHost));
		for (int ch = 0; ch < nch; ch++)
			if (n > 0 && memcmp(&a[(size_t) ch * cap], &b[(size_t) ch * cap], sizeof(double) * (size_t) n) != 0)
			{
				fprintf(stderr, "%d channels: channel %d differs (call of %d samples)\n", nch, ch, l);
				return 7;
			}
		total += n;
	}
	if (total <= 0) return 8;
	char want[96], got[96];
	for (int s = 0; s < r8b_batch_stage_count(all); s++)
	{
		if (r8b_batch_stage_symbol(all, s, want, sizeof want) != 0) return 9;
		for (int g = 0; g < sh.shards(); g++)
			if (sh.handle(g) && (r8b_batch_stage_symbol(sh.handle(g), s, got, sizeof got) != 0 || strcmp(want, got) != 0))
			{
				fprintf(stderr, "%d channels: shard %d stage %d ran %s, the whole batch %s\n", nch, g, s, got, want);
				return 11;
			}
	}
	CHECK(hipFree(d_in));
	CHECK(hipFree(d_out));
	CHECK(hipFree(d_out2));
	for (hipStream_t s : st) CHECK(hipStreamDestroy(s));
	r8b_batch_delete(all);
	printf("%d channels: %lld outputs per channel\n", nch, total);
	return 0;
}

int main()
{
	{
		// 11 channels over three shards (4 + 4 + 3)
		r8b::BatchSharded sh(44100.0, 96000.0, 3000, 2.0, 180.15, 11, { 0, 0, 0 });
		if (sh.shards() != 3 || sh.shard_channels(0) != 4 || sh.shard_channels(1) != 4 || sh.shard_channels(2) != 3 ||
			sh.first_channel(1) != 4 || sh.first_channel(2) != 8 || sh.device(0) != 0)
		{
			fprintf(stderr, "shards: %d %d %d\n", sh.shard_channels(0), sh.shard_channels(1), sh.shard_channels(2));
			return 3;
		}
	}
	if (int rc = run_case(11, 3000, { 3000, 3000, 1, 777, 3000, 2, 2999, 3000 }, { 0, 0, 0 }, 11)) return rc;
	// 130 channels at 16384 per call: 13 overlap-save blocks per call, so the whole batch (65 pairs x 13 = 845 workgroups)
	// is above the half-array threshold of 512 (Engine::half_worth) and each shard of 66 + 64 (33 x 13 = 429) below it
	if (int rc = run_case(130, 16384, { 16384, 7777, 16384 }, { 0, 0 }, 130)) return rc;
	printf("OK\n");
	return 0;
}
