// tests/cxx_pcm_boundary.cpp -- TEST INFRASTRUCTURE ONLY: every kernel of the PCM boundary (tests/pcm_boundary_cases.py) in
// every sample format once under AddressSanitizer and UndefinedBehaviorSanitizer on the host (tests/emul/Makefile, target
// `boundary`: the emulation's sources and this file as ONE program, nothing preloaded).
// The 48 forms are started through the launcher itself (launch_pcm_in / launch_pcm_out of tests/emul/emul_pcm.cpp, i.e.
// r8b_pcm_dispatch.h and the kernels' own phases), so the <DITHER, ...> forms meet the float and G.711 formats too, which
// no call of the C ABI hands them.  The emulation's "device memory" is host memory: every buffer is a heap block sized to
// the byte -- the PCM side to its last valid sample (a packed side: the regions end to end, of odd lengths, so bases fall
// on every byte alignment), the staging rows to the window -- and a read past an input's last sample, before a packed
// clip's base or past a tile is an overrun the sanitizer sees here and no device run can.
// Per form and format: six rows (clips of one channel for the row forms, two clips of three for the tile forms; the mixing
// ingest takes two channels per clip), a window of frames [3, 3 + n) with n five frames past a tile (a row form: past a
// chunk), clips that are empty, end inside the window and run past it.  Checked: the symbol the launcher noted, that an
// ingest wrote every staging sample of the window and an egress every valid sample (a padding form: the whole window)
// and nothing else, and the launcher's three refusals by their words.
// Exit status 0, "48 forms, 0 failed" and a last line "OK": every form ran clean.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "r8b_launch.h"

using namespace r8bhip;

namespace {

struct Form
{
	std::string name;
	bool egress, clip, tiles;
	int addr; // 0 strided, 1 packed, 2 scheduled
	bool dither, meter, pad, mix;
};

std::string sym(const std::string& name, std::initializer_list<bool> a)
{
	std::string s = name + "<";
	for (const bool* p = a.begin(); p != a.end(); p++) s += std::string(p == a.begin() ? "" : ", ") + (*p ? "true" : "false");
	return s + ">";
}

std::vector<Form> table()
{
	std::vector<Form> t = {
		{"k_pcm_in", false, false, true, 0, false, false, false, false},
		{"k_pcm_rows_in", false, false, false, 0, false, false, false, false},
		{"k_clip_rows_in", false, true, false, 0, false, false, false, false},
		{"k_clip_frames_in", false, true, true, 0, false, false, false, false},
		{"k_clip_mix_in", false, true, true, 0, false, false, false, true},
		{"k_clip_packed_rows_in", false, true, false, 1, false, false, false, false},
		{"k_clip_packed_frames_in", false, true, true, 1, false, false, false, false},
		{"k_clip_packed_mix_in", false, true, true, 1, false, false, false, true},
		{"k_pcm_out", true, false, true, 0, false, false, false, false},
		{"k_pcm_rows_out", true, false, false, 0, false, false, false, false},
	};
	for (int dm = 0; dm < 4; dm++)
	{
		const bool d = (dm & 2) != 0, m = (dm & 1) != 0;
		if (dm != 0)
		{
			t.push_back({sym("k_pcm_finish", {d, m}), true, false, true, 0, d, m, false, false});
			t.push_back({sym("k_pcm_rows_finish", {d, m}), true, false, false, 0, d, m, false, false});
		}
		t.push_back({sym("k_clip_rows_out", {d, m}), true, true, false, 0, d, m, true, false});
		t.push_back({sym("k_clip_frames_out", {d, m}), true, true, true, 0, d, m, true, false});
		t.push_back({sym("k_clip_packed_rows_out", {d, m}), true, true, false, 1, d, m, false, false});
		t.push_back({sym("k_clip_packed_frames_out", {d, m}), true, true, true, 1, d, m, false, false});
		for (int p = 0; p < 2; p++)
		{
			t.push_back({sym("k_clip_sched_rows_out", {d, m, p != 0}), true, true, false, 2, d, m, p != 0, false});
			t.push_back({sym("k_clip_sched_frames_out", {d, m, p != 0}), true, true, true, 2, d, m, p != 0, false});
		}
	}
	return t;
}

const int kFormats[] = {kPcmF64, kPcmF32, kPcmS32, kPcmS24, kPcmS16, kPcmU8, kPcmUlaw, kPcmAlaw};
const unsigned char kSentinel = 0xA5;
const int kRows = 6;
const long long kFrame0 = 3;

// one form in one format; returns the number of failed checks
int run(const Form& f, int fmt)
{
	int bad = 0;
	const int B = pcm_io_bytes(fmt);
	const int K = f.clip && f.tiles ? 3 : 1, Kc = f.mix ? 2 : K;       // object / PCM-side channels per clip
	const int nclips = kRows / K, prow = nclips * Kc;                    // rows of the PCM side
	const long long unit = f.tiles ? (f.clip ? 512 : 64) : 2048;        // (K = 3 and a mix of two: tiles of 512 frames)
	const long long n = unit + 5, T = kFrame0 + n;
	const bool il = f.tiles && (f.clip ? Kc > 1 : true);
	const bool based = f.addr != 0, padded = !f.clip || f.pad;
	// the clips' lengths: empty, inside the window, past it, ...
	std::vector<long long> len((size_t) kRows), base;
	for (int i = 0; i < nclips; i++)
		for (int k = 0; k < K; k++) len[(size_t) (i * K + k)] = i % 3 == 0 ? 0 : i % 3 == 1 ? T - 2 : T + 9;
	// the PCM side, sized to the byte
	long long elems = 0, stride = 0;
	if (!f.clip)
	{
		stride = il ? kRows : n;
		elems = n * kRows;
	}
	else if (!based)
	{
		// (an ingest never loads past a clip's length, but its rows lie a stride apart all the same)
		stride = il ? T * Kc : T;
		elems = (il ? nclips : prow) * stride;
	}
	else
	{
		// regions end to end, last clip first: per clip (interleaved) or per row (planar)
		base.assign((size_t) (il ? nclips : prow), 0);
		for (int i = nclips - 1; i >= 0; i--)
		{
			const long long fr = f.addr == 2 && f.pad ? T : len[(size_t) (i * K)]; // (PAD: the window's end; else the clip)
			if (il)
			{
				base[(size_t) i] = elems;
				elems += fr * Kc;
			}
			else
				for (int k = 0; k < Kc; k++)
				{
					base[(size_t) (i * Kc + k)] = elems;
					elems += fr;
				}
		}
	}
	if (f.clip && !based && !f.egress)
		// a strided ingest: the last clip's rows end at its last valid frame (what lies behind is never read)
		elems -= (il ? Kc : 1) * (T - std::min(T, len[(size_t) (kRows - 1)]));
	std::vector<unsigned char>* pcm = new std::vector<unsigned char>((size_t) (elems * B), f.egress ? kSentinel : (unsigned char) 0x40);
	std::vector<double>* planar = new std::vector<double>((size_t) (kRows * n));
	for (size_t j = 0; j < planar->size(); j++) (*planar)[j] = f.egress ? 0.6 * std::sin(0.37 * (double) j) : NAN;
	if (f.egress)
	{
		(*planar)[0] = 2.0;
		(*planar)[1] = INFINITY;
		(*planar)[2] = NAN;
	}
	std::vector<unsigned long long> meters((size_t) (3 * kRows), 0);
	std::vector<long long> chan((size_t) kRows);
	for (int r = 0; r < kRows; r++) chan[(size_t) r] = kRows - 1 - r;
	const double mixm[6] = {0.5, 0.25, 0.0, -0.5, 0.25, 0.0};
	PcmLaunch L;
	L.pcm = pcm->data();
	L.fmt = fmt;
	L.interleaved = il ? 1 : 0;
	L.pcm_stride = stride;
	L.planar = planar->data();
	L.planar_stride = n;
	L.nch = kRows;
	L.n = n;
	if (f.dither)
	{
		L.dither = 1;
		L.seed = 0x5EEDC0DE12345678ULL;
		L.first_channel = 5;
	}
	if (f.meter)
	{
		L.m_peak = meters.data();
		L.m_clipped = L.m_peak + kRows;
		L.m_nonfinite = L.m_clipped + kRows;
	}
	if (f.clip)
	{
		L.clip_len = len.data();
		L.clip_channels = K;
		L.frame0 = L.in_frame0 = kFrame0;
		if (f.mix)
		{
			L.mix_channels = Kc;
			L.mix = mixm;
		}
		if (based) L.clip_base = base.data();
		if (f.addr == 2)
		{
			// (PAD alone makes a scheduled launch too: the channels' array in every other one)
			if (!f.pad || f.dither) L.clip_chan = chan.data();
			L.clip_pad = f.pad ? 1 : 0;
		}
	}
	else L.frame0 = 1000;
	launch_symbol_note(nullptr);
	if (f.egress) launch_pcm_out(L, nullptr);
	else launch_pcm_in(L, nullptr);
	const char* s = launch_symbol_last();
	if (s == nullptr || f.name != s)
	{
		printf("%s fmt %d: the launcher noted %s\n", f.name.c_str(), fmt, s ? s : "(nothing)");
		bad++;
	}
	if (!f.egress)
	{
		// every staging sample of the window is written: a number, and +0.0 past the clip's end
		for (int r = 0; r < kRows; r++)
			for (long long j = 0; j < n; j++)
			{
				const double v = (*planar)[(size_t) (r * n + j)];
				const bool past = f.clip && kFrame0 + j >= len[(size_t) r];
				if (v != v || (past && (v != 0.0 || std::signbit(v))))
				{
					printf("%s fmt %d: staging row %d frame %lld holds %g\n", f.name.c_str(), fmt, r, j, v);
					bad++;
					j = n;
				}
			}
	}
	else if (B > 1)
	{
		// every sample the form owes is written and no other (the multi-byte formats: none encodes a sample of these rows
		// as kSentinel bytes throughout)
		long long untouched = 0;
		for (long long e = 0; e < elems; e++)
		{
			bool all = true;
			for (int b = 0; b < B; b++) all = all && (*pcm)[(size_t) (e * B + b)] == kSentinel;
			untouched += all;
		}
		long long owed = 0;
		for (int r = 0; r < kRows; r++)
		{
			const long long v = f.clip ? std::max(0LL, std::min(T, len[(size_t) r]) - kFrame0) : n;
			owed += padded ? n : v;
		}
		if (elems - untouched != owed)
		{
			printf("%s fmt %d: %lld samples written, %lld owed\n", f.name.c_str(), fmt, elems - untouched, owed);
			bad++;
		}
	}
	if (f.meter && (meters[0] != 0x7FF0000000000000ULL || meters[(size_t) kRows] < 2 || meters[(size_t) (2 * kRows)] != 2) && !f.clip)
	{
		printf("%s fmt %d: meters of channel 0: peak %llx clipped %llu nonfinite %llu\n", f.name.c_str(), fmt, meters[0],
			meters[(size_t) kRows], meters[(size_t) (2 * kRows)]);
		bad++;
	}
	delete pcm;
	delete planar;
	return bad;
}

int refusal(const char* words, bool egress, void (*set)(PcmLaunch&))
{
	static double rows[64];
	static unsigned char bytes[512];
	static const long long len[6] = {1, 1, 1, 1, 1, 1};
	static unsigned long long m[6];
	PcmLaunch L;
	L.pcm = bytes;
	L.fmt = kPcmS16;
	L.interleaved = 1;
	L.pcm_stride = 8;
	L.planar = rows;
	L.planar_stride = 4;
	L.nch = 6;
	L.n = 1;
	L.clip_len = len;
	L.clip_channels = 3;
	L.m_peak = m;
	L.m_clipped = L.m_nonfinite = m;
	set(L);
	try
	{
		if (egress) launch_pcm_out(L, nullptr);
		else launch_pcm_in(L, nullptr);
	}
	catch (const std::logic_error& e)
	{
		if (strstr(e.what(), words) != nullptr) return 0;
		printf("refusal: \"%s\" where \"%s\" was due\n", e.what(), words);
		return 1;
	}
	printf("refusal: \"%s\" did not come\n", words);
	return 1;
}

} // namespace

int main()
{
	int failed = 0, forms = 0;
	for (const Form& f : table())
	{
		int bad = 0;
		for (int fmt : kFormats) bad += run(f, fmt);
		forms++;
		failed += bad != 0;
	}
	int bad = 0;
	bad += refusal("clip_channels must be 1 .. 64 and divide the channel count", false, [](PcmLaunch& L) { L.clip_channels = 4; });
	bad += refusal("clip_channels must be 1 .. 64 and divide the channel count", true, [](PcmLaunch& L) { L.clip_channels = 65; });
	bad += refusal("mix_channels must be 1 .. 64 and come with a matrix", false, [](PcmLaunch& L) { L.mix_channels = 2; });
	bad += refusal("meters need all three arrays", true, [](PcmLaunch& L) { L.m_nonfinite = nullptr; });
	printf("%d forms, %d failed\n", forms, failed);
	if (failed != 0 || bad != 0 || forms != 48) return 1;
	printf("OK\n");
	return 0;
}
