// tests/cxx_stage_census.cpp -- TEST INFRASTRUCTURE ONLY: the table-driven stage kernels (tests/stage_census.py) once under
// AddressSanitizer and UndefinedBehaviorSanitizer on the host (tests/emul/Makefile, target `stages`: the emulation's
// sources and this file as ONE program, nothing preloaded).
// The emulator allocates a launch's LDS arrays per launch and the engine its ring buffers per object: a half-band cascade
// that writes past its two buffers or the slack around them at depth 8, or a stage that reads past a ring, is an overrun
// the sanitizer sees here, on the CPU.
//   cxx_stage_census TABLE
// TABLE is what `python tests/stage_census.py --dump` writes: a line per entry,
//   what|kind|a|b|c|d|i0|i1|maxin|option=value,...|stage=symbol,stage=,...
// what = "stage": a stand-alone stage object of the descriptor (kind, a, b, c, d, i0, i1) -- one half-band row per tap
// count, up and down; what = "chain": a = src, b = dst, c = transition band, d = attenuation -- the up-sampling and the
// decimating chains of every cascade depth.  A stage listed with a symbol must have launched it, a stage listed without
// one is a member of the run in front of it and must have launched nothing.
// For each line: a three-channel object (full scale, 1e-6 of full scale, silence) with the library's own designer, whole
// calls of MaxInLen samples of noise until outputs flow and two more, then a call of 17 samples and one of a single
// sample; outputs must be finite and the silent channel exact zeros.  tests/test_stage_census.py compares samples.
// Exit status 0 and a last line "OK": every entry ran clean.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "../include/r8bsrc.h"

namespace {

const int kCh = 3;
const double kLevel[kCh] = { 1.0, 1e-6, 0.0 };

std::vector<std::string> split(const std::string& s, char sep)
{
	std::vector<std::string> v;
	std::stringstream ss(s);
	std::string f;
	while (std::getline(ss, f, sep)) v.push_back(f);
	if (!s.empty() && s.back() == sep) v.push_back("");
	return v;
}

int run(const std::string& line)
{
	const std::vector<std::string> f = split(line, '|');
	if (f.size() != 11) { printf("malformed line: %s\n", line.c_str()); return 1; }
	const bool chain = f[0] == "chain";
	const double a = atof(f[2].c_str()), b_ = atof(f[3].c_str()), c = atof(f[4].c_str()), d = atof(f[5].c_str());
	const int kind = atoi(f[1].c_str()), i0 = atoi(f[6].c_str()), i1 = atoi(f[7].c_str()), maxin = atoi(f[8].c_str());
	const std::string name = f[0] + " " + f[1] + " " + f[2] + " " + f[3] + " " + f[5] + " " + f[6] + " " + f[7] + " [" + f[9] + "]";
	CR8BBatch b = chain ? r8b_batch_create(a, b_, maxin, c, d, kCh, -1) :
		r8b_batch_create_stage(kind, a, b_, c, d, i0, i1, maxin, kCh, -1);
	if (b == nullptr) { printf("%s: create: %s\n", name.c_str(), r8b_last_error()); return 1; }
	int bad = 0;
	for (const std::string& kv : split(f[9], ','))
	{
		const size_t eq = kv.find('=');
		if (eq == std::string::npos || r8b_batch_set_option(b, kv.substr(0, eq).c_str(), atoi(kv.c_str() + eq + 1)) != 0)
		{
			printf("%s: option %s\n", name.c_str(), kv.c_str());
			bad = 1;
		}
	}
	if (r8b_batch_set_option(b, "timing", 1) != 0) bad = 1;
	std::vector<std::pair<int, std::string>> want;
	for (const std::string& kv : split(f[10], ','))
	{
		const size_t eq = kv.find('=');
		if (eq == std::string::npos) { printf("%s: symbol list %s\n", name.c_str(), kv.c_str()); bad = 1; continue; }
		want.emplace_back(atoi(kv.c_str()), kv.substr(eq + 1));
	}
	const int cap = r8b_batch_max_out_len(b) > 0 ? r8b_batch_max_out_len(b) : 1;
	std::vector<double> x((size_t) kCh * maxin), y((size_t) kCh * cap);
	unsigned state = 12345u;
	long long total = 0;
	double level = 0.0;
	// whole calls until outputs flow (long chains answer late: 4096 calls at the most), two more, then two short ones
	int whole = 0, after = 0;
	for (int step = 0; step < 3 && !bad;)
	{
		const int l = step == 0 ? maxin : (step == 1 ? (17 < maxin ? 17 : maxin) : 1);
		for (int ch = 0; ch < kCh; ch++)
			for (int k = 0; k < l; k++)
			{
				state = state * 1664525u + 1013904223u;
				x[(size_t) ch * l + k] = kLevel[ch] * ((double) (state >> 8) / 8388608.0 - 1.0);
			}
		const int n = r8b_batch_process_host(b, x.data(), l, l, y.data(), cap);
		if (n < 0) { printf("%s: process: %s\n", name.c_str(), r8b_last_error()); bad = 1; break; }
		for (int ch = 0; ch < kCh; ch++)
			for (int k = 0; k < n; k++)
			{
				const double v = y[(size_t) ch * cap + k];
				if (!(std::fabs(v) < 16.0 * (kLevel[ch] > 0.0 ? kLevel[ch] : 1.0)) || (ch == 2 && v != 0.0))
				{
					printf("%s: channel %d output %lld is %g\n", name.c_str(), ch, total + k, v);
					bad = 1;
				}
				if (ch == 0 && std::fabs(v) > level) level = std::fabs(v);
			}
		total += n;
		if (step == 0)
		{
			whole++;
			if (level > 1e-3) after++;
			if (after >= 3 || whole >= 4096) step++;
		}
		else step++;
	}
	for (const auto& w : want)
	{
		char sym[96] = "";
		if (r8b_batch_stage_symbol(b, w.first, sym, (int) sizeof(sym)) != 0 || w.second != sym)
		{
			printf("%s: stage %d ran \"%s\", expected \"%s\"\n", name.c_str(), w.first, sym, w.second.c_str());
			bad = 1;
		}
	}
	r8b_batch_delete(b);
	if (!(level > 1e-3)) { printf("%s: no output (peak %g)\n", name.c_str(), level); bad = 1; }
	printf("%s %s: %d calls, %lld outputs per channel, peak %.3g\n", bad ? "FAILED" : "ran", name.c_str(), whole + 2, total, level);
	return bad;
}

} // namespace

int main(int argc, char** argv)
{
	if (argc != 2) { printf("usage: %s TABLE\n", argv[0]); return 2; }
	std::ifstream in(argv[1]);
	if (!in) { printf("cannot read %s\n", argv[1]); return 2; }
	int bad = 0, lines = 0;
	std::string line;
	while (std::getline(in, line))
	{
		if (line.empty() || line[0] == '#') continue;
		lines++;
		bad += run(line);
	}
	printf("%d entries, %d failed\n", lines, bad);
	printf(bad || lines == 0 ? "FAILED\n" : "OK\n");
	return bad || lines == 0 ? 1 : 0;
}
