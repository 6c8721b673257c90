// tests/cxx_kernel_census.cpp -- TEST INFRASTRUCTURE ONLY: every reachable instance of the compile-time-sized convolver
// kernels (tests/kernel_census.py) once under AddressSanitizer and UndefinedBehaviorSanitizer on the host (tests/emul/
// Makefile, target `census`: the emulation's sources and this file as ONE program, nothing preloaded).
// The emulator allocates a launch's LDS array (LaunchGrid::lds) per launch, and the engine its park and ring buffers per
// object: an instance that indexes past one of them is an overrun the sanitizer sees here, on the CPU.
//   cxx_kernel_census TABLE
// TABLE is what `python tests/kernel_census.py --dump` writes: a line per reachable instance,
//   symbol|src|dst|maxin|tb|atten|phase|stage|option=value,option=value
// For each line: a five-channel object (full scale, 1e-6 of full scale, silence, full scale, and a fifth without a
// partner) with the library's own designer, two calls of MaxInLen samples of noise, then a call of 17 and one of a single
// sample; the symbol the stage ran is read after every call (r8b_batch_stage_symbol names the latest launch) and must
// show up; outputs must be finite and the silent channel exact zeros.  tests/test_kernel_census.py compares samples.
// Exit status 0 and a last line "OK": every chain ran its instance clean.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../include/r8bsrc.h"

namespace {

const int kCh = 5;
const double kLevel[kCh] = { 1.0, 1e-6, 0.0, 1.0, 1.0 };

std::vector<std::string> split(const std::string& s, char sep)
{
	std::vector<std::string> v;
	std::stringstream ss(s);
	std::string f;
	while (std::getline(ss, f, sep)) v.push_back(f);
	return v;
}

int run(const std::string& line)
{
	const std::vector<std::string> f = split(line, '|');
	if (f.size() < 8) { printf("malformed line: %s\n", line.c_str()); return 1; }
	const std::string& symbol = f[0];
	const double src = atof(f[1].c_str()), dst = atof(f[2].c_str()), tb = atof(f[4].c_str()), att = atof(f[5].c_str());
	const int maxin = atoi(f[3].c_str()), phase = atoi(f[6].c_str()), stage = atoi(f[7].c_str());
	CR8BBatch b = r8b_batch_create_ex(src, dst, maxin, tb, att, phase, kCh, -1);
	if (b == nullptr) { printf("%s: create: %s\n", symbol.c_str(), r8b_last_error()); return 1; }
	int bad = 0;
	if (f.size() > 8)
		for (const std::string& kv : split(f[8], ','))
		{
			const size_t eq = kv.find('=');
			if (eq == std::string::npos || r8b_batch_set_option(b, kv.substr(0, eq).c_str(), atoi(kv.c_str() + eq + 1)) != 0)
			{
				printf("%s: option %s\n", symbol.c_str(), kv.c_str());
				bad = 1;
			}
		}
	if (r8b_batch_set_option(b, "timing", 1) != 0) bad = 1;
	const int cap = r8b_batch_max_out_len(b) > 0 ? r8b_batch_max_out_len(b) : 1;
	std::vector<double> x((size_t) kCh * maxin), y((size_t) kCh * cap);
	unsigned state = 12345u;
	bool ran = false;
	long long total = 0;
	double level = 0.0;
	// whole calls until the stage has launched its instance twice over (long chains answer late), then two short ones
	const int lens[4] = { maxin, maxin, 17 < maxin ? 17 : maxin, 1 };
	int whole = 0;
	for (int i = 0; i < 4 && !bad;)
	{
		const int l = lens[i];
		for (int ch = 0; ch < kCh; ch++)
			for (int k = 0; k < l; k++)
			{
				state = state * 1664525u + 1013904223u;
				x[(size_t) ch * l + k] = kLevel[ch] * ((double) (state >> 8) / 8388608.0 - 1.0);
			}
		const int n = r8b_batch_process_host(b, x.data(), l, l, y.data(), cap);
		if (n < 0) { printf("%s: process: %s\n", symbol.c_str(), r8b_last_error()); bad = 1; break; }
		char name[96] = "";
		if (r8b_batch_stage_symbol(b, stage, name, (int) sizeof(name)) != 0) { printf("%s: stage %d\n", symbol.c_str(), stage); bad = 1; break; }
		const bool now = symbol == name;
		for (int ch = 0; ch < kCh; ch++)
			for (int k = 0; k < n; k++)
			{
				const double v = y[(size_t) ch * cap + k];
				if (!(std::fabs(v) < 16.0 * (kLevel[ch] > 0.0 ? kLevel[ch] : 1.0)) || (ch == 2 && v != 0.0))
				{
					printf("%s: channel %d output %lld is %g\n", symbol.c_str(), ch, total + k, v);
					bad = 1;
				}
				if (ch == 0 && std::fabs(v) > level) level = std::fabs(v);
			}
		total += n;
		// (the second whole call is repeated, 64 times at most, until the instance has run and outputs flow)
		ran = ran || now;
		if (i == 1 && !(ran && level > 0.1) && whole < 64) whole++;
		else i++;
	}
	r8b_batch_delete(b);
	if (!ran) { printf("%s: never launched by its chain\n", symbol.c_str()); bad = 1; }
	if (!(level > 0.1)) { printf("%s: no output (peak %g)\n", symbol.c_str(), level); bad = 1; }
	printf("%s %s: %lld outputs per channel, peak %.3f\n", bad ? "FAILED" : "ran", symbol.c_str(), total, level);
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
	printf("%d instances, %d failed\n", lines, bad);
	printf(bad || lines == 0 ? "FAILED\n" : "OK\n");
	return bad || lines == 0 ? 1 : 0;
}
