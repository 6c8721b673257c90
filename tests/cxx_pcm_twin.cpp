// tests/cxx_pcm_twin.cpp -- TEST INFRASTRUCTURE ONLY: the PCM twin of the stage kernels (tests/pcm_twin_cases.py) once under
// AddressSanitizer and UndefinedBehaviorSanitizer on the host (tests/emul/Makefile, target `pcm`: the emulation's sources
// and this file as ONE program, nothing preloaded).
// The emulation's "device memory" is host memory, so the caller's planar PCM buffers are heap blocks here, and they are
// sized to the byte: rows of l elements on a stride of l + 3, the last row without its gap, nothing behind it.  src_load /
// dst_store form byte addresses from an element stride and the format's size; a three-byte row read or written one byte
// past its end is an overrun the sanitizer sees here and no device run can.
//   cxx_pcm_twin TABLE
// TABLE is what `python tests/pcm_twin_cases.py --dump` writes: a line per entry, one per kernel of the twin,
//   what|kind|a|b|c|d|i0|i1|maxin|option=value,...|first stage's symbol|last stage's symbol
// what = "stage": a stand-alone stage object of the descriptor (kind, a, b, c, d, i0, i1); what = "chain": a = src, b = dst,
// c = transition band, d = attenuation.
// For each line and each of the pairs S24 -> S16 and F32 -> S24: a three-channel object (full scale, 2^-10 of full scale,
// silence) and an identical one that is fed the decoded rows as fp64; whole calls of MaxInLen samples until outputs flow
// and two more, then a call of 17 samples and one of a single sample.  Every call returns the fp64 object's count, every
// code is the encoding of the fp64 object's output (round half to even, saturated), the silent channel encodes zeros, no
// side went through the staging rows, and the first and last stage launched the symbols the line names (the emulator's
// launcher reports both forms of the generic convolver as k_conv).
// Exit status 0 and a last line "OK": every entry ran clean.
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

const int kCh = 3;

std::vector<std::string> split(const std::string& s, char sep)
{
	std::vector<std::string> v;
	std::stringstream ss(s);
	std::string f;
	while (std::getline(ss, f, sep)) v.push_back(f);
	if (!s.empty() && s.back() == sep) v.push_back("");
	return v;
}

int bytes_of(int fmt) { return r8b_pcm_sample_bytes(fmt); }

double scale_of(int fmt) { return fmt == R8B_PCM_S16 ? 32768.0 : 8388608.0; }

// the documented convention: rint(v * scale), saturated
long long encode(double v, double scale)
{
	double q = std::nearbyint(v * scale);
	if (q < -scale) q = -scale;
	if (q > scale - 1.0) q = scale - 1.0;
	return (long long) q;
}

long long read_code(const unsigned char* p, int fmt)
{
	if (fmt == R8B_PCM_S16)
	{
		short s;
		memcpy(&s, p, 2);
		return s;
	}
	long long u = (long long) p[0] | ((long long) p[1] << 8) | ((long long) p[2] << 16);
	return u >= (1 << 23) ? u - (1 << 24) : u;
}

CR8BBatch create(const std::vector<std::string>& f, int* bad)
{
	const bool chain = f[0] == "chain";
	const double a = atof(f[2].c_str()), b_ = atof(f[3].c_str()), c = atof(f[4].c_str()), d = atof(f[5].c_str());
	const int kind = atoi(f[1].c_str()), i0 = atoi(f[6].c_str()), i1 = atoi(f[7].c_str()), maxin = atoi(f[8].c_str());
	CR8BBatch b = chain ? r8b_batch_create(a, b_, maxin, c, d, kCh, -1) :
		r8b_batch_create_stage(kind, a, b_, c, d, i0, i1, maxin, kCh, -1);
	if (b == nullptr) { printf("create: %s\n", r8b_last_error()); *bad = 1; return nullptr; }
	for (const std::string& kv : split(f[9], ','))
	{
		const size_t eq = kv.find('=');
		if (eq == std::string::npos || r8b_batch_set_option(b, kv.substr(0, eq).c_str(), atoi(kv.c_str() + eq + 1)) != 0)
		{
			printf("option %s\n", kv.c_str());
			*bad = 1;
		}
	}
	if (r8b_batch_set_option(b, "timing", 1) != 0) *bad = 1;
	return b;
}

int run_pair(const std::vector<std::string>& f, const std::string& name, int fin, int fout)
{
	int bad = 0;
	const int maxin = atoi(f[8].c_str());
	CR8BBatch p = create(f, &bad), d = create(f, &bad);
	if (p == nullptr || d == nullptr) return 1;
	const int cap = r8b_batch_max_out_len(d) > 0 ? r8b_batch_max_out_len(d) : 1;
	const int bi = bytes_of(fin), bo = bytes_of(fout);
	std::vector<double> x((size_t) kCh * maxin), y((size_t) kCh * cap);
	unsigned state = 12345u;
	long long total = 0;
	double level = 0.0;
	int whole = 0, after = 0;
	for (int step = 0; step < 3 && !bad;)
	{
		const int l = step == 0 ? maxin : (step == 1 ? (17 < maxin ? 17 : maxin) : 1);
		// rows of l elements on a stride of l + 3, to the byte
		const size_t in_size = ((size_t) (kCh - 1) * (l + 3) + l) * bi;
		unsigned char* in = (unsigned char*) malloc(in_size);
		memset(in, 0xA5, in_size);
		for (int ch = 0; ch < kCh; ch++)
			for (int k = 0; k < l; k++)
			{
				state = state * 1664525u + 1013904223u;
				unsigned char* at = in + ((size_t) ch * (l + 3) + k) * bi;
				if (fin == R8B_PCM_S24)
				{
					int v = (int) (state >> 8) - (1 << 23);
					v = ch == 0 ? v : (ch == 1 ? v / 1024 : 0);
					at[0] = (unsigned char) (v & 255);
					at[1] = (unsigned char) ((v >> 8) & 255);
					at[2] = (unsigned char) ((v >> 16) & 255);
					x[(size_t) ch * l + k] = (double) v / 8388608.0;
				}
				else
				{
					const double u = (double) (state >> 8) / 8388608.0 - 1.0;
					const float v = (float) (ch == 0 ? u : (ch == 1 ? u / 1024.0 : 0.0));
					memcpy(at, &v, 4);
					x[(size_t) ch * l + k] = (double) v;
				}
			}
		const int n = r8b_batch_process_host(d, x.data(), l, l, y.data(), cap);
		if (n < 0) { printf("%s: process: %s\n", name.c_str(), r8b_last_error()); bad = 1; free(in); break; }
		const size_t out_size = ((size_t) (kCh - 1) * (n + 3) + n) * bo;
		unsigned char* out = (unsigned char*) malloc(out_size);
		memset(out, 0xA5, out_size);
		const int m = r8b_batch_process_pcm(p, in, fin, 0, l + 3, l, out, fout, 0, n + 3, nullptr);
		if (m != n)
		{
			printf("%s: the PCM call returned %d, the fp64 object %d (%s)\n", name.c_str(), m, n, m < 0 ? r8b_last_error() : "");
			bad = 1;
		}
		for (int ch = 0; ch < kCh && !bad; ch++)
		{
			for (int k = 0; k < n; k++)
			{
				const double v = y[(size_t) ch * cap + k];
				const long long got = read_code(out + ((size_t) ch * (n + 3) + k) * bo, fout);
				if (got != encode(v, scale_of(fout)) || (ch == 2 && got != 0))
				{
					printf("%s: channel %d output %lld is code %lld, the fp64 object's %.17g\n", name.c_str(), ch, total + k, got, v);
					bad = 1;
					break;
				}
				if (ch == 0 && std::fabs(v) > level) level = std::fabs(v);
			}
			// the gap between the rows
			for (int k = n * bo; ch + 1 < kCh && k < (n + 3) * bo; k++)
				if (out[(size_t) ch * (n + 3) * bo + k] != 0xA5)
				{
					printf("%s: channel %d: a byte behind the row's %d outputs was written\n", name.c_str(), ch, n);
					bad = 1;
					break;
				}
		}
		free(in);
		free(out);
		total += n;
		if (step == 0)
		{
			whole++;
			if (level > 1e-3) after++;
			if (after >= 3 || whole >= 4096) step++;
		}
		else step++;
	}
	if (r8b_batch_stat(p, "pcm_staged_sides") != 0) { printf("%s: a side went through the staging rows\n", name.c_str()); bad = 1; }
	if (r8b_batch_stat(p, "tail_launches") <= 0) { printf("%s: no k_tail launch\n", name.c_str()); bad = 1; }
	std::string first, last;
	for (int s = 0; s < r8b_batch_stage_count(p); s++)
	{
		char sym[96] = "";
		if (r8b_batch_stage_symbol(p, s, sym, (int) sizeof(sym)) != 0) bad = 1;
		if (sym[0] == 0) continue;
		if (first.empty()) first = sym;
		last = sym;
	}
	auto emulated = [](const std::string& s) { return s == "k_conv_big" ? std::string("k_conv") : s; };
	if (first != emulated(f[10]) || last != emulated(f[11]))
	{
		printf("%s: ran \"%s\" ... \"%s\", expected \"%s\" ... \"%s\"\n", name.c_str(), first.c_str(), last.c_str(), f[10].c_str(), f[11].c_str());
		bad = 1;
	}
	r8b_batch_delete(p);
	r8b_batch_delete(d);
	if (!(level > 1e-3)) { printf("%s: no output (peak %g)\n", name.c_str(), level); bad = 1; }
	printf("%s %s: %d calls, %lld outputs per channel, peak %.3g\n", bad ? "FAILED" : "ran", name.c_str(), whole + 2, total, level);
	return bad;
}

int run(const std::string& line)
{
	const std::vector<std::string> f = split(line, '|');
	if (f.size() != 12) { printf("malformed line: %s\n", line.c_str()); return 1; }
	const std::string name = f[0] + " " + f[1] + " " + f[2] + " " + f[3] + " " + f[5] + " [" + f[9] + "] " + f[10] + " ... " + f[11];
	const int a = run_pair(f, name + " S24->S16", R8B_PCM_S24, R8B_PCM_S16);
	const int b = run_pair(f, name + " F32->S24", R8B_PCM_F32, R8B_PCM_S24);
	return a || b;
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
