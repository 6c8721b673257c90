// tests/cxx_conv_tables.cpp -- the convolver's table unit (csrc/r8b_conv_tables.h) on its own: ONE program from
// r8b_conv_tables.cpp, r8b_design.cpp, r8b_plan.cpp and this driver, built with -fsanitize=address,undefined by
// `make tables` of tests/emul/Makefile (tests/test_conv_tables.py runs it).  No engine and no launcher is linked: that it links is the check that the unit is host-only.
//
// The layouts are checked with an index-coded spectrum, H[m] = m: every sum and difference is exact then, and an entry
// names the bins it was made of.  Transform lengths 32, 64 and 256 (NT = 2, 4, 16 threads' worth of entries): the split and
// one-channel builders take the length as a parameter and lay out 16 x n / 16 entries at any n, so the 8192 points they run
// on in the engine add nothing to what a layout can get wrong.  Prints one line per finding and "OK" at the end.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "r8b_conv_tables.h"

using namespace r8bhip;

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_bad++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static int rev(int v, int bits)
{
	int r = 0;
	for (int b = 0; b < bits; b++) r |= ((v >> b) & 1) << (bits - 1 - b);
	return r;
}
static int lg(int n) { int l = 0; while ((1 << l) < n) l++; return l; }

// distance in units of the last place (same sign or zeros; anything else: far)
static long long ulps(double a, double b)
{
	if (a == b) return 0;
	if (std::isnan(a) || std::isnan(b) || (a < 0) != (b < 0)) return 1LL << 62;
	int64_t x, y;
	memcpy(&x, &a, 8);
	memcpy(&y, &b, 8);
	return x > y ? x - y : y - x;
}

// bins 0 .. NH / 2 of an NH-point spectrum: index coded, or smooth values that are no integers
static std::vector<double> spectrum(int NH, bool coded)
{
	std::vector<double> H((size_t) NH / 2 + 1);
	for (int m = 0; m <= NH / 2; m++) H[(size_t) m] = coded ? m : 1.0 / (m + 3.0) - 0.37 * std::sin(0.61 * m);
	return H;
}
static std::vector<double> with_zero_imag(const std::vector<double>& H)
{
	std::vector<double> Hc(H.size() * 2, 0.0);
	for (size_t m = 0; m < H.size(); m++) Hc[m * 2] = H[m];
	return Hc;
}
struct Mirrored
{
	const std::vector<double>& H;
	int NH;
	long double operator()(int m) const { return H[(size_t) (m <= NH / 2 ? m : NH - m)]; }
};
static const long double kPi = 3.14159265358979323846264338327950288L;

// ---- layouts: each real pair_constants* entry against the bin formula of its header comment
static void check_layouts(int N)
{
	const int ln = lg(N), NT = N / 16;
	{
		// 1:1: entry (c, t) = (H[rev(16 t + 2 c)], H[rev(16 t + 2 c + 1)])
		const std::vector<double> H = spectrum(N, true), hp = pair_constants(H, N, N);
		const Mirrored Hm{H, N};
		CHECK(hp.size() == (size_t) 8 * NT * 2, "pair 1:1 size %zu at %d", hp.size(), N);
		for (int t = 0; t < NT; t++)
			for (int c = 0; c < 8; c++)
				for (int j = 0; j < 2; j++)
					CHECK(hp[((size_t) c * NT + t) * 2 + j] == (double) Hm(rev(16 * t + 2 * c + j, ln)), "pair 1:1 (%d, %d)[%d] at %d", c, t, j, N);
	}
	{
		// 2x up: entry (c, t) = (H[k] + H[k + N], H[k] - H[k + N]), k = rev(8 t + c), H over 2 N points, NT = 2 N / 16
		const std::vector<double> H = spectrum(2 * N, true), hp = pair_constants(H, N, 2 * N);
		const Mirrored Hm{H, 2 * N};
		const int NT2 = 2 * N / 16;
		CHECK(hp.size() == (size_t) 8 * NT2 * 2, "pair 2x size %zu at %d", hp.size(), N);
		for (int t = 0; t < NT2; t++)
			for (int c = 0; c < 8; c++)
			{
				const int k = rev(8 * t + c, ln);
				CHECK(hp[((size_t) c * NT2 + t) * 2] == (double) (Hm(k) + Hm(k + N)), "pair 2x sum (%d, %d) at %d", c, t, N);
				CHECK(hp[((size_t) c * NT2 + t) * 2 + 1] == (double) (Hm(k) - Hm(k + N)), "pair 2x difference (%d, %d) at %d", c, t, N);
			}
	}
	for (int D = 2; D <= 4 && N / D >= 16; D *= 2)
	{
		// decimating by D: thread t keeps positions 16 t + 2 D (c' / 2) + (c' odd ? 2 D - 1 : 0); entry (c' / 2, t)[c' & 1]
		const std::vector<double> H = spectrum(N, true), hp = pair_constants(H, N, N / D);
		const Mirrored Hm{H, N};
		CHECK(hp.size() == (size_t) 8 * NT * 2, "pair down size %zu at %d", hp.size(), N);
		std::vector<double> want(hp.size(), 0.0);
		for (int t = 0; t < NT; t++)
			for (int cp = 0; cp < 16 / D; cp++)
				want[((size_t) (cp >> 1) * NT + t) * 2 + (cp & 1)] = (double) Hm(rev(16 * t + 2 * D * (cp >> 1) + ((cp & 1) ? 2 * D - 1 : 0), ln));
		CHECK(hp == want, "pair decimating by %d at %d", D, N);
	}
	{
		// split: entry (c, t) = (H[k] + H[k + N], H[k] - H[k + N]), k = rev(16 t + c); one-channel: (a, b) of the same bins
		const std::vector<double> H = spectrum(2 * N, true), sp = pair_constants_split(H, N), so = pair_constants_solo(H, N);
		const Mirrored Hm{H, 2 * N};
		CHECK(sp.size() == (size_t) 16 * NT * 2 && so.size() == sp.size(), "split / solo size at %d", N);
		for (int t = 0; t < NT; t++)
			for (int c = 0; c < 16; c++)
			{
				const int k = rev(16 * t + c, ln);
				const long double hs = Hm(k) + Hm(k + N), hd = Hm(k) - Hm(k + N), th = kPi * k / N;
				const size_t o = ((size_t) c * NT + t) * 2;
				CHECK(sp[o] == (double) hs && sp[o + 1] == (double) hd, "split (%d, %d) at %d", c, t, N);
				CHECK(ulps(so[o], (double) (hs - hd * sinl(th))) <= 1 && ulps(so[o + 1], (double) (hd * cosl(th))) <= 1, "solo (%d, %d) at %d", c, t, N);
			}
		// one-channel, decimating: c a multiple of down: (H[k], H[n / down - k]); c + 1: (cos, sin) of pi k / n
		for (int down = 2; down <= 4; down *= 2)
		{
			const std::vector<double> sd = pair_constants_solo_down(H, N, down);
			CHECK(sd.size() == (size_t) 16 * NT * 2, "solo down size at %d", N);
			std::vector<double> want(sd.size(), 0.0);
			for (int t = 0; t < NT; t++)
				for (int c = 0; c < 16; c += down)
				{
					const int k = rev(16 * t + c, ln);
					CHECK(k < N / down, "solo down: kept bin %d at %d", k, N);
					want[((size_t) c * NT + t) * 2] = H[(size_t) k];
					want[((size_t) c * NT + t) * 2 + 1] = H[(size_t) (N / down - k)];
					want[((size_t) (c + 1) * NT + t) * 2] = (double) cosl(kPi * k / N);
					want[((size_t) (c + 1) * NT + t) * 2 + 1] = (double) sinl(kPi * k / N);
				}
			for (size_t i = 0; i < sd.size(); i++) CHECK(ulps(sd[i], want[i]) <= 1, "solo down by %d entry %zu at %d", down, i, N);
		}
	}
}

// ---- real against complex forms: a zero imaginary part, entries at the corresponding positions to 1 ulp (both round the
// same long-double quantity).  At these lengths, with the index-coded and with the smooth spectrum, all four pairs -- pair,
// split, solo, solo-down -- turn out exactly equal, 0 ulp apart (the program prints the largest distance of each); the bound
// asserted stays 1 ulp
static long long g_worst[6];
static void same(int which, double got, double want, const char* what, int N)
{
	const long long u = ulps(got, want);
	if (u > g_worst[which]) g_worst[which] = u;
	CHECK(u <= 1, "%s at %d: %.17g against %.17g", what, N, got, want);
}
static void check_real_complex(int N, bool coded)
{
	const int ln = lg(N), NT = N / 16;
	for (int form = 0; form < 4; form++) // the pair: 1:1, 2x up, decimating by 2 and by 4
	{
		const int n_out = form == 0 ? N : (form == 1 ? 2 * N : N / (form == 2 ? 2 : 4));
		if (n_out < 16) continue;
		const int NH = std::max(N, n_out), nt = NH / 16;
		const std::vector<double> H = spectrum(NH, coded), re = pair_constants(H, N, n_out), cx = pair_constants_complex(with_zero_imag(H), N, n_out);
		CHECK(cx.size() == (size_t) 16 * nt * 2, "pair complex size at %d", N);
		for (int t = 0; t < nt; t++)
			for (int c = 0; c < 16; c++)
			{
				const size_t o = ((size_t) c * nt + t) * 2;
				// (2x up: Hs in rows 0 .. 7, Hd in rows 8 .. 15; otherwise row c is value c & 1 of the real row c / 2; the
				// decimating form fills 16 / D rows)
				const double want = form == 1 ? re[((size_t) (c & 7) * nt + t) * 2 + (c >> 3)] : re[((size_t) (c >> 1) * nt + t) * 2 + (c & 1)];
				same(0, cx[o], want, "pair complex", N);
				CHECK(cx[o + 1] == 0.0, "pair complex imaginary part at %d", N);
			}
	}
	const std::vector<double> H = spectrum(2 * N, coded), Hc = with_zero_imag(H);
	const std::vector<double> sp = pair_constants_split(H, N), spc = pair_constants_split_complex(Hc, N);
	const std::vector<double> so = pair_constants_solo(H, N), soc = pair_constants_solo_complex(Hc, N);
	const std::vector<double> sd = pair_constants_solo_down(H, N, 2), sdc = pair_constants_solo_down_complex(Hc, N);
	CHECK(spc.size() == (size_t) 32 * NT * 2 && soc.size() == spc.size() && sdc.size() == (size_t) 24 * NT * 2, "long-block complex sizes at %d", N);
	const Mirrored Hm{H, 2 * N};
	for (int t = 0; t < NT; t++)
		for (int c = 0; c < 16; c++)
		{
			const size_t o = ((size_t) c * NT + t) * 2, o2 = ((size_t) (16 + c) * NT + t) * 2;
			const int k = rev(16 * t + c, ln);
			const long double hd = Hm(k) - Hm(k + N), th = kPi * k / N;
			// split: Hs, then Hd e^{+i pi k / n} -- the real form's Hd turned by the angle
			same(1, spc[o], sp[o], "split complex sum", N);
			CHECK(spc[o + 1] == 0.0, "split complex sum's imaginary part at %d", N);
			same(2, spc[o2], (double) (hd * cosl(th)), "split complex difference (re)", N);
			same(2, spc[o2 + 1], (double) (hd * sinl(th)), "split complex difference (im)", N);
			// one-channel: A = a, B = i b
			same(3, soc[o], so[o], "solo complex A", N);
			CHECK(soc[o + 1] == 0.0 && soc[o2] == 0.0, "solo complex: A real, B imaginary at %d", N);
			same(4, soc[o2 + 1], so[o + 1], "solo complex B", N);
			// one-channel decimating by 2: rows c even and c + 1 as in the real form, row 16 + c / 2 the partner bin
			if ((c & 1) == 0)
			{
				const size_t o3 = ((size_t) (16 + c / 2) * NT + t) * 2, o1 = ((size_t) (c + 1) * NT + t) * 2;
				same(5, sdc[o], sd[o], "solo down complex H[k]", N);
				same(5, sdc[o3], sd[o + 1], "solo down complex H[n / 2 - k]", N);
				same(5, sdc[o1], sd[o1], "solo down complex cos", N);
				same(5, sdc[o1 + 1], sd[o1 + 1], "solo down complex sin", N);
				CHECK(sdc[o + 1] == 0.0 && sdc[o3 + 1] == 0.0, "solo down complex imaginary parts at %d", N);
			}
		}
}

static void check_twiddles()
{
	for (int len = 8; len <= 4096; len *= 2)
	{
		const std::vector<double> t = make_twiddles(len);
		CHECK(t.size() == (size_t) len * 2, "twiddles size at %d", len);
		const double axes[4][2] = { { 1, 0 }, { 0, -1 }, { -1, 0 }, { 0, 1 } }; // exp(-2 pi i e / len) at e = 0, len / 4, ...
		for (int a = 0; a < 4; a++)
			CHECK(t[(size_t) a * (len / 4) * 2] == axes[a][0] && t[(size_t) a * (len / 4) * 2 + 1] == axes[a][1], "twiddles: axis %d at %d", a, len);
		for (int e = 1; e < len; e++)
			CHECK(t[(size_t) (len - e) * 2] == t[(size_t) e * 2] && t[(size_t) (len - e) * 2 + 1] == -t[(size_t) e * 2 + 1], "twiddles: conjugate of %d at %d", e, len);
	}
}

static void check_radices()
{
	for (int bits = 4; bits <= 13; bits++)
		for (int mr = 4; mr <= 16; mr *= 2)
		{
			const std::vector<int> r = plan_radices(1 << bits, mr);
			long long prod = 1;
			for (size_t i = 0; i < r.size(); i++)
			{
				prod *= r[i];
				CHECK((r[i] == 2 || r[i] == 4 || r[i] == 8 || r[i] == 16) && r[i] <= mr, "radix %d of 2^%d under %d", r[i], bits, mr);
				CHECK(i == 0 || r[i] <= r[i - 1], "radices of 2^%d under %d: largest first", bits, mr);
			}
			CHECK(prod == 1LL << bits, "radices of 2^%d under %d: product %lld", bits, mr, prod);
		}
}

// the whole-step interpolator of the chain src -> dst (its last stage)
static StagePlan whole_stage(double src, double dst, double atten)
{
	ChainPlan p;
	p.init(build_topology(src, dst, 2.0, atten), 1024);
	const StagePlan& w = p.stages.back();
	CHECK(w.desc.kind == kFrac && w.whole, "%g -> %g: no whole-step interpolator at the end", src, dst);
	return w;
}

static void check_whole_step_rows()
{
	const StagePlan w = whole_stage(48000.0, 47000.0, 100.0); // 96 : 47, 14 taps
	const std::vector<double> rows = whole_step_rows(w);
	const std::vector<double>& bank = w.bank->table;
	CHECK(w.in_step == 96 && w.out_step == 47, "48000 -> 47000 steps %d : %d", w.in_step, w.out_step);
	CHECK(rows.size() == (size_t) w.flen * w.out_step, "whole-step rows size");
	for (int r = 0; r < w.out_step; r++)
		for (int i = 0; i < w.flen; i++)
			CHECK(rows[(size_t) i * w.out_step + r] == bank[(size_t) ((long long) r * w.in_step % w.out_step) * w.flen + i], "whole-step row %d tap %d", r, i);
}

static int lane_deals_cached()
{
	int counts[3];
	design_cache_counts(counts);
	return counts[2];
}

static void check_two_phase(double src, double dst, int In, int Out)
{
	const StagePlan w = whole_stage(src, dst, 180.15);
	CHECK(w.in_step == In && w.out_step == Out && w.flen <= 24, "%g -> %g: %d : %d, %d taps", src, dst, w.in_step, w.out_step, w.flen);
	const int before = lane_deals_cached();
	const std::optional<TwoPhaseTables> first = two_phase_tables(w);
	CHECK(first.has_value(), "%d : %d has no two-phase tables", In, Out);
	if (!first) return;
	CHECK(lane_deals_cached() == before + 1, "%d : %d: the search left no cache entry", In, Out);
	const std::optional<TwoPhaseTables> again = two_phase_tables(w);
	CHECK(lane_deals_cached() == before + 1, "%d : %d: the second call searched again", In, Out);
	CHECK(again && again->ptab == first->ptab && again->ctab == first->ctab && again->nsets == first->nsets && again->taps2 == first->taps2,
		"%d : %d: the cached call differs", In, Out);
	const TwoPhaseTables& T = *first;
	const int NP = (Out + 1) / 2, ctp = (NP + 3) & ~3;
	auto r_of = [&](int ph) { return (int) ((long long) ph * In / Out); };
	int maxdl = 0;
	for (int q = 0; 2 * q + 1 < Out; q++) maxdl = std::max(maxdl, r_of(2 * q + 1) - r_of(2 * q));
	CHECK((T.taps2 == 25) == (maxdl <= 1) && (T.taps2 == 25 || T.taps2 == 27), "%d : %d: taps2 %d with window starts %d apart", In, Out, T.taps2, maxdl);
	CHECK(T.nsets == 16 / ((NP + 15) / 16), "%d : %d: nsets %d", In, Out, T.nsets);
	// every phase pair once per set; each entry q | set << 8 | floor(2 q In / Out) << 12
	CHECK(T.ptab.size() == 256, "ptab size");
	std::map<std::pair<int, int>, int> seen;
	for (int e : T.ptab)
	{
		if (e < 0) { CHECK(e == -1, "ptab: idle entry %d", e); continue; }
		const int q = e & 255, set = (e >> 8) & 15;
		CHECK(q < NP && set < T.nsets && (e >> 12) == r_of(2 * q), "ptab entry %#x of %d : %d", (unsigned) e, In, Out);
		seen[std::make_pair(q, set)]++;
	}
	CHECK(seen.size() == (size_t) NP * T.nsets, "%d : %d: %zu (pair, set) entries", In, Out, seen.size());
	for (const auto& s : seen) CHECK(s.second == 1, "%d : %d: pair %d of set %d %d times", In, Out, s.first.first, s.first.second, s.second);
	// ctab: value v of pair q at ((v / 2) ctp + q) 2 + v % 2 -- the taps of phase 2 q, then, from taps2 + its window offset on,
	// those of phase 2 q + 1; zero everywhere else
	const std::vector<double>& bank = w.bank->table;
	std::vector<double> want((size_t) 2 * T.taps2 * ctp, 0.0);
	for (int q = 0; q < NP; q++)
		for (int ph = 2 * q; ph <= 2 * q + 1 && ph < Out; ph++)
			for (int i = 0; i < w.flen; i++)
			{
				const int v = ph == 2 * q ? i : T.taps2 + i + r_of(ph) - r_of(2 * q);
				want[((size_t) (v / 2) * ctp + q) * 2 + (v & 1)] = bank[(size_t) ((long long) ph * In % Out) * w.flen + i];
			}
	CHECK(T.ctab == want, "%d : %d: ctab", In, Out);
}

int main()
{
	for (int N : { 32, 64, 256 })
	{
		check_layouts(N);
		check_real_complex(N, true);
		check_real_complex(N, false);
	}
	static const char* const names[6] = { "pair", "split sum", "split difference", "solo A", "solo B", "solo down" };
	for (int i = 0; i < 6; i++) printf("real against complex, %s: at most %lld ulp apart\n", names[i], g_worst[i]);
	check_twiddles();
	check_radices();
	check_whole_step_rows();
	check_two_phase(44100.0, 96000.0, 147, 160);
	check_two_phase(48000.0, 44100.0, 320, 147); // (In > Out: window starts up to three samples apart, 27-entry rows)
	CHECK(!two_phase_tables(whole_stage(8000.0, 8190.0, 180.15)), "819 phases have two-phase tables");
	CHECK(!two_phase_tables(whole_stage(44100.0, 96000.0, 206.91)), "28 taps have two-phase tables");
	if (g_bad) { printf("%d checks failed\n", g_bad); return 1; }
	printf("OK\n");
	return 0;
}
