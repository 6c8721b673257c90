// r8b_conv_tables.cpp -- see r8b_conv_tables.h.  Host arithmetic only: compiled with the host flags of the Makefile, whose
// -ffp-contract=off keeps every table the same bits whatever surrounds an expression.  The library gets this unit through
// r8b_engine.cpp, which includes it at its end (no build file lists it); the table test compiles it by itself.
#include "r8b_conv_tables.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <list>
#include <mutex>
#include <stdexcept>
#include <utility>

// (for the geometry predicates conv*_ok alone: no launcher and no dev_* function is called from this unit)
#include "r8b_launch.h"

namespace r8bhip {

namespace {

typedef std::complex<long double> C;

// the `bits` low bits of v in reverse order (the one bit reversal of the host code)
int bit_reverse(int v, int bits)
{
	int r = 0;
	for (int b = 0; b < bits; b++)
		if (v & (1 << b)) r |= 1 << (bits - 1 - b);
	return r;
}

// the smallest l with 2^l >= n
int log2_ceil(int n)
{
	int l = 0;
	while ((1 << l) < n) l++;
	return l;
}

// bin m, 0 <= m < NH, of a real spectrum of NH points stored as its bins 0 .. NH / 2: mirrored above
struct MirroredSpectrum
{
	const std::vector<double>& H;
	int NH;
	long double operator()(int m) const { return H[(size_t) (m <= NH / 2 ? m : NH - m)]; }
};

// bin m (mod NH) of a complex spectrum of NH points stored as its bins 0 .. NH / 2, interleaved: Hermitian above
struct HermitianSpectrum
{
	const std::vector<double>& Hc;
	int NH;
	C operator()(int m) const
	{
		m &= NH - 1;
		if (m <= NH / 2) return C(Hc[(size_t) m * 2], Hc[(size_t) m * 2 + 1]);
		return std::conj(C(Hc[(size_t) (NH - m) * 2], Hc[(size_t) (NH - m) * 2 + 1]));
	}
};

// complex entry (row, t) of a table of rows of `pitch` entries, interleaved (re, im)
void put_complex(std::vector<double>& out, int pitch, int row, int t, C v)
{
	out[((size_t) row * pitch + t) * 2] = (double) v.real();
	out[((size_t) row * pitch + t) * 2 + 1] = (double) v.imag();
}

const long double kPi = 3.14159265358979323846264338327950288L;

} // namespace

std::vector<double> make_twiddles(int len)
{
	std::vector<double> t((size_t) len * 2);
	const long double two_pi = 6.283185307179586476925286766559L;
	const int quarter = len / 4;
	for (int e = 0; e < len; e++)
	{
		double c, s;
		if (quarter > 0 && len % 4 == 0)
		{
			const int quad = e / quarter, rem = e - quad * quarter;
			long double c0 = 1.0L, s0 = 0.0L;
			if (rem != 0)
			{
				// evaluate in the first octant pair and reflect for accuracy/symmetry
				if (2 * rem <= quarter)
				{
					c0 = cosl(two_pi * rem / len);
					s0 = sinl(two_pi * rem / len);
				}
				else
				{
					const int r2 = quarter - rem;
					c0 = sinl(two_pi * r2 / len);
					s0 = cosl(two_pi * r2 / len);
				}
			}
			switch (quad)
			{
			case 0: c = (double) c0; s = (double) s0; break;
			case 1: c = (double) -s0; s = (double) c0; break;
			case 2: c = (double) -c0; s = (double) -s0; break;
			default: c = (double) s0; s = (double) -c0; break;
			}
		}
		else
		{
			c = (double) cosl(two_pi * e / len);
			s = (double) sinl(two_pi * e / len);
		}
		t[(size_t) e * 2] = c;
		t[(size_t) e * 2 + 1] = -s;
	}
	return t;
}

std::vector<double> kernel_spectrum(const LpFilter& f, int bl2, double scale)
{
	const std::vector<double> tw = make_twiddles(bl2);
	std::vector<double> H((size_t) bl2 / 2 + 1);
	const double* c = &f.taps[(size_t) f.fl2];
	for (int m = 0; m <= bl2 / 2; m++)
	{
		long double acc = c[0];
		for (int t = 1; t <= f.fl2; t++)
		{
			const int e = (int) (((long long) m * t) & (bl2 - 1));
			acc += 2.0L * c[t] * tw[(size_t) e * 2];
		}
		H[(size_t) m] = (double) (acc * scale);
	}
	return H;
}

std::vector<double> kernel_spectrum_complex(const LpFilter& f, int bl2, int align, double scale)
{
	const std::vector<double> tw = make_twiddles(bl2);
	std::vector<double> H((size_t) (bl2 / 2 + 1) * 2);
	const int K = (int) f.taps.size();
	for (int m = 0; m <= bl2 / 2; m++)
	{
		long double re = 0.0L, im = 0.0L;
		for (int n = 0; n < K; n++)
		{
			const long long e = ((long long) m * (n - align)) & (bl2 - 1);
			re += (long double) f.taps[(size_t) n] * tw[(size_t) e * 2];
			im += (long double) f.taps[(size_t) n] * tw[(size_t) e * 2 + 1];
		}
		H[(size_t) m * 2] = (double) (re * scale);
		H[(size_t) m * 2 + 1] = (double) (im * scale);
	}
	return H;
}

// the bin of a slot of the one-channel kernel's spectral stage over an N-point complex transform, and back: slot s < N / 2
// holds bin bitrev(s) over log2(N) - 1 bits, slot N / 2 bin N / 2
static int slot_bin(int slot, int N)
{
	return slot < N / 2 ? bit_reverse(slot, log2_ceil(N) - 1) : N / 2;
}

std::vector<double> spectral_constants(const std::vector<double>& H, const std::vector<double>& tw,
	int bl2, int n_in, int up)
{
	const int N = n_in / 2, N2 = N * up;
	const int slots = N / 2 + 1;
	const int nconst = up == 1 ? 4 : 8;
	std::vector<double> out((size_t) nconst * slots * 2, 0.0);
	auto W = [&](long long e) // exp(-2 pi i e / bl2)
	{
		e &= bl2 - 1;
		return C(tw[(size_t) e * 2], tw[(size_t) e * 2 + 1]);
	};
	auto put = [&](int c, int slot, C v) { put_complex(out, slots, c, slot, v); };
	const C I(0.0L, 1.0L);
	const int tsf = bl2 / (2 * N), tsh = bl2 / (2 * N2);
	for (int slot = 0; slot < slots; slot++)
	{
		const int kf = slot_bin(slot, N);
		// R[kf] = A Z1 + B conj(Z2),  R[N-kf] = conj(B) conj(Z1) + conj(A) Z2
		const C w = W((long long) kf * tsf);
		const C A = 0.5L * (C(1.0L) - I * w), B = 0.5L * (C(1.0L) + I * w);
		auto cw = [&](int k) { return std::conj(W((long long) k * tsh)); }; // conj(w_{2 N2}^k)
		if (up == 1)
		{
			const long double ha = H[(size_t) kf], hb = H[(size_t) (N - kf)];
			// Z'[kf] = ha (1 + i cw) R + hb (1 - i cw) conj(R[N-kf])
			C f = ha * (C(1.0L) + I * cw(kf)), g = hb * (C(1.0L) - I * cw(kf));
			put(0, slot, f * A + g * B);
			put(1, slot, f * B + g * A);
			// Z'[N-kf] = hb (1 + i cw2) R[N-kf] + ha (1 - i cw2) conj(R)
			f = hb * (C(1.0L) + I * cw(N - kf));
			g = ha * (C(1.0L) - I * cw(N - kf));
			put(2, slot, f * std::conj(B) + g * std::conj(A));
			put(3, slot, f * std::conj(A) + g * std::conj(B));
		}
		else
		{
			// zero-stuffed spectrum: bins kf / 2N-kf carry R / conj R, bins N-kf / N+kf carry
			// R[N-kf] / its conjugate
			long double ha = H[(size_t) kf], hb = H[(size_t) (2 * N - kf)];
			C c1 = C(ha + hb) + I * cw(kf) * C(ha - hb);
			put(0, slot, c1 * A);
			put(1, slot, c1 * B);
			C d1 = C(hb + ha) + I * cw(2 * N - kf) * C(hb - ha);
			put(2, slot, d1 * std::conj(A));
			put(3, slot, d1 * std::conj(B));
			if (kf != 0)
			{
				ha = H[(size_t) (N - kf)];
				hb = H[(size_t) (N + kf)];
				C c2 = C(ha + hb) + I * cw(N - kf) * C(ha - hb);
				put(4, slot, c2 * std::conj(B));
				put(5, slot, c2 * std::conj(A));
				C d2 = C(hb + ha) + I * cw(N + kf) * C(hb - ha);
				put(6, slot, d2 * B);
				put(7, slot, d2 * A);
			}
			else
			{
				// bin N is its own partner: Z'[N] = 2 H[N] R[N]
				const C c2 = C(2.0L * H[(size_t) N]);
				put(4, slot, c2 * std::conj(B));
				put(5, slot, c2 * std::conj(A));
			}
		}
	}
	return out;
}

std::vector<double> spectral_constants_down(const std::vector<double>& H,
	const std::vector<double>& tw, int bl2, int n_in, int down)
{
	const int N = n_in / 2, N2 = N / down;
	const int slots = N2 / 2 + 1;
	std::vector<double> out((size_t) 8 * slots * 2, 0.0);
	const C I(0.0L, 1.0L);
	auto W = [&](long long e) // exp(-2 pi i e / bl2)
	{
		e &= bl2 - 1;
		return C(tw[(size_t) e * 2], tw[(size_t) e * 2 + 1]);
	};
	long double hmax = 0.0L;
	for (double h : H) hmax = std::max(hmax, (long double) std::fabs(h));
	for (int slot = 0; slot < slots; slot++)
	{
		const int k = slot_bin(slot, N2);
		const int idx[4] = { k, (N - k) & (N - 1), N2 - k, (N - N2 + k) & (N - 1) };
		// the model, with the forward transform being zero except Z[pe] = pv
		int pe = 0;
		C pv;
		auto Z = [&](int j) { return j == pe ? pv : C(0.0L); };
		auto X = [&](int m) // bin m of the bl2-point real spectrum, 0 <= m <= N
		{
			const C z1 = Z(m & (N - 1)), z2 = std::conj(Z((N - m) & (N - 1)));
			return 0.5L * (z1 + z2) + W((long long) m * (bl2 / (2 * N))) * ((z1 - z2) / (2.0L * I));
		};
		auto Y = [&](int m) // product spectrum handed to the backward transform, 0 <= m <= N2
		{
			const C x = X(m);
			if (m == N2) return C((long double) H[(size_t) m] * (x.real() + x.imag()));
			return (long double) H[(size_t) m] * x;
		};
		auto Zp = [&](int m) // packed input m of the N2-point backward transform
		{
			const C sa = Y(m), sb = std::conj(Y(N2 - m));
			return (sa + sb) + I * std::conj(W((long long) m * (bl2 / (2 * N2)))) * (sa - sb);
		};
		const int nout = k != 0 && k != N2 / 2 ? 2 : 1;
		for (int o = 0; o < nout; o++)
		{
			const int m = o == 0 ? k : N2 - k;
			for (int u = 0; u < 4; u++)
			{
				bool seen = false;
				for (int v = 0; v < u; v++) seen = seen || idx[v] == idx[u];
				if (seen) continue;
				pe = idx[u];
				pv = C(1.0L);
				const C f1 = Zp(m);
				pv = I;
				const C fi = Zp(m);
				const C coef[2] = { 0.5L * (f1 - I * fi), 0.5L * (f1 + I * fi) }; // plain, conj
				for (int cj = 0; cj < 2; cj++)
				{
					if (std::abs(coef[cj]) <= 1e-19L * hmax) continue;
					// where does element idx[u] appear plain (cj = 0) / conjugated (cj = 1)?
					// form 1: plain at positions 0, 3; form 2: plain at positions 1, 2
					int where = -1;
					for (int form = 0; form < 2 && where < 0; form++)
					{
						if (k != 0 && form != o) continue;
						for (int pos = 0; pos < 4 && where < 0; pos++)
						{
							const bool plain = form == 0 ? (pos == 0 || pos == 3) :
								(pos == 1 || pos == 2);
							if (idx[pos] == idx[u] && plain == (cj == 0)) where = form * 4 + pos;
						}
					}
					if (where < 0)
						throw std::logic_error("spectral_constants_down: term does not fit");
					put_complex(out, slots, where, slot, coef[cj]);
				}
			}
		}
	}
	return out;
}

// Backward bin k = ca(k) Z[k mod N] + cb(k) conj(Z[-k mod N]): (ca, cb) of bin k out of the per-slot table `sc`
// (spectral_constants, up 1 or 2)
static void bin_constants(const std::vector<double>& sc, int N, int up, int k, double* ca, double* cb)
{
	const int slots = N / 2 + 1;
	// (the slot of a bin: the reversal is its own inverse)
	auto slot_of = [&](int kf) { return slot_bin(kf, N); };
	int a, b, kf;
	if (up == 1)
	{
		if (k <= N / 2) { kf = k; a = 0; b = 1; }
		else { kf = N - k; a = 3; b = 2; }
	}
	else
	{
		if (k <= N / 2) { kf = k; a = 0; b = 1; }
		else if (k <= N) { kf = N - k; a = 5; b = 4; }
		else if (k < N + N / 2) { kf = k - N; a = 6; b = 7; }
		else { kf = 2 * N - k; a = 3; b = 2; }
	}
	const size_t ia = ((size_t) a * slots + slot_of(kf)) * 2, ib = ((size_t) b * slots + slot_of(kf)) * 2;
	ca[0] = sc[ia]; ca[1] = sc[ia + 1];
	cb[0] = sc[ib]; cb[1] = sc[ib + 1];
}

std::vector<double> spectral_constants_by_position(const std::vector<double>& sc, int n_in, int up)
{
	const int N = n_in / 2, N2 = N * up;
	const int logn2 = log2_ceil(N2);
	std::vector<double> out((size_t) N2 * 2 * 2, 0.0);
	for (int P = 0; P < N2; P++)
		bin_constants(sc, N, up, bit_reverse(P, logn2), &out[(size_t) P * 2], &out[((size_t) N2 + P) * 2]);
	return out;
}

std::vector<double> pair_constants(const std::vector<double>& H, int n_in, int n_out)
{
	const int N = n_in, N2 = n_out, NT = std::max(N, N2) / 16;
	const int ln = log2_ceil(N);
	const MirroredSpectrum Hf{H, std::max(N, N2)};
	std::vector<double> out((size_t) 8 * NT * 2, 0.0);
	if (N2 < N)
	{
		const int D = N / N2, E2 = 16 / D;
		for (int t = 0; t < NT; t++)
			for (int cp = 0; cp < E2; cp++)
			{
				const int p = 16 * t + 2 * D * (cp >> 1) + ((cp & 1) ? 2 * D - 1 : 0);
				out[((size_t) (cp >> 1) * NT + t) * 2 + (cp & 1)] = (double) Hf(bit_reverse(p, ln));
			}
		return out;
	}
	const int up = N2 / N;
	for (int t = 0; t < NT; t++)
		for (int c = 0; c < 8; c++)
		{
			double* o = &out[((size_t) c * NT + t) * 2];
			if (up == 2)
			{
				const int k = bit_reverse(8 * t + c, ln);
				o[0] = (double) (Hf(k) + Hf(k + N));
				o[1] = (double) (Hf(k) - Hf(k + N));
			}
			else
			{
				o[0] = (double) Hf(bit_reverse(16 * t + 2 * c, ln));
				o[1] = (double) Hf(bit_reverse(16 * t + 2 * c + 1, ln));
			}
		}
	return out;
}

std::vector<double> pair_constants_split(const std::vector<double>& H, int n_in)
{
	const int N = n_in, NT = N / 16;
	const int ln = log2_ceil(N);
	const MirroredSpectrum Hf{H, 2 * N};
	std::vector<double> out((size_t) 16 * NT * 2, 0.0);
	for (int t = 0; t < NT; t++)
		for (int c = 0; c < 16; c++)
		{
			const int k = bit_reverse(16 * t + c, ln);
			out[((size_t) c * NT + t) * 2] = (double) (Hf(k) + Hf(k + N));
			out[((size_t) c * NT + t) * 2 + 1] = (double) (Hf(k) - Hf(k + N));
		}
	return out;
}

std::vector<double> pair_constants_solo(const std::vector<double>& H, int n)
{
	const int N = n, NT = N / 16;
	const int ln = log2_ceil(N);
	const MirroredSpectrum Hf{H, 2 * N};
	const long double pi = kPi;
	std::vector<double> out((size_t) 16 * NT * 2, 0.0);
	for (int t = 0; t < NT; t++)
		for (int c = 0; c < 16; c++)
		{
			const int k = bit_reverse(16 * t + c, ln);
			const long double hs = Hf(k) + Hf(k + N), hd = Hf(k) - Hf(k + N), th = pi * k / N;
			out[((size_t) c * NT + t) * 2] = (double) (hs - hd * sinl(th));
			out[((size_t) c * NT + t) * 2 + 1] = (double) (hd * cosl(th));
		}
	return out;
}

std::vector<double> pair_constants_solo_down(const std::vector<double>& H, int n, int down)
{
	const int N = n, NT = N / 16, N2 = N / down;
	const int ln = log2_ceil(N);
	const long double pi = kPi;
	std::vector<double> out((size_t) 16 * NT * 2, 0.0);
	for (int t = 0; t < NT; t++)
		for (int c = 0; c < 16; c += down)
		{
			const int k = bit_reverse(16 * t + c, ln); // (< N2: the lowest bits of c are the highest of k)
			const long double th = pi * k / N;
			out[((size_t) c * NT + t) * 2] = H[(size_t) k];
			out[((size_t) c * NT + t) * 2 + 1] = H[(size_t) (N2 - k)];
			out[((size_t) (c + 1) * NT + t) * 2] = (double) cosl(th);
			out[((size_t) (c + 1) * NT + t) * 2 + 1] = (double) sinl(th);
		}
	return out;
}

static std::vector<double> long_block_constants_complex(const std::vector<double>& Hc, int n, bool solo)
{
	const int N = n, NT = N / 16;
	const int ln = log2_ceil(N);
	const HermitianSpectrum Hf{Hc, 2 * N};
	const long double pi = kPi;
	std::vector<double> out((size_t) 32 * NT * 2, 0.0);
	auto put = [&](int row, int t, C v) { put_complex(out, NT, row, t, v); };
	for (int t = 0; t < NT; t++)
		for (int c = 0; c < 16; c++)
		{
			const int k = bit_reverse(16 * t + c, ln);
			const C hs = Hf(k) + Hf(k + N), hd = Hf(k) - Hf(k + N);
			const long double th = pi * k / N;
			if (solo)
			{
				put(c, t, hs - hd * sinl(th));
				put(16 + c, t, C(0.0L, 1.0L) * hd * cosl(th));
			}
			else
			{
				put(c, t, hs);
				put(16 + c, t, hd * C(cosl(th), sinl(th)));
			}
		}
	return out;
}
std::vector<double> pair_constants_solo_down_complex(const std::vector<double>& Hc, int n)
{
	const int N = n, NT = N / 16, N2 = N / 2;
	const int ln = log2_ceil(N);
	const long double pi = kPi;
	std::vector<double> out((size_t) 24 * NT * 2, 0.0);
	for (int t = 0; t < NT; t++)
		for (int c = 0; c < 16; c += 2)
		{
			const int k = bit_reverse(16 * t + c, ln), j = N2 - k; // (0 <= k < N2: both bins inside the stored half)
			const long double th = pi * k / N;
			out[((size_t) c * NT + t) * 2] = Hc[(size_t) k * 2];
			out[((size_t) c * NT + t) * 2 + 1] = Hc[(size_t) k * 2 + 1];
			out[((size_t) (c + 1) * NT + t) * 2] = (double) cosl(th);
			out[((size_t) (c + 1) * NT + t) * 2 + 1] = (double) sinl(th);
			out[((size_t) (16 + c / 2) * NT + t) * 2] = Hc[(size_t) j * 2];
			out[((size_t) (16 + c / 2) * NT + t) * 2 + 1] = Hc[(size_t) j * 2 + 1];
		}
	return out;
}
std::vector<double> pair_constants_split_complex(const std::vector<double>& Hc, int n)
{
	return long_block_constants_complex(Hc, n, false);
}
std::vector<double> pair_constants_solo_complex(const std::vector<double>& Hc, int n)
{
	return long_block_constants_complex(Hc, n, true);
}

std::vector<double> pair_constants_complex(const std::vector<double>& Hc, int n_in, int n_out)
{
	const int N = n_in, N2 = n_out, NT = std::max(N, N2) / 16;
	const int ln = log2_ceil(N);
	const HermitianSpectrum Hf{Hc, std::max(N, N2)};
	std::vector<double> out((size_t) 16 * NT * 2, 0.0);
	auto put = [&](int c, int t, C v) { put_complex(out, NT, c, t, v); };
	for (int t = 0; t < NT; t++)
	{
		if (N2 < N)
		{
			const int D = N / N2, E2 = 16 / D;
			for (int cp = 0; cp < E2; cp++)
				put(cp, t, Hf(bit_reverse(16 * t + 2 * D * (cp >> 1) + ((cp & 1) ? 2 * D - 1 : 0), ln)));
		}
		else if (N2 == 2 * N)
		{
			for (int c = 0; c < 8; c++)
			{
				const int k = bit_reverse(8 * t + c, ln);
				put(c, t, Hf(k) + Hf(k + N));
				put(c + 8, t, Hf(k) - Hf(k + N));
			}
		}
		else
			for (int c = 0; c < 16; c++) put(c, t, Hf(bit_reverse(16 * t + c, ln)));
	}
	return out;
}

std::vector<double> pair_constants_poly3(const LpFilter& f, int fl2, int N, int a, int b)
{
	const int NT = N / 16, K = (int) f.taps.size();
	const int ln = log2_ceil(N);
	const std::vector<double> tw = make_twiddles(N); // exp(-2 pi i e / N)
	std::vector<double> out((size_t) 3 * 16 * NT * 2, 0.0);
	for (int r = 0; r < 3; r++)
	{
		// (the component's taps with their circular positions)
		std::vector<std::pair<int, double>> taps;
		for (int d = -a; d <= b; d++)
		{
			const long long i = 3LL * d + r + fl2;
			if (i >= 0 && i < K) taps.emplace_back(((d - b) % N + N) % N, f.taps[(size_t) i]);
		}
		std::vector<long double> Gr((size_t) N), Gi((size_t) N);
		for (int k = 0; k <= N / 2; k++)
		{
			long double re = 0.0L, im = 0.0L;
			for (const auto& t : taps)
			{
				const long long e = ((long long) k * t.first) & (N - 1);
				re += (long double) t.second * tw[(size_t) e * 2];
				im += (long double) t.second * tw[(size_t) e * 2 + 1];
			}
			Gr[(size_t) k] = re / N;
			Gi[(size_t) k] = im / N;
			if (k > 0 && k < N / 2)
			{
				Gr[(size_t) (N - k)] = re / N;
				Gi[(size_t) (N - k)] = -im / N;
			}
		}
		for (int t = 0; t < NT; t++)
			for (int c = 0; c < 16; c++)
			{
				const int k = bit_reverse(16 * t + c, ln);
				const size_t o = (((size_t) r * 16 + c) * NT + t) * 2;
				out[o] = (double) Gr[(size_t) k];
				out[o + 1] = (double) Gi[(size_t) k];
			}
	}
	return out;
}

std::vector<double> pair_twiddles(const std::vector<double>& tw, int tw_len, int n_in, int n_out)
{
	const int NT = std::max(n_in, n_out) / 16, e1 = n_in / NT, e2 = n_out / NT;
	const bool dec = n_out < n_in || n_out > 4096; // (the mirrored backward side: decimating, or 8192 points)
	int npost = 0, rmb = 1;
	if (dec)
	{
		const int ln2 = log2_ceil(n_out), eb2 = log2_ceil(e2);
		npost = (ln2 - 1) / eb2;
		rmb = 1 << (ln2 - npost * eb2);
	}
	const int r2 = n_out >= 256 ? n_out / 256 : n_out / 16;
	const int nb2 = r2 > 1 ? 16 / r2 : 0;
	const int nslots = dec ? 3 + npost : 4 + nb2;
	std::vector<double> out((size_t) nslots * 6 * NT * 2, 0.0);
	static const int mult[6] = { 1, 2, 3, 4, 8, 12 };
	for (int slot = 0; slot < nslots; slot++)
	{
		int n, jmod, joff = 0;
		if (slot < 3)
		{
			n = n_in;
			for (int i = 0; i < slot; i++) n /= e1;
			jmod = n / e1; // butterflies per sub-transform
			if (n < 2 * e1) continue;
		}
		else if (dec)
		{
			n = rmb;
			for (int i = 0; i < slot - 2; i++) n *= e2;
			jmod = n / e2;
		}
		else if (slot == 3)
		{
			if (n_out < 256) continue;
			n = 256; jmod = 16;
		}
		else { n = n_out; jmod = n_out; joff = NT * (slot - 4); }
		for (int t = 0; t < NT; t++)
			for (int c = 0; c < 6; c++)
			{
				const long long j = (t % jmod) + joff;
				const long long e = (long long) (tw_len / n) * j * mult[c];
				const size_t o = (((size_t) slot * 6 + c) * NT + t) * 2, i = (size_t) (e % tw_len) * 2;
				out[o] = tw[i];
				out[o + 1] = tw[i + 1];
			}
	}
	return out;
}

std::vector<int> plan_radices(int N, int max_radix)
{
	std::vector<int> r;
	if (max_radix < 2) max_radix = 2;
	if (max_radix > 16) max_radix = 16;
	const int bits = log2_ceil(N);
	int mb = 0;
	while ((2 << mb) <= max_radix) mb++;
	// spread the bits as evenly as possible over the fewest passes
	const int np = (bits + mb - 1) / mb;
	for (int i = 0; i < np; i++)
	{
		const int b = (bits + np - 1 - i) / np;
		r.push_back(1 << b);
	}
	return r;
}

bool convx_edge3(const ConvGeom& g) { return convx_mode3_ok(g.n_in, g.n_out, g.up, g.down, g.up_pow2, g.down_pow2); }
bool convx_plain(const ConvGeom& g) { return convx_geometry_ok(g.n_in, g.n_out, g.up, g.down, g.up_pow2); }
bool pair_plain(const ConvGeom& g) { return convp_geometry_ok(g.n_in, g.n_out, g.up, g.down, g.up_pow2); }
bool pair_edge3(const ConvGeom& g) { return convp_mode3_ok(g.n_in, g.n_out, g.up, g.down, g.up_pow2, g.down_pow2); }
PairTables pair_tables(const ConvGeom& g)
{
	if ((!g.complex_h || g.down == 2) && convp_solo_down_ok(g.n_in, g.n_out, g.up, g.down, g.up_pow2, g.down_pow2, g.in_len))
		return kTabSoloDown;
	if (convp_solo_ok(g.n_in, g.n_out, g.up, g.down, g.up_pow2, g.down_pow2, g.in_len)) return kTabSolo;
	if (convp_split_ok(g.n_in, g.n_out, g.up, g.down, g.up_pow2, g.down_pow2)) return kTabSplit;
	return pair_plain(g) || pair_edge3(g) ? kTabPair : kTabNone;
}

ConvTables conv_tables(const StagePlan& sp)
{
	const ConvGeom& g = sp.cg;
	ConvTables T;
	if (g.p3)
	{
		T.hp3 = pair_constants_poly3(*sp.lp, g.fl2, g.p3_n, g.p3_a, g.p3_b);
		T.ptw3 = pair_twiddles(make_twiddles(g.p3_n), g.p3_n, g.p3_n, g.p3_n);
	}
	std::vector<double>& H = g.complex_h ? T.Hc : T.H;
	H = g.complex_h ? kernel_spectrum_complex(*sp.lp, g.bl2, g.fl2, 1.0 / g.bl2) : kernel_spectrum(*sp.lp, g.bl2, 1.0 / g.bl2);
	T.tw = make_twiddles(g.bl2);
	if ((convx_edge3(g) || convx_plain(g)) && !g.complex_h)
	{
		// (3x zero stuffing / 3x strided decimation are 1:1 for the transforms)
		const int eup = g.up_pow2 ? g.up : 1, edown = g.down_pow2 ? g.down : 1;
		T.spec = edown > 1 ? spectral_constants_down(H, T.tw, g.bl2, g.n_in, edown) :
			spectral_constants(H, T.tw, g.bl2, g.n_in, eup);
		if (edown == 1) T.spec2 = spectral_constants_by_position(T.spec, g.n_in, eup);
	}
	// the pair kernel's constants per forward position and the passes of the geometry its layout works on: the
	// one-channel form (decimating by 2 or 4: 8192 -> 4096 / 2048 points; 1:1: 8192 points), the split 2x up-sampling
	// form (8192 points 1:1), the pair itself -- with a complex spectrum one complex multiplication per bin
	const PairTables pk = pair_tables(g);
	const int n = pk == kTabSolo || pk == kTabSoloDown ? g.n_in / 2 : g.n_in;
	const int n2 = pk == kTabSoloDown ? g.n_out / 2 : (pk == kTabPair ? g.n_out : n);
	switch (pk)
	{
	case kTabSoloDown: T.hp = g.complex_h ? pair_constants_solo_down_complex(H, n) : pair_constants_solo_down(H, n, g.down); break;
	case kTabSolo: T.hp = g.complex_h ? pair_constants_solo_complex(H, n) : pair_constants_solo(H, n); break;
	case kTabSplit: T.hp = g.complex_h ? pair_constants_split_complex(H, n) : pair_constants_split(H, n); break;
	case kTabPair: T.hp = g.complex_h ? pair_constants_complex(H, g.n_in, g.n_out) : pair_constants(H, g.n_in, g.n_out); break;
	case kTabNone: break;
	}
	if (pk != kTabNone) T.ptw = pair_twiddles(T.tw, g.bl2, n, n2);
	return T;
}

std::vector<double> whole_step_rows(const StagePlan& w)
{
	const std::vector<double>& t = w.bank->table;
	std::vector<double> rows((size_t) w.flen * w.out_step);
	for (int r = 0; r < w.out_step; r++)
	{
		const int ph = (int) (((long long) r * w.in_step) % w.out_step);
		for (int i = 0; i < w.flen; i++)
			rows[(size_t) i * w.out_step + r] = t[(size_t) ph * w.flen + i];
	}
	return rows;
}

// whether a whole-step interpolator has two-phase tables at all: at most 24 taps, 2 ... 510 phases, the window starts of a
// phase pair at most three samples apart; *maxdl_out: that distance
bool two_phase_possible(const StagePlan& w, int* maxdl_out)
{
	const int In = w.in_step, Out = w.out_step;
	if (w.flen > 24 || Out < 2 || Out > 510) return false;
	const int NP = (Out + 1) / 2, nsg = (NP + 15) / 16;
	if (16 / nsg < 1) return false;
	int maxdl = 0;
	for (int q = 0; 2 * q + 1 < Out; q++)
		maxdl = std::max(maxdl, (int) ((long long) (2 * q + 1) * In / Out) - (int) ((long long) (2 * q) * In / Out));
	if (maxdl_out) *maxdl_out = maxdl;
	return maxdl <= 3;
}

// The lane deal of a ratio: which (data quad, set) item each of the 64 (service group, lane quad) slots of a workgroup
// takes -- [service group * 4 + rank] -> item = set * NQ + data quad, -1: the slot stays empty.
//
// Phase pairs go to lanes in QUADS: the four lanes of an aligned lane quad own four consecutive phase pairs of one
// group set, i.e. store 64 consecutive bytes of a channel's output per group (one L2 write request per quad;
// assigned pair by pair, the 16-byte pieces of a store instruction were scattered over the whole group: 19 bytes
// per request measured).  A workgroup has 16 LDS service groups of four lane quads each (the 16 lanes LDS serves
// in one cycle of a 16-byte read), and a service group takes as many cycles as its most crowded 16-byte bank
// group: ONE pair of windows starting in the same bank group (start mod 16) doubles the time of all its reads.
// The (data quad, set) items -- NQ x nsets <= 64 -- are therefore dealt to the 64 (service group, lane quad)
// slots such that as few service groups as possible hold a clash.  Items of DIFFERENT sets may share a service
// group (a set shifts the window starts by In mod 16), and slots may stay empty: with both freedoms cfg2 comes to
// 2 clashing service groups of 16, where set-by-set dealing left one clash in every group (7.5 LDS cycles per read
// instead of 4; counters: bank conflicts 30 % of the LDS cycles).  Deterministic annealing over slot swaps (fixed
// seed: the same tables for the same ratio, always).
static std::vector<int> lane_deal(int In, int Out)
{
	const int NP = (Out + 1) / 2;           // phase pairs
	const int nsg = (NP + 15) / 16;         // 16-lane LDS service groups per set
	const int nsets = 16 / nsg;             // a workgroup has 16 service groups
	const int NQ = (NP + 3) / 4, NI = NQ * nsets;
	std::vector<int> slot_item(64, -1);
	// (the table depends on the ratio alone: searched once per process and ratio)
	// (bounded like the designer's caches -- kLaneDealCacheMax ratios, most recently used first; an entry is copied out,
	// so dropping the oldest one costs a host that comes back to its ratio one more search, nothing else)
	static std::mutex cache_mutex;
	static std::list<std::pair<std::pair<int, int>, std::vector<int>>> cache;
	{
		std::lock_guard<std::mutex> lock(cache_mutex);
		for (auto it = cache.begin(); it != cache.end(); ++it)
			if (it->first == std::make_pair(In, Out))
			{
				cache.splice(cache.begin(), cache, it);
				return cache.front().second;
			}
	}
	auto r_of = [&](int ph) { return (int) ((long long) ph * In / Out); };
	auto res_of = [&](int item, int j) // bank group of the window start of pair j of the item (-1: no such pair)
	{
		const int dq = item % NQ, set = item / NQ, q = 4 * dq + j;
		return q < NP ? (int) ((r_of(2 * q) + (long long) In * set) & 15) : -1;
	};
	auto sg_cost = [&](const int* sl) // clashes of one service group
	{
		int cnt[16] = { 0 }, c = 0;
		for (int k = 0; k < 4; k++)
			if (sl[k] >= 0)
				for (int j = 0; j < 4; j++)
				{
					const int r = res_of(sl[k], j);
					if (r >= 0 && cnt[r]++) c++;
				}
		return c;
	};
	// start: set by set, data quads in order
	for (int i = 0; i < NI; i++)
	{
		const int set = i / NQ, dq = i % NQ;
		slot_item[(size_t) ((set * nsg + dq / 4) * 4 + dq % 4)] = i;
	}
	auto total = [&]()
	{
		int c = 0;
		for (int g = 0; g < 16; g++) c += sg_cost(&slot_item[(size_t) g * 4]);
		return c;
	};
	std::vector<int> best = slot_item;
	int cur = total(), best_cost = cur;
	unsigned long long rng = 0x9E3779B97F4A7C15ull;
	auto next = [&]() { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return (unsigned) (rng >> 33); };
	double temp = 1.0;
	for (int it = 0; it < 250000 && best_cost > 0; it++)
	{
		const int a = (int) (next() % 64u), b = (int) (next() % 64u);
		if (a / 4 == b / 4 || (slot_item[(size_t) a] < 0 && slot_item[(size_t) b] < 0)) continue;
		int* ga = &slot_item[(size_t) (a / 4) * 4];
		int* gb = &slot_item[(size_t) (b / 4) * 4];
		const int before = sg_cost(ga) + sg_cost(gb);
		std::swap(slot_item[(size_t) a], slot_item[(size_t) b]);
		const int after = sg_cost(ga) + sg_cost(gb);
		bool keep = after <= before;
		if (!keep)
		{
			// (accept a worse state with probability exp(-(after - before) / temp))
			const double u = (next() & 0xffffff) / 16777216.0;
			keep = u < std::exp(-(after - before) / temp);
		}
		if (keep) cur += after - before;
		else std::swap(slot_item[(size_t) a], slot_item[(size_t) b]);
		if (cur < best_cost)
		{
			best_cost = cur;
			best = slot_item;
		}
		temp = std::max(0.05, temp * 0.99998);
	}
	slot_item = best;
	{
		std::lock_guard<std::mutex> lock(cache_mutex);
		bool have = false; // (another thread may have searched the same ratio meanwhile: same table, one entry)
		for (const auto& e : cache) have = have || e.first == std::make_pair(In, Out);
		if (!have)
		{
			int dropped = 0;
			while (cache.size() >= (size_t) kLaneDealCacheMax)
			{
				cache.pop_back();
				dropped++;
			}
			cache.emplace_front(std::make_pair(In, Out), slot_item);
			lane_deal_cache_count(1 - dropped, nullptr);
		}
	}
	if (std::getenv("R8B_DEBUG_TWO")) fprintf(stderr, "two-phase tables: %d phase pairs in %d quads x %d sets, %d bank clashes over the 16 service groups\n", NP, NQ, nsets, best_cost);
	return slot_item;
}

std::optional<TwoPhaseTables> two_phase_tables(const StagePlan& w)
{
	const int In = w.in_step, Out = w.out_step;
	int maxdl = 0;
	if (!two_phase_possible(w, &maxdl)) return std::nullopt;
	const int NP = (Out + 1) / 2;           // phase pairs
	const int nsg = (NP + 15) / 16;         // 16-lane LDS service groups per set
	const int NQ = (NP + 3) / 4;
	auto r_of = [&](int ph) { return (int) ((long long) ph * In / Out); };
	TwoPhaseTables R;
	R.nsets = 16 / nsg;                     // a workgroup has 16 service groups
	// rows of T2 entries: the taps plus the largest distance between the window starts of a pair
	const int T2 = R.taps2 = maxdl <= 1 ? 25 : 27;
	const std::vector<int> slot_item = lane_deal(In, Out);
	// lanes LDS serves together for 16-byte reads (MI355X_MICROARCH.md, LDS): within each half of a
	// wave the quads {0, 3, 5, 6} and {1, 2, 4, 7}
	R.ptab.assign(256, -1);
	const int ctp = (NP + 3) & ~3;
	R.ctab.assign((size_t) 2 * T2 * ctp, 0.0);
	const std::vector<double>& T = w.bank->table;
	for (int t = 0; t < 256; t++)
	{
		const int wave = t >> 6, lane = t & 63, half = lane >> 5, quad = (lane & 31) >> 2;
		static const int cls_of[8] = { 0, 1, 1, 0, 1, 0, 0, 1 }, rank_of[8] = { 0, 0, 1, 1, 2, 2, 3, 3 };
		const int sg = 4 * wave + 2 * half + cls_of[quad];
		const int item = slot_item[(size_t) (sg * 4 + rank_of[quad])];
		if (item < 0) continue;
		const int set = item / NQ;
		const int q = 4 * (item % NQ) + (lane & 3);
		if (q >= NP) continue;
		R.ptab[(size_t) t] = q | (set << 8) | (r_of(2 * q) << 12);
		const int p0 = 2 * q, p1 = 2 * q + 1;
		const int row0 = (int) (((long long) p0 * In) % Out);
		// value v (0 .. 2 T2 - 1: the T2 taps of phase p0, then of p1 shifted by its window offset) of phase PAIR q
		// sits in pair v / 2: ctab[((v / 2) * ctp + q) * 2 + v % 2], ctp = NP rounded up to whole quads.  Indexed by the
		// pair, not by the thread: the lanes of the nsets sets that own the same pair read the same entries, and a
		// workgroup pulls every row through L2 once instead of nsets times (cfg2: 34 KB instead of 102 KB per block).
		auto put = [&](int v, double x) { R.ctab[((size_t) (v / 2) * ctp + q) * 2 + (v & 1)] = x; };
		for (int i = 0; i < w.flen; i++) put(i, T[(size_t) row0 * w.flen + i]);
		if (p1 < Out)
		{
			const int row1 = (int) (((long long) p1 * In) % Out), dl = r_of(p1) - r_of(p0);
			for (int i = 0; i < w.flen; i++) put(T2 + i + dl, T[(size_t) row1 * w.flen + i]);
		}
	}
	return R;
}

} // namespace r8bhip
