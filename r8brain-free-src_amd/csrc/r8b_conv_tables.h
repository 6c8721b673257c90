// r8b_conv_tables.h -- the tables the convolver kernels read, computed from a designed filter (r8b_design.h) and a stage's
// geometry (r8b_plan.h).  Host arithmetic only, in long double: nothing here touches a device or an Engine, and the unit
// links into a program that has no launcher at all (tests/cxx_conv_tables.cpp).  The engine asks three questions --
// conv_tables, whole_step_rows, two_phase_tables -- and uploads what they return; the builders below them are declared
// for the tests.
#ifndef R8B_CONV_TABLES_H
#define R8B_CONV_TABLES_H

#include <optional>
#include <vector>

#include "r8b_design.h"
#include "r8b_plan.h"

namespace r8bhip {

// ---- which kernels exist for a geometry (r8b_launch.h conv*_ok), asked by conv_tables and by Engine::resolve_forms' rules only ----
// the one-channel kernel (r8b_convx.h), behind a 3x zero-stuffing load / in front of a 3x strided store as well
bool convx_edge3(const ConvGeom& g);
bool convx_plain(const ConvGeom& g);
// the pair kernel (r8b_convp.h): the layout that takes the geometry -- and whose constants conv_tables builds, whatever
// the options say --: the one-channel form on 16384-point blocks, decimating in the spectrum (a complex spectrum: by 2
// only) or 1:1, the split form on 8192 -> 16384 points, the pair itself (3x edges included)
enum PairTables { kTabNone, kTabPair, kTabSplit, kTabSolo, kTabSoloDown };
bool pair_plain(const ConvGeom& g);
bool pair_edge3(const ConvGeom& g);
PairTables pair_tables(const ConvGeom& g);

// The tables of one convolver stage, interleaved (re, im) where complex; empty where the stage has none.
//   H / Hc       the kernel spectrum, real or (ConvGeom::complex_h) complex -- one of the two
//   tw           exp(-2 pi i e / bl2), bl2 entries
//   spec, spec2  the one-channel kernel's spectral constants, per slot and (no decimation) per backward position: real
//                spectra on a geometry that kernel has
//   hp, ptw      the pair kernel's constants and twiddles, in the layout pair_tables names -- on the transforms that layout
//                works on: the one-channel forms on half the block's lengths, the split form 1:1 on the forward length
//   hp3, ptw3    the polyphase 3x form (ConvGeom::p3): the three component spectra and the twiddles of its own geometry
//                (beside the tables of the zero-stuffing block, which option up3_poly = 0 falls back to)
struct ConvTables
{
	std::vector<double> H, Hc, tw, spec, spec2, hp, ptw, hp3, ptw3;
};
ConvTables conv_tables(const StagePlan& sp);

// whole-step interpolator: the bank transposed per residue class (the fused kernels' wtab): w[i * Out + r] = row
// (r In) mod Out of the bank, tap i
std::vector<double> whole_step_rows(const StagePlan& w);

// Tables of the pair kernel's two-phases-per-thread interpolator (r8b_convp.h MODE 4) behind a whole-step interpolator w:
// ptab: per thread of a 256-thread workgroup, q | set << 8 | floor(2 q In / Out) << 12 of its phase pair q (-1: idle);
// ctab: row pairs of taps2 entries per phase pair (two_phase_tables, r8b_conv_tables.cpp); nsets: group sets per workgroup;
// taps2: 25 (window starts of a pair at most one sample apart) or 27.  Nothing: more than 24 taps, fewer than 2 or more
// than 510 phases, or window starts more than three samples apart.  The lane deal behind ptab is searched once per
// process and ratio and kept in a bounded cache (kLaneDealCacheMax, r8b_design.h).
struct TwoPhaseTables
{
	std::vector<int> ptab;
	std::vector<double> ctab;
	int nsets = 0, taps2 = 25;
};
bool two_phase_possible(const StagePlan& w, int* maxdl_out);
std::optional<TwoPhaseTables> two_phase_tables(const StagePlan& w);

// ---- the builders ----
// complex twiddle table exp(-2 pi i e / len), exact on the axes; interleaved (re, im)
std::vector<double> make_twiddles(int len);
// zero-phase kernel spectrum H[m] = sum_t h[t] cos(2 pi m t / bl2), m = 0..bl2/2, times `scale`
std::vector<double> kernel_spectrum(const LpFilter& f, int bl2, double scale);
// general form: H[m] = scale * sum_n taps[n] exp(-2 pi i m (n - align) / bl2), m = 0..bl2/2 (interleaved re, im);
// align = ConvGeom::fl2
std::vector<double> kernel_spectrum_complex(const LpFilter& f, int bl2, int align, double scale);
// constants of the fast path's spectral stage (r8b_convx.h cx_spec_write) for a block convolver
// with forward complex length N = n_in/2 and backward length N2 = N*up (up in {1,2}): per slot
// s (bin kf = bitrev(s) for s < N/2, kf = N/2 for s == N/2) 4 (up 1) or 8 (up 2) complex values,
// constant c of slot s at [c*(N/2+1) + s]; interleaved (re, im).  H is the scaled kernel
// spectrum (kernel_spectrum), tw the exp(-2 pi i e / bl2) table.
std::vector<double> spectral_constants(const std::vector<double>& H, const std::vector<double>& tw,
	int bl2, int n_in, int up);
// The same for the 2x-decimating convolver (r8b_convx.h, UPLOG < 0): slot -> backward pair
// (k, N2-k), N2 = N / down, fed by the forward bins idx = {k, N-k, N2-k, N-N2+k}:
//   Z'[k]    = c0 Z1 + c1 conj Z2 + c2 conj Z3 + c3 Z4      (form 1)
//   Z'[N2-k] = c4 conj Z1 + c5 Z2 + c6 Z3 + c7 conj Z4      (form 2; slot k = 0: added to Z'[0])
// The constants are read off a long-double model of the chain real-FFT unpacking -> kernel
// multiplication -> Nyquist fix-up of the shortened transform (reference
// CDSPBlockConvolver.h:329-342) -> packing, by probing it with unit inputs: a real-linear map of
// one complex input is a*z + b*conj(z) with a = (F(1) - i F(i)) / 2, b = (F(1) + i F(i)) / 2.
std::vector<double> spectral_constants_down(const std::vector<double>& H,
	const std::vector<double>& tw, int bl2, int n_in, int down);
// Constants of the fast path's spectral stage addressed by output position (r8b_convx.h
// cx_spec2_compute): entry c * N2 + P holds ca (c = 0) / cb (c = 1) of bin bitrev(P), where backward bin k =
// ca(k) Z[k mod N] + cb(k) conj(Z[-k mod N]) -- every case of the per-slot table `sc` (spectral_constants, up 1 or 2)
// reduces to this form.
std::vector<double> spectral_constants_by_position(const std::vector<double>& sc, int n_in, int up);
// kernel constants of the pair kernel's middle pass (r8b_convp.h): 8 x NT pairs, NT = max(n_in, n_out) / 16, entry
// c * NT + t; 2x up (n_out = 2 n_in): (H[k] + H[k+N], H[k] - H[k+N]) for forward position 8 t + c, bin k =
// bitrev(position), N = n_in; 1:1: H of backward positions 16 t + 2 c and 16 t + 2 c + 1; decimating by D = n_in / n_out
// (r8b_convp.h cp_middle_compute_down): thread t keeps the forward positions 16 t + 2 D (c' / 2) + (c' odd ? 2 D - 1 : 0),
// c' = 0 .. 16 / D - 1; entry (c, t) = H of c' = 2c, 2c + 1.  H is the scaled kernel spectrum (bl2/2 + 1 reals), mirrored
// for bins above bl2/2.
std::vector<double> pair_constants(const std::vector<double>& H, int n_in, int n_out);
// The same with a complex kernel spectrum Hc (bl2/2 + 1 complex bins, Hermitian beyond): 16 x NT entries of one complex
// value (r8b_convp.h cp_hp_prefetch, CX) -- 1:1: H of backward position 16 t + c; 2x up: Hs (c < 8) / Hd
// (c >= 8) of forward position 8 t + (c & 7); decimating: H of the thread's kept position c.
std::vector<double> pair_constants_complex(const std::vector<double>& Hc, int n_in, int n_out);
// ... of the split 2x up-sampling form (r8b_convp.h cp_sp_middle): 16 x (n_in / 16) pairs, entry c * NT + t = (H[k] +
// H[k + n_in], H[k] - H[k + n_in]) for forward position 16 t + c, bin k = bitrev(position); H over 2 n_in points
std::vector<double> pair_constants_split(const std::vector<double>& H, int n_in);
// ... of the one-channel form (r8b_convp.h cp_solo_mid_b): 16 x (n / 16) pairs (a, b) per forward position 16 t + c of the
// n-point complex transform, bin k = bitrev(position): a = (H[k] + H[k + n]) - (H[k] - H[k + n]) sin(pi k / n),
// b = (H[k] - H[k + n]) cos(pi k / n); H over 2 n points
std::vector<double> pair_constants_solo(const std::vector<double>& H, int n);
// ... decimating by `down` = 2 or 4 (cp_solo_mid_b_down): per forward position 16 t + c, c a multiple of down -- kept bin k --:
// (H[k], H[n / down - k]);
// c + 1: (cos, sin) of pi k / n
std::vector<double> pair_constants_solo_down(const std::vector<double>& H, int n, int down);
// ... of the split form and of the one-channel form (1:1) with a complex kernel spectrum Hc (n + 1 complex bins, Hermitian
// beyond): 32 x (n / 16) complex entries -- split: H[k] + H[k+n], then (H[k] - H[k+n]) e^{+i pi k / n}; one-channel:
// A = (H[k] + H[k+n]) - (H[k] - H[k+n]) sin(pi k / n), then B = i (H[k] - H[k+n]) cos(pi k / n)
std::vector<double> pair_constants_split_complex(const std::vector<double>& Hc, int n);
std::vector<double> pair_constants_solo_complex(const std::vector<double>& Hc, int n);
// ... one-channel form decimating by 2: 24 x (n / 16) entries -- row c even: H[k]; c + 1: (cos, sin) of pi k / n; row
// 16 + c / 2: H[n / 2 - k]
std::vector<double> pair_constants_solo_down_complex(const std::vector<double>& Hc, int n);
// Polyphase 3x form (ConvGeom::p3; r8b_convp.h mode 19): the spectra of the filter's three polyphase components
// g_r[d] = h[3 d + r + fl2], d in [-a, b], each laid out circularly so that the block's first valid output comes out at
// circular position 0 -- gc_r[(d - b) mod N] = g_r[d] --, scaled by 1 / N (unnormalised transforms both ways), one
// complex value per backward position: hp3[((r * 16 + c) * NT + t)] = G_r[bitrev(16 t + c)] (cf. pair_constants_complex).
std::vector<double> pair_constants_poly3(const LpFilter& f, int fl2, int N, int a, int b);
// twiddle base powers of the pair kernel's passes per thread (r8b_convp.h ptw_fetch), rows of NT = max(n_in, n_out) / 16
// complex entries, 6 per slot; slots 0-2 forward passes (radix e1 = n_in / NT); then, 1:1 / 2x up: 3 the backward pass with
// sub-length 256, 4 + m butterfly m of the last backward pass (sub-length n_out); decimating, or 8192 points (the mirrored
// backward side): 2 + I backward pass I (radix e2 = n_out / NT, sub-length rmb e2^I).  tw = exp(-2 pi i e / tw_len) table
std::vector<double> pair_twiddles(const std::vector<double>& tw, int tw_len, int n_in, int n_out);
// radices (each in {2,4,8,16}, <= max_radix) whose product is N, largest first
std::vector<int> plan_radices(int N, int max_radix);

} // namespace r8bhip

#endif
