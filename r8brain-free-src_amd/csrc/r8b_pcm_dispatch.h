// r8b_pcm_dispatch.h -- which kernel a PcmLaunch runs (launch_pcm_in, launch_pcm_out).  The launch's fields pick the
// form, in this order:
//   plain / finishing / clip   clip_len set: a clip form (r8b_clip*.h); else, egress with dither or meters: a finishing
//                              form; else the plain kernels (r8b_pcm.h)
//   rows / tiles               `interleaved` clear: a workgroup per chunk of a row; set: per tile.  The mixing ingest
//                              (clip_len AND mix_channels, ingest only) is a tile kernel for either layout
//   addressing (clip forms)    ClipStrided; clip_base set: ClipPacked; egress with clip_base AND (clip_chan OR clip_pad)
//                              (clip_sched_launch, r8b_clip_sched.h: asked here alone): ClipSched, PAD by clip_pad.
//                              The strided egress stores its padding (PAD), the packed one has none
//   <DITHER, METER>            egress: by `dither` and m_peak.  The finishing kernels have no <false, false> -- that is
//                              the plain egress -- the clip egress kernels have one
// and with the form come the launcher's refusals, the grid and the dynamic LDS bytes.
// One copy for the device launcher (r8b_kernels.hip) and the CPU emulator (tests/emul/emul_pcm.cpp), which include it
// after the kernel headers and differ only in the backend B that runs what was decided -- a call per kernel family, with
// the template arguments the kernels take (Base: the addressing rule):
//   void pcm_rows_in(L, g);  void pcm_in(L, g);  void pcm_rows_out(L, g);  void pcm_out(L, g);
//   template<bool DITHER, bool METER> void pcm_rows_finish(L, g);  ... void pcm_finish(L, g);
//   template<class Base> void clip_rows_in(L, g);  ... void clip_frames_in(L, g);  ... void clip_mix_in(L, g);
//   template<class Base, bool PAD, bool DITHER, bool METER> void clip_rows_out(L, g);  ... void clip_frames_out(L, g);
#ifndef R8B_PCM_DISPATCH_H
#define R8B_PCM_DISPATCH_H

#include <initializer_list>
#include <stdexcept>
#include <string>
#include <type_traits>

namespace r8bhip {

struct PcmGrid
{
	unsigned x, y; // workgroups: chunks or tiles of the window by rows, channel groups or clips
	size_t lds;    // dynamic LDS bytes
};

namespace {

// planar buffers: chunks of kPcmRowChunk frames by rows
inline PcmGrid pcm_row_grid(const PcmLaunch& L)
{
	return {(unsigned) ((L.n + kPcmRowChunk - 1) / kPcmRowChunk), (unsigned) L.nch, 0};
}

// frame-major buffers: tiles of kPcmTile frames by groups of kPcmTile channels
inline PcmGrid pcm_tile_grid(const PcmLaunch& L)
{
	return {(unsigned) ((L.n + kPcmTile - 1) / kPcmTile), (unsigned) ((L.nch + kPcmTile - 1) / kPcmTile), 0};
}

// clips through a tile of Kt rows (clip_channels, or mix_channels on a mixing ingest): tiles of FT frames by clips, and
// the tile's bytes (16 KB; at most kClipTileDoubles doubles, 33 KB, at Kt = 64)
inline PcmGrid clip_tile_grid(const PcmLaunch& L, int Kt, int lanes)
{
	const long long FT = 1LL << clip_tile_log2(Kt);
	return {(unsigned) ((L.n + FT - 1) / FT), (unsigned) (L.nch / L.clip_channels),
		(size_t) Kt * (FT + clip_tile_pad(Kt, lanes)) * sizeof(double)};
}

// (the tile forms alone: a planar clip side has rows, not clips)
inline void clip_channels_check(const PcmLaunch& L)
{
	const int K = L.clip_channels;
	if (K < 1 || K > kClipChannelsMax || L.nch % K != 0)
		throw std::logic_error("launch_pcm: clip_channels must be 1 .. 64 and divide the channel count");
}

// a kernel's device symbol as rocprofv3 prints it without namespace and argument list -- "k_pcm_finish<true, false>",
// the template arguments in the kernel's own order -- for the backends' launch_symbol_note
inline std::string pcm_symbol(const char* name, std::initializer_list<bool> args = {})
{
	std::string s(name);
	for (const bool* a = args.begin(); a != args.end(); a++)
		s += std::string(a == args.begin() ? "<" : ", ") + (*a ? "true" : "false");
	return args.size() != 0 ? s + ">" : s;
}

// f(DITHER, METER) with the two as constants
template<class F>
void pcm_finish_instance(bool dither, bool meter, F f)
{
	if (dither && meter) f(std::true_type(), std::true_type());
	else if (meter) f(std::false_type(), std::true_type());
	else if (dither) f(std::true_type(), std::false_type());
	else f(std::false_type(), std::false_type());
}

// the clip egress of one addressing rule
template<class Base, bool PAD, class B>
void clip_out_dispatch(const PcmLaunch& L, B& b)
{
	pcm_finish_instance(L.dither != 0, L.m_peak != nullptr, [&](auto dither, auto meter)
	{
		constexpr bool DITHER = decltype(dither)::value, METER = decltype(meter)::value;
		if (L.interleaved)
			b.template clip_frames_out<Base, PAD, DITHER, METER>(L, clip_tile_grid(L, L.clip_channels, kClipLanesOut));
		else b.template clip_rows_out<Base, PAD, DITHER, METER>(L, pcm_row_grid(L));
	});
}

} // namespace

template<class B>
void pcm_in_dispatch(const PcmLaunch& L, B& b)
{
	if (L.n <= 0 || L.nch <= 0) return;
	if (L.clip_len == nullptr)
	{
		if (L.interleaved) b.pcm_in(L, pcm_tile_grid(L));
		else b.pcm_rows_in(L, pcm_row_grid(L));
		return;
	}
	const bool packed = L.clip_base != nullptr;
	if (L.mix_channels != 0)
	{
		clip_channels_check(L);
		if (L.mix_channels < 1 || L.mix_channels > kClipChannelsMax || L.mix == nullptr)
			throw std::logic_error("launch_pcm_in: mix_channels must be 1 .. 64 and come with a matrix");
		const PcmGrid g = clip_tile_grid(L, L.mix_channels, kClipLanesIn);
		if (packed) b.template clip_mix_in<ClipPacked>(L, g);
		else b.template clip_mix_in<ClipStrided>(L, g);
	}
	else if (L.interleaved)
	{
		clip_channels_check(L);
		const PcmGrid g = clip_tile_grid(L, L.clip_channels, kClipLanesIn);
		if (packed) b.template clip_frames_in<ClipPacked>(L, g);
		else b.template clip_frames_in<ClipStrided>(L, g);
	}
	else if (packed) b.template clip_rows_in<ClipPacked>(L, pcm_row_grid(L));
	else b.template clip_rows_in<ClipStrided>(L, pcm_row_grid(L));
}

template<class B>
void pcm_out_dispatch(const PcmLaunch& L, B& b)
{
	if (L.n <= 0 || L.nch <= 0) return;
	const bool clip = L.clip_len != nullptr;
	if (clip && L.interleaved) clip_channels_check(L);
	if (L.m_peak != nullptr && (L.m_clipped == nullptr || L.m_nonfinite == nullptr))
		throw std::logic_error("launch_pcm_out: meters need all three arrays");
	if (!clip)
	{
		pcm_finish_instance(L.dither != 0, L.m_peak != nullptr, [&](auto dither, auto meter)
		{
			constexpr bool DITHER = decltype(dither)::value, METER = decltype(meter)::value;
			if constexpr (!DITHER && !METER)
			{
				if (L.interleaved) b.pcm_out(L, pcm_tile_grid(L));
				else b.pcm_rows_out(L, pcm_row_grid(L));
			}
			else if (L.interleaved) b.template pcm_finish<DITHER, METER>(L, pcm_tile_grid(L));
			else b.template pcm_rows_finish<DITHER, METER>(L, pcm_row_grid(L));
		});
		return;
	}
	if (clip_sched_launch(L))
	{
		if (L.clip_pad != 0) clip_out_dispatch<ClipSched, true>(L, b);
		else clip_out_dispatch<ClipSched, false>(L, b);
	}
	else if (L.clip_base != nullptr) clip_out_dispatch<ClipPacked, false>(L, b);
	else clip_out_dispatch<ClipStrided, true>(L, b);
}

} // namespace r8bhip

#endif
