"""Host-side mirror of the reference's front-end over the C ABI (include/r8bsrc.h).

Names, arguments and behaviour follow r8b::CDSPResampler (reference CDSPResampler.h:117-120,
406-421, 476-519, 521-529, 559-575, 592-651) and its presets CDSPResampler16 / 16IR / 24
(:729-810), so the parity tests read like calls into the reference.  `BatchResampler` is the
N-channel object the throughput numbers are quoted on: process() takes torch CUDA tensors (device
memory and streams are the only things torch is used for).

`lib=` lets the tests bind another library that exports the same ABI; the default is the HIP
library and nothing else.
"""
import ctypes as C

import numpy as np

from . import _capi

fprLinearPhase = 0
fprMinPhase = 1


# r8b_pcm_format (include/r8bsrc.h)
PCM_F64, PCM_F32, PCM_S16, PCM_S24, PCM_S32 = 0, 1, 2, 3, 4
# ... the one-byte formats: unsigned 8-bit PCM and G.711 mu-law / A-law, uint8 tensors named by `in_format=`
PCM_U8, PCM_ULAW, PCM_ALAW = 16, 17, 18
_PCM8 = (PCM_U8, PCM_ULAW, PCM_ALAW)
# r8b_dither_mode
DITHER_NONE, DITHER_TPDF = 0, 1
# enum r8b_clip_flags (include/r8bsrc.h)
CLIPS_DROP_FINISHED, CLIPS_LONGEST_FIRST = 1, 2
# enum r8b_pseudo_stage: the PCM boundary's launches in r8b_batch_stage_symbol
STAGE_PCM_IN, STAGE_PCM_OUT = -1, -2


def _dptr(a):
    return a.ctypes.data_as(_capi.dp)


def _pcm_formats():
    """(r8b_pcm_format of a tensor's dtype, dtype of a format's tensor)"""
    import torch
    fmt_of = {torch.float64: PCM_F64, torch.float32: PCM_F32, torch.int16: PCM_S16,
              torch.int32: PCM_S32, torch.uint8: PCM_S24}
    dtype_of = {v: k for k, v in fmt_of.items()}
    dtype_of.update({f: torch.uint8 for f in _PCM8})
    return fmt_of, dtype_of


def _pcm_in_format(x, in_format, dims, fmt_of):
    """the format of the input tensor x, whose samples have `dims` axes.  in_format None: by the dtype, uint8 being packed
    24-bit with a trailing axis of 3; a one-byte format has to be named: x is uint8 without that axis"""
    inferred = fmt_of[x.dtype]
    if in_format is None:
        if inferred == PCM_S24 and x.dim() == dims:
            raise ValueError("a uint8 tensor without the trailing axis of 3 of packed 24-bit samples: name its format "
                             "with in_format= (PCM_U8, PCM_ULAW or PCM_ALAW)")
        return inferred
    in_format = int(in_format)
    if (inferred != PCM_S24 or x.dim() != dims) if in_format in _PCM8 else in_format != inferred:
        raise ValueError("in_format=%d does not describe a %s tensor of %d dimensions" % (in_format, x.dtype, x.dim()))
    return in_format


class _Base:
    def __init__(self, lib):
        self._lib = lib if lib is not None else _capi.load()
        self._h = None

    def _err(self):
        return self._lib.r8b_last_error().decode()


class BatchResampler(_Base):
    """`nch` independent CDSPResampler streams sharing one schedule (C ABI part 2)."""

    def __init__(self, SrcSampleRate, DstSampleRate, aMaxInLen, ReqTransBand=2.0,
                 ReqAtten=206.91, nch=1, device=-1, lib=None, stage=None, phase=0):
        """phase: 0 = fprLinearPhase (the reference's default), 1 = fprMinPhase"""
        super().__init__(lib)
        self.nch = int(nch)
        self.MaxInLen = int(aMaxInLen)
        self._rates = (float(SrcSampleRate), float(DstSampleRate))
        if stage is not None:
            kind, a, b, c, d, i0, i1 = stage
            self._h = self._lib.r8b_batch_create_stage(int(kind), a, b, c, d, int(i0), int(i1),
                                                       self.MaxInLen, self.nch, int(device))
        elif phase:
            self._h = self._lib.r8b_batch_create_ex(SrcSampleRate, DstSampleRate, self.MaxInLen,
                                                    ReqTransBand, ReqAtten, int(phase), self.nch,
                                                    int(device))
        else:
            self._h = self._lib.r8b_batch_create(SrcSampleRate, DstSampleRate, self.MaxInLen,
                                                 ReqTransBand, ReqAtten, self.nch, int(device))
        if not self._h:
            raise RuntimeError(self._err())
        self.max_out_len = self._lib.r8b_batch_max_out_len(self._h)

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.r8b_batch_delete(self._h)
            self._h = None

    def getMaxOutLen(self, MaxInLen=0):
        return self.max_out_len

    def getInLenBeforeOutPos(self, ReqOutPos):
        return self._lib.r8b_batch_inlen_before_outpos(self._h, int(ReqOutPos))

    def getInputRequiredForOutput(self, ReqOutSamples):
        return self._lib.r8b_batch_inlen(self._h, int(ReqOutSamples))

    def clear(self):
        self._lib.r8b_batch_clear(self._h)
        self._produced = 0

    def describe(self):
        n = self._lib.r8b_batch_describe(self._h, None, 0)
        buf = C.create_string_buffer(n + 1)
        self._lib.r8b_batch_describe(self._h, buf, n + 1)
        return buf.value.decode()

    def set_option(self, name, value):
        if self._lib.r8b_batch_set_option(self._h, name.encode(), int(value)) != 0:
            raise KeyError(name)

    def getLatencyFrac(self):
        """reference CDSPResampler.h:491-494: the chain's residual fractional latency (0.0 for linear phase)"""
        return self._lib.r8b_batch_latency_frac(self._h)

    def stat(self, name):
        """a counter of the engine since creation (include/r8bsrc.h r8b_batch_stat)"""
        v = self._lib.r8b_batch_stat(self._h, name.encode())
        if v < 0:
            raise KeyError(name)
        return v

    def stage_timings(self):
        """[(kernel name, total ms, launches, samples in, samples out)] per stage since the last
        query (needs set_option("timing", 1)); sample counts are per channel; waits for the
        recorded events."""
        res = []
        for s in range(self._lib.r8b_batch_stage_count(self._h)):
            ms, n = C.c_double(), C.c_int()
            si, so = C.c_longlong(), C.c_longlong()
            name = C.create_string_buffer(64)
            if self._lib.r8b_batch_stage_timing(self._h, s, ms, n, si, so, name, 64) != 0:
                raise RuntimeError(self._err())
            res.append((name.value.decode(), ms.value, n.value, si.value, so.value))
        return res

    def stage_symbols(self):
        """device symbol of every stage's most recent timed launch, as rocprofv3 names it (r8b_batch_stage_symbol)"""
        res = []
        for s in range(self._lib.r8b_batch_stage_count(self._h)):
            buf = C.create_string_buffer(96)
            if self._lib.r8b_batch_stage_symbol(self._h, s, buf, 96) != 0:
                raise RuntimeError(self._err())
            res.append(buf.value.decode())
        return res

    def boundary_symbols(self):
        """(ingest, egress): the device symbols of the PCM boundary's most recent launches in the most recent PCM or clip
        call made with set_option("timing", 1) -- r8b_batch_stage_symbol's pseudo-stages R8B_STAGE_PCM_IN / _OUT; "" for
        a side that call launched nothing for"""
        res = []
        for s in (STAGE_PCM_IN, STAGE_PCM_OUT):
            buf = C.create_string_buffer(96)
            if self._lib.r8b_batch_stage_symbol(self._h, s, buf, 96) != 0:
                raise RuntimeError(self._err())
            res.append(buf.value.decode())
        return tuple(res)

    def process_ptr(self, d_in, in_stride, l, d_out, out_stride, stream=0):
        """Raw device-pointer entry (r8b_batch_process)."""
        n = self._lib.r8b_batch_process(self._h, C.c_void_p(d_in), in_stride, int(l),
                                        C.c_void_p(d_out), out_stride, C.c_void_p(stream))
        if n < 0:
            raise RuntimeError(self._err())
        return n

    def process(self, x, out=None):
        """x: float64 CUDA tensor [nch, l] (row stride >= l); returns a view [nch, n] of `out`
        (allocated [nch, max_out_len] if not given).  Enqueues on torch's current stream."""
        import torch
        assert x.is_cuda and x.dtype == torch.float64 and x.dim() == 2 and x.shape[0] == self.nch
        assert x.stride(1) == 1
        dev = self._lib.r8b_batch_device(self._h)
        if x.device.index != dev or (out is not None and out.device.index != dev):
            raise ValueError("tensors on cuda:%s, the resampler lives on cuda:%d" % (x.device.index, dev))
        l = x.shape[1]
        if out is None:
            # rows on a 64-byte pitch, this call's outputs at column (outputs produced so far) mod 8: output j of
            # the stream always sits at a column congruent to j mod 8, so the 64-byte pieces the fused kernels store
            # (four adjacent phase pairs of a group) are whole aligned segments in every call
            cap = max(self.max_out_len, 1)
            off = getattr(self, "_produced", 0) % 8
            out = torch.empty((self.nch, (cap + 7) // 8 * 8 + 8), dtype=torch.float64, device=x.device)[:, off:off + cap]
        assert out.is_cuda and out.dtype == torch.float64 and out.stride(1) == 1
        assert out.shape[0] == self.nch and out.shape[1] >= self.max_out_len
        stream = torch.cuda.current_stream(x.device).cuda_stream
        n = self.process_ptr(x.data_ptr(), x.stride(0), l, out.data_ptr(), out.stride(0), stream)
        self._produced = getattr(self, "_produced", 0) + n
        return out[:, :n]

    def state_dict(self, stream=0):
        """Checkpoint of the streaming state of all channels as one numpy uint8 blob
        (r8b_batch_state_save); waits for `stream`."""
        size = self._lib.r8b_batch_state_size(self._h)
        buf = np.empty(size, dtype=np.uint8)
        n = self._lib.r8b_batch_state_save(self._h, C.c_void_p(buf.ctypes.data), size,
                                           C.c_void_p(stream))
        if n < 0:
            raise RuntimeError(self._err())
        return buf[:n]

    def load_state_dict(self, blob, stream=0):
        """Resume from a blob of state_dict() taken from an equally configured object."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        if self._lib.r8b_batch_state_load(self._h, C.c_void_p(blob.ctypes.data), blob.size,
                                          C.c_void_p(stream)) < 0:
            raise RuntimeError(self._err())

    def process_pcm_ptr(self, d_in, in_format, in_interleaved, in_stride, l, d_out, out_format,
                        out_interleaved, out_stride, stream=0):
        """Raw device-pointer PCM entry (r8b_batch_process_pcm); strides in samples."""
        n = self._lib.r8b_batch_process_pcm(self._h, C.c_void_p(d_in), int(in_format),
                                            int(bool(in_interleaved)), in_stride, int(l),
                                            C.c_void_p(d_out), int(out_format),
                                            int(bool(out_interleaved)), out_stride,
                                            C.c_void_p(stream))
        if n < 0:
            raise RuntimeError(self._err())
        return n

    def process_pcm(self, x, out_format=None, out=None, planar=False, in_format=None):
        """PCM in, PCM out, both CUDA tensors.  Interleaved (default): x is [frames, nch] of
        int16 / int32 / float32 / float64, or uint8 [frames, nch, 3] for packed 24-bit; returns a
        view [n, nch(, 3)] of `out` (allocated [max_out_len, nch(, 3)] if not given) in
        `out_format` (default: the input's).  planar=True: x is [nch, frames(, 3)] and the result
        [nch, n(, 3)]; the conversion then happens inside the first and last stage kernels, no
        staging copy.  in_format: PCM_U8, PCM_ULAW or PCM_ALAW for a uint8 x of one-byte samples, [frames, nch] or
        [nch, frames] (None: by the dtype, as above); an out_format of these gives a uint8 result without the trailing
        axis; such a side always goes through the staging rows.  Enqueues on torch's current stream."""
        import torch
        fmt_of, dtype_of = _pcm_formats()
        if planar:
            return self._process_pcm_planar(x, fmt_of, dtype_of, out_format, out, in_format)
        assert x.is_cuda and x.is_contiguous() and x.shape[1] == self.nch
        in_format = _pcm_in_format(x, in_format, 2, fmt_of)
        assert (x.dim() == 3 and x.shape[2] == 3) if in_format == PCM_S24 else x.dim() == 2
        if out_format is None:
            out_format = in_format
        tail = (3,) if out_format == PCM_S24 else ()
        if out is None:
            out = torch.empty((max(self.max_out_len, 1), self.nch) + tail,
                              dtype=dtype_of[out_format], device=x.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == dtype_of[out_format]
        assert out.shape[0] >= self.max_out_len and tuple(out.shape[1:]) == (self.nch,) + tail
        stream = torch.cuda.current_stream(x.device).cuda_stream
        n = self.process_pcm_ptr(x.data_ptr(), in_format, True, self.nch, x.shape[0],
                                 out.data_ptr(), out_format, True, self.nch, stream)
        return out[:n]

    def _process_pcm_planar(self, x, fmt_of, dtype_of, out_format, out, in_format=None):
        import torch
        assert x.is_cuda and x.is_contiguous() and x.shape[0] == self.nch
        in_format = _pcm_in_format(x, in_format, 2, fmt_of)
        assert (x.dim() == 3 and x.shape[2] == 3) if in_format == PCM_S24 else x.dim() == 2
        if out_format is None:
            out_format = in_format
        tail = (3,) if out_format == PCM_S24 else ()
        cap = max(self.max_out_len, 1)
        if out is None:
            out = torch.empty((self.nch, cap) + tail, dtype=dtype_of[out_format], device=x.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == dtype_of[out_format]
        assert out.shape[0] == self.nch and out.shape[1] >= self.max_out_len
        stream = torch.cuda.current_stream(x.device).cuda_stream
        n = self.process_pcm_ptr(x.data_ptr(), in_format, False, x.shape[1], x.shape[1],
                                 out.data_ptr(), out_format, False, out.shape[1], stream)
        return out[:, :n]

    def set_dither(self, mode, seed=0, first_channel=0):
        """TPDF dither of the integer PCM outputs (r8b_batch_set_dither): a pure function of (seed, first_channel +
        channel, absolute output frame), so the bytes do not depend on how the stream is cut into calls, survive
        state_dict() / load_state_dict() into an object with the same settings, and a shard that passes its channel
        offset reproduces its rows of the whole batch.  mode: DITHER_NONE / DITHER_TPDF.  May change between calls."""
        if self._lib.r8b_batch_set_dither(self._h, int(mode), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                          int(first_channel)) != 0:
            raise ValueError(self._err())

    def enable_meters(self, on=True):
        """per-channel peak / clipped / nonfinite meters of the PCM egress (r8b_batch_meter_enable)"""
        if self._lib.r8b_batch_meter_enable(self._h, int(bool(on))) != 0:
            raise RuntimeError(self._err())

    def read_meters(self, reset=False, stream=0):
        """{"peak": float64[nch], "clipped": int64[nch], "nonfinite": int64[nch]} accumulated by the process_pcm calls
        since the last reset / clear(); waits for `stream`.  Raises if the meters were never enabled."""
        peak = np.empty(self.nch, dtype=np.float64)
        clipped = np.empty(self.nch, dtype=np.int64)
        nonfinite = np.empty(self.nch, dtype=np.int64)
        llp = C.POINTER(C.c_longlong)
        if self._lib.r8b_batch_meter_read(self._h, _dptr(peak), clipped.ctypes.data_as(llp),
                                          nonfinite.ctypes.data_as(llp), int(bool(reset)),
                                          C.c_void_p(stream)) != 0:
            raise RuntimeError(self._err())
        return {"peak": peak, "clipped": clipped, "nonfinite": nonfinite}

    def enable_true_peak(self, on=True):
        """per-channel true-peak meter of the PCM egress (r8b_batch_true_peak_enable): the maximum of the 4x interpolated
        fp64 output, independent of enable_meters()"""
        if self._lib.r8b_batch_true_peak_enable(self._h, int(bool(on))) != 0:
            raise RuntimeError(self._err())

    def read_true_peak(self, reset=False, stream=0):
        """float64[nch]: the true peak of every channel, a linear amplitude like read_meters()["peak"], over the
        process_pcm / resample_clips calls since the last reset / clear(); waits for `stream`.  Raises if the meter was
        never enabled."""
        tp = np.empty(self.nch, dtype=np.float64)
        if self._lib.r8b_batch_true_peak_read(self._h, _dptr(tp), int(bool(reset)), C.c_void_p(stream)) != 0:
            raise RuntimeError(self._err())
        return tp

    def enable_loudness(self, on=True, capacity=600):
        """per-channel BS.1770 K-weighted loudness meter of the PCM egress (r8b_batch_loudness_enable): the energy of every
        100 ms sub-block, `capacity` of them per channel between two draining reads; independent of the other meters"""
        if self._lib.r8b_batch_loudness_enable(self._h, int(bool(on)), int(capacity)) != 0:
            raise RuntimeError(self._err())

    @property
    def loudness_hop(self):
        """frames of a sub-block at the destination rate (H of include/r8bsrc.h)"""
        hop = C.c_longlong()
        if self._lib.r8b_loudness_design(self._rates[1], None, None, C.byref(hop)) != 0:
            raise RuntimeError(self._err())
        return hop.value

    def read_loudness(self, drain=False, stream=0):
        """(sums float64[nch, most], counts int64[nch]): the K-weighted sum of squares of every completed sub-block of
        every channel since the last draining read / clear() (a clip call: of that call), row c valid up to counts[c];
        waits for `stream`.  Raises if the meter was never enabled."""
        llp = C.POINTER(C.c_longlong)
        counts = np.zeros(self.nch, dtype=np.int64)
        most = self._lib.r8b_batch_loudness_read(self._h, None, 0, counts.ctypes.data_as(llp), 0, C.c_void_p(stream))
        if most < 0:
            raise RuntimeError(self._err())
        sums = np.zeros((self.nch, most), dtype=np.float64)
        if self._lib.r8b_batch_loudness_read(self._h, _dptr(sums), most, counts.ctypes.data_as(llp), int(bool(drain)),
                                             C.c_void_p(stream)) < 0:
            raise RuntimeError(self._err())
        return sums, counts

    def integrated_loudness(self, sums, counts, channels_per_programme=1, weights=None):
        """float64[nch / channels_per_programme]: the gated programme loudness in LUFS of every run of
        channels_per_programme consecutive channels (r8b_loudness_integrated; -inf where no block passes the gates)"""
        sums = np.ascontiguousarray(sums, dtype=np.float64)
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        Kp = int(channels_per_programme)
        assert sums.ndim == 2 and Kp >= 1 and len(counts) == sums.shape[0] and sums.shape[0] % Kp == 0
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        assert w is None or len(w) == Kp
        nprog = sums.shape[0] // Kp
        lufs = np.empty(nprog, dtype=np.float64)
        if self._lib.r8b_loudness_integrated(_dptr(sums), sums.shape[1],
                                             counts.ctypes.data_as(C.POINTER(C.c_longlong)), nprog, Kp,
                                             None if w is None else _dptr(w), self.loudness_hop, _dptr(lufs)) != 0:
            raise RuntimeError(self._err())
        return lufs

    def clip_out_len(self, SrcSampleRate, DstSampleRate, in_len):
        """frames a clip of in_len frames yields (r8b_clip_out_len: int(in_len * Dst / Src), the reference tool's rule)"""
        return self._lib.r8b_clip_out_len(SrcSampleRate, DstSampleRate, int(in_len))

    def resample_clips_ptr(self, d_in, in_format, in_stride, in_lengths, d_out, out_format, out_stride,
                           out_lengths, stream=0):
        """Raw device-pointer entry (r8b_batch_resample_clips): planar rows, strides in samples, the two length
        sequences of nch ints each.  Returns P = max(out_lengths)."""
        assert len(in_lengths) == self.nch and len(out_lengths) == self.nch
        ll = C.c_longlong * self.nch
        p = self._lib.r8b_batch_resample_clips(self._h, C.c_void_p(d_in), int(in_format), in_stride,
                                               ll(*[int(v) for v in in_lengths]), C.c_void_p(d_out),
                                               int(out_format), out_stride,
                                               ll(*[int(v) for v in out_lengths]), C.c_void_p(stream))
        if p < 0:
            raise RuntimeError(self._err())
        self._produced = 0
        return p

    def resample_clips_ex_ptr(self, clip_channels, d_in, in_format, in_interleaved, in_stride, in_lengths, d_out,
                              out_format, out_interleaved, out_stride, out_lengths, stream=0):
        """Raw device-pointer entry (r8b_batch_resample_clips_ex): nch / clip_channels clips of clip_channels channels
        each, either side interleaved (clip i frame-major at i * stride) or planar (row c at c * stride), strides in
        samples, the two length sequences of one int per clip.  Returns P = max(out_lengths)."""
        nclips = self.nch // max(int(clip_channels), 1)
        assert len(in_lengths) == nclips and len(out_lengths) == nclips
        ll = C.c_longlong * nclips
        p = self._lib.r8b_batch_resample_clips_ex(self._h, int(clip_channels), C.c_void_p(d_in), int(in_format),
                                                  int(bool(in_interleaved)), in_stride,
                                                  ll(*[int(v) for v in in_lengths]), C.c_void_p(d_out),
                                                  int(out_format), int(bool(out_interleaved)), out_stride,
                                                  ll(*[int(v) for v in out_lengths]), C.c_void_p(stream))
        if p < 0:
            raise RuntimeError(self._err())
        self._produced = 0
        return p

    def resample_clips_mix_ptr(self, in_channels, clip_channels, mix, d_in, in_format, in_interleaved, in_stride,
                               in_lengths, d_out, out_format, out_interleaved, out_stride, out_lengths, stream=0):
        """Raw device-pointer entry (r8b_batch_resample_clips_mix): resample_clips_ex_ptr with in_channels channels
        per clip on the input side (interleaved: clip i frame-major at i * stride; planar: row i * in_channels + k at
        its multiple of stride) mixed down to the clip_channels object channels of the clip by `mix`, a
        [clip_channels, in_channels] array-like of gains (host memory).  Returns P = max(out_lengths)."""
        nclips = self.nch // max(int(clip_channels), 1)
        assert len(in_lengths) == nclips and len(out_lengths) == nclips
        m = np.ascontiguousarray(mix, dtype=np.float64)
        assert m.shape == (int(clip_channels), int(in_channels))
        ll = C.c_longlong * nclips
        p = self._lib.r8b_batch_resample_clips_mix(self._h, int(in_channels), int(clip_channels), _dptr(m),
                                                   C.c_void_p(d_in), int(in_format), int(bool(in_interleaved)),
                                                   in_stride, ll(*[int(v) for v in in_lengths]), C.c_void_p(d_out),
                                                   int(out_format), int(bool(out_interleaved)), out_stride,
                                                   ll(*[int(v) for v in out_lengths]), C.c_void_p(stream))
        if p < 0:
            raise RuntimeError(self._err())
        self._produced = 0
        return p

    def resample_clips(self, x, lengths, out_lengths=None, out_format=None, out=None, clip_channels=1,
                       interleaved=False, out_interleaved=None, mix=None, drop_finished=False, longest_first=False,
                       in_format=None):
        """Whole clips of unequal length in one call (r8b_batch_resample_clips / _ex).  x: CUDA tensor [nch, T(, 3)] of
        int16 / int32 / float32 / float64 or packed 24-bit uint8, clip c in row c, its first lengths[c] <= T frames
        valid (the rest is never read).  out_lengths: frames wanted per clip, default int(lengths[c] * Dst / Src).
        Returns (view [nch, P(, 3)] of `out`, out_lengths), P = max(out_lengths): row c holds out_lengths[c] frames
        of clip c resampled, then zeros.  `out` (allocated if not given): [nch, >= P(, 3)] in `out_format` (default:
        the input's).  The object must be fresh (new, or clear()ed) and is fresh again afterwards.  Enqueues on
        torch's current stream and does not wait for it.
        clip_channels = K > 1: nch / K clips of K channels, clip i through channels i K .. i K + K - 1, one length per
        clip.  interleaved: x is [nclips, T, K(, 3)], frame-major as a decoder hands it over; otherwise the K rows of
        a clip are rows i K .. of [nch, T(, 3)].  out_interleaved (None: as the input): the result is a view
        [nclips, P, K(, 3)] of `out` [nclips, >= P, K(, 3)], or planar as above.
        mix: a [K, Kin] array-like of gains (r8b_batch_resample_clips_mix): the INPUT holds Kin channels per clip --
        x is [nclips, T, Kin(, 3)] with interleaved=True, [nclips * Kin, T(, 3)] planar -- and object channel i K + m
        receives sum over k of mix[m][k] x channel k of clip i; the output side is as without it (out_interleaved
        None: planar when K == 1, else as the input).  "Decode, mix down, resample": stereo int16 to mono is
        clip_channels=1, mix=[[.5, .5]], interleaved=True.
        drop_finished / longest_first: the flags of r8b_batch_resample_clips_sched -- finished clips leave the later
        steps, and the clips ride through the object longest first so that the finished ones are at its end; buffers
        and lengths stay in the caller's order (resample_clips_sched_ptr).
        in_format: PCM_U8, PCM_ULAW or PCM_ALAW for a uint8 x of one-byte samples, shaped as the other formats' tensors
        (no trailing axis of 3); None: by the dtype.  An out_format of these gives a uint8 result of that shape."""
        import torch
        fmt_of, dtype_of = _pcm_formats()
        K = int(clip_channels)
        assert 1 <= K and self.nch % K == 0
        nclips = self.nch // K
        interleaved = bool(interleaved)
        Kin = K
        if mix is not None:
            mix = np.ascontiguousarray(mix, dtype=np.float64)
            assert mix.ndim == 2 and mix.shape[0] == K and mix.shape[1] >= 1
            Kin = int(mix.shape[1])
            if out_interleaved is None:
                out_interleaved = interleaved and K > 1
        out_interleaved = interleaved if out_interleaved is None else bool(out_interleaved)
        in_format = _pcm_in_format(x, in_format, 3 if interleaved else 2, fmt_of)
        in_tail = (3,) if in_format == PCM_S24 else ()
        assert x.is_cuda and x.is_contiguous()
        if interleaved:
            assert x.dim() == 3 + len(in_tail) and x.shape[0] == nclips and tuple(x.shape[2:]) == (Kin,) + in_tail
        else:
            assert x.dim() == 2 + len(in_tail) and x.shape[0] == nclips * Kin and tuple(x.shape[2:]) == in_tail
        lengths = [int(v) for v in lengths]
        assert len(lengths) == nclips and all(0 <= v <= x.shape[1] for v in lengths)
        if out_lengths is None:
            src, dst = self._rates
            out_lengths = [self.clip_out_len(src, dst, v) for v in lengths]
        out_lengths = [int(v) for v in out_lengths]
        if out_format is None:
            out_format = in_format
        tail = (3,) if out_format == PCM_S24 else ()
        P = max(out_lengths) if out_lengths else 0
        if out_interleaved:
            rows, tail = nclips, (K,) + tail
        else:
            rows = self.nch
        if out is None:
            out = torch.empty((rows, max(P, 1)) + tail, dtype=dtype_of[out_format], device=x.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == dtype_of[out_format]
        assert out.shape[0] == rows and out.shape[1] >= P and tuple(out.shape[2:]) == tail
        dev = self._lib.r8b_batch_device(self._h)
        if x.device.index != dev or out.device.index != dev:
            raise ValueError("tensors on cuda:%s, the resampler lives on cuda:%d" % (x.device.index, dev))
        stream = torch.cuda.current_stream(x.device).cuda_stream
        flags = (CLIPS_DROP_FINISHED if drop_finished else 0) | (CLIPS_LONGEST_FIRST if longest_first else 0)
        if flags:
            p = self.resample_clips_sched_ptr(Kin if mix is not None else 0, K, mix, x.data_ptr(), in_format, interleaved,
                                              x.shape[1] * (Kin if interleaved else 1), None, lengths, out.data_ptr(),
                                              out_format, out_interleaved, out.shape[1] * (K if out_interleaved else 1),
                                              None, out_lengths, flags, stream)
        elif mix is not None:
            p = self.resample_clips_mix_ptr(Kin, K, mix, x.data_ptr(), in_format, interleaved,
                                            x.shape[1] * (Kin if interleaved else 1), lengths, out.data_ptr(),
                                            out_format, out_interleaved, out.shape[1] * (K if out_interleaved else 1),
                                            out_lengths, stream)
        elif K == 1 and not interleaved and not out_interleaved:
            p = self.resample_clips_ptr(x.data_ptr(), in_format, x.shape[1], lengths, out.data_ptr(), out_format,
                                        out.shape[1], out_lengths, stream)
        else:
            p = self.resample_clips_ex_ptr(K, x.data_ptr(), in_format, interleaved,
                                           x.shape[1] * (K if interleaved else 1), lengths, out.data_ptr(), out_format,
                                           out_interleaved, out.shape[1] * (K if out_interleaved else 1), out_lengths,
                                           stream)
        return out[:, :p], out_lengths

    def clip_pack_offsets(self, lengths, channels=1, align=1):
        """(offsets, total) of clips packed end to end (r8b_clip_pack_offsets): offsets[i] is the running sum of
        lengths[j] * channels, each base rounded up to a multiple of `align` elements; total: the elements the buffer
        needs."""
        n = len(lengths)
        ll = C.c_longlong * max(n, 1)
        off = ll()
        total = self._lib.r8b_clip_pack_offsets(n, ll(*[int(v) for v in lengths]), int(channels), int(align), off)
        if total < 0:
            raise ValueError("r8b_clip_pack_offsets: a negative length, channels < 1 or align < 1")
        return [int(off[i]) for i in range(n)], int(total)

    def resample_clips_packed_ptr(self, in_channels, clip_channels, mix, d_in, in_format, in_interleaved, in_stride,
                                  in_offsets, in_lengths, d_out, out_format, out_interleaved, out_stride, out_offsets,
                                  out_lengths, stream=0):
        """Raw device-pointer entry (r8b_batch_resample_clips_packed): resample_clips_mix_ptr / resample_clips_ex_ptr
        with an optional sequence of per-clip element offsets on each side.  in_offsets / out_offsets None: that side is
        strided as ever; given: clip i's region starts at offsets[i] and holds the clip's channels at the clip's own
        length, the stride is ignored.  mix None: no mix (in_channels 0 or clip_channels).  Returns P =
        max(out_lengths)."""
        nclips = self.nch // max(int(clip_channels), 1)
        assert len(in_lengths) == nclips and len(out_lengths) == nclips
        assert in_offsets is None or len(in_offsets) == nclips
        assert out_offsets is None or len(out_offsets) == nclips
        m = None
        if mix is not None:
            m = np.ascontiguousarray(mix, dtype=np.float64)
            assert m.shape == (int(clip_channels), int(in_channels))
        ll = C.c_longlong * nclips

        def arr(v):
            return None if v is None else ll(*[int(e) for e in v])
        p = self._lib.r8b_batch_resample_clips_packed(self._h, int(in_channels), int(clip_channels),
                                                      None if m is None else _dptr(m), C.c_void_p(d_in),
                                                      int(in_format), int(bool(in_interleaved)), int(in_stride),
                                                      arr(in_offsets), arr(in_lengths), C.c_void_p(d_out),
                                                      int(out_format), int(bool(out_interleaved)), int(out_stride),
                                                      arr(out_offsets), arr(out_lengths), C.c_void_p(stream))
        if p < 0:
            raise RuntimeError(self._err())
        self._produced = 0
        return p

    def resample_clips_sched_ptr(self, in_channels, clip_channels, mix, d_in, in_format, in_interleaved, in_stride,
                                 in_offsets, in_lengths, d_out, out_format, out_interleaved, out_stride, out_offsets,
                                 out_lengths, flags=0, stream=0):
        """Raw device-pointer entry (r8b_batch_resample_clips_sched): resample_clips_packed_ptr with `flags`, a sum of
        CLIPS_DROP_FINISHED (a step runs only the channels whose clips still owe outputs) and CLIPS_LONGEST_FIRST (the
        clips ride through the object sorted by output length, longest first: clip_schedule gives the order).  flags 0
        is resample_clips_packed_ptr.  Returns P = max(out_lengths)."""
        nclips = self.nch // max(int(clip_channels), 1)
        assert len(in_lengths) == nclips and len(out_lengths) == nclips
        assert in_offsets is None or len(in_offsets) == nclips
        assert out_offsets is None or len(out_offsets) == nclips
        m = None
        if mix is not None:
            m = np.ascontiguousarray(mix, dtype=np.float64)
            assert m.shape == (int(clip_channels), int(in_channels))
        ll = C.c_longlong * nclips

        def arr(v):
            return None if v is None else ll(*[int(e) for e in v])
        p = self._lib.r8b_batch_resample_clips_sched(self._h, int(in_channels), int(clip_channels),
                                                     None if m is None else _dptr(m), C.c_void_p(d_in),
                                                     int(in_format), int(bool(in_interleaved)), int(in_stride),
                                                     arr(in_offsets), arr(in_lengths), C.c_void_p(d_out),
                                                     int(out_format), int(bool(out_interleaved)), int(out_stride),
                                                     arr(out_offsets), arr(out_lengths), int(flags), C.c_void_p(stream))
        if p < 0:
            raise RuntimeError(self._err())
        self._produced = 0
        return p

    def clip_schedule(self, out_lengths, flags):
        """order[g] = the clip that rides in slot g of a resample_clips_sched_ptr call with these flags
        (r8b_clip_schedule): the identity, or with CLIPS_LONGEST_FIRST the clips by output length descending, equal
        lengths by ascending index"""
        n = len(out_lengths)
        order = (C.c_int * max(n, 1))()
        if self._lib.r8b_clip_schedule(n, (C.c_longlong * max(n, 1))(*[int(v) for v in out_lengths]), int(flags),
                                       order) != 0:
            raise ValueError("r8b_clip_schedule: a negative length or an unknown flag")
        return [int(order[i]) for i in range(n)]

    def resample_clips_packed(self, x, lengths, offsets=None, out_lengths=None, out_offsets=None, out_format=None,
                              out=None, clip_channels=1, interleaved=False, out_interleaved=None, mix=None,
                              out_packed=True, drop_finished=False, longest_first=False, in_format=None):
        """resample_clips for clips packed end to end in ONE buffer (r8b_batch_resample_clips_packed), as a loader holds
        them: x is a 1-D CUDA tensor of samples ([total, 3] uint8 for packed 24-bit), clip i's region starting at
        element offsets[i] and holding lengths[i] frames of Kin channels (Kin = clip_channels, or the mix's columns) --
        interleaved: frame-major; otherwise channel after channel at the clip's own length, as a [Kin, n] tensor.
        offsets None: clips end to end, clip_pack_offsets(lengths, Kin).  Regions may overlap; nothing outside them is
        read.  out_lengths, out_format, clip_channels, interleaved, out_interleaved and mix are resample_clips's.
        out_packed (default): returns (out, out_offsets, out_lengths) -- `out` a 1-D tensor ([total, 3] for 24-bit) in
        which clip i occupies the out_lengths[i] * K elements from out_offsets[i] (None: end to end) and nothing else
        is written; allocated with exactly that size if not given.
        out_packed=False: the output side is resample_clips's -- returns (padded view of `out`, out_lengths).
        drop_finished / longest_first: as in resample_clips (offsets and lengths stay in the caller's order).
        in_format: PCM_U8, PCM_ULAW or PCM_ALAW for a 1-D uint8 x of one-byte samples (None: by the dtype); an out_format
        of these gives a 1-D uint8 result."""
        import torch
        fmt_of, dtype_of = _pcm_formats()
        K = int(clip_channels)
        assert 1 <= K and self.nch % K == 0
        nclips = self.nch // K
        interleaved = bool(interleaved)
        Kin = K
        if mix is not None:
            mix = np.ascontiguousarray(mix, dtype=np.float64)
            assert mix.ndim == 2 and mix.shape[0] == K and mix.shape[1] >= 1
            Kin = int(mix.shape[1])
            if out_interleaved is None:
                out_interleaved = interleaved and K > 1
        out_interleaved = interleaved if out_interleaved is None else bool(out_interleaved)
        in_format = _pcm_in_format(x, in_format, 1, fmt_of)
        in_tail = (3,) if in_format == PCM_S24 else ()
        assert x.is_cuda and x.is_contiguous() and x.dim() == 1 + len(in_tail) and tuple(x.shape[1:]) == in_tail
        lengths = [int(v) for v in lengths]
        assert len(lengths) == nclips and all(v >= 0 for v in lengths)
        if offsets is None:
            offsets, _ = self.clip_pack_offsets(lengths, Kin)
        offsets = [int(v) for v in offsets]
        assert len(offsets) == nclips
        assert all(o >= 0 and (n == 0 or o + n * Kin <= x.shape[0]) for o, n in zip(offsets, lengths))
        if out_lengths is None:
            src, dst = self._rates
            out_lengths = [self.clip_out_len(src, dst, v) for v in lengths]
        out_lengths = [int(v) for v in out_lengths]
        if out_format is None:
            out_format = in_format
        tail = (3,) if out_format == PCM_S24 else ()
        P = max(out_lengths) if out_lengths else 0
        if out_packed:
            if out_offsets is None:
                out_offsets, total = self.clip_pack_offsets(out_lengths, K)
            else:
                out_offsets = [int(v) for v in out_offsets]
                total = max([o + n * K for o, n in zip(out_offsets, out_lengths)] + [0])
            if out is None:
                out = torch.empty((total,) + tail, dtype=dtype_of[out_format], device=x.device)
            assert out.dim() == 1 + len(tail) and out.shape[0] >= total and tuple(out.shape[1:]) == tail
            out_stride = 0
        else:
            assert out_offsets is None
            if out_interleaved:
                rows, tail = nclips, (K,) + tail
            else:
                rows = self.nch
            if out is None:
                out = torch.empty((rows, max(P, 1)) + tail, dtype=dtype_of[out_format], device=x.device)
            assert out.shape[0] == rows and out.shape[1] >= P and tuple(out.shape[2:]) == tail
            out_stride = out.shape[1] * (K if out_interleaved else 1)
        assert out.is_cuda and out.is_contiguous() and out.dtype == dtype_of[out_format]
        dev = self._lib.r8b_batch_device(self._h)
        if x.device.index != dev or out.device.index != dev:
            raise ValueError("tensors on cuda:%s, the resampler lives on cuda:%d" % (x.device.index, dev))
        stream = torch.cuda.current_stream(x.device).cuda_stream
        flags = (CLIPS_DROP_FINISHED if drop_finished else 0) | (CLIPS_LONGEST_FIRST if longest_first else 0)
        p = self.resample_clips_sched_ptr(Kin if mix is not None else 0, K, mix, x.data_ptr(), in_format, interleaved, 0,
                                          offsets, lengths, out.data_ptr(), out_format, out_interleaved, out_stride,
                                          out_offsets, out_lengths, flags, stream)
        if out_packed:
            return out, out_offsets, out_lengths
        return out[:, :p], out_lengths

    def process_host(self, x):
        """x: float64 numpy [nch, l]; synchronous; returns numpy [nch, n]."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.ndim == 2 and x.shape[0] == self.nch
        l = x.shape[1]
        cap = max(self.max_out_len, 1)
        out = np.empty((self.nch, cap), dtype=np.float64)
        n = self._lib.r8b_batch_process_host(self._h, _dptr(x), l, l, _dptr(out), cap)
        if n < 0:
            raise RuntimeError(self._err())
        return out[:, :n].copy()


class CDSPResampler(_Base):
    """Single stream through the reference's own five C-ABI symbols is `DLLResampler`; this class
    mirrors the C++ front-end, i.e. arbitrary ReqAtten (the DLL only offers three presets)."""

    def __init__(self, SrcSampleRate, DstSampleRate, aMaxInLen, ReqTransBand=2.0,
                 ReqAtten=206.91, ReqPhase=fprLinearPhase, lib=None, device=-1):
        super().__init__(lib)
        self._b = BatchResampler(SrcSampleRate, DstSampleRate, aMaxInLen, ReqTransBand, ReqAtten,
                                 nch=1, device=device, lib=self._lib, phase=int(ReqPhase))
        self.SrcSampleRate, self.DstSampleRate = SrcSampleRate, DstSampleRate
        self.MaxInLen = int(aMaxInLen)

    def getInLenBeforeOutPos(self, ReqOutPos):
        return self._b.getInLenBeforeOutPos(ReqOutPos)

    def getInputRequiredForOutput(self, ReqOutSamples):
        return self._b.getInputRequiredForOutput(ReqOutSamples)

    def getInLenBeforeOutStart(self, ReqOutPos=0):
        """reference CDSPResampler.h:443-464: feed one zero sample at a time until the output
        length passes ReqOutPos, then clear().  (Legacy/test helper; slow by design.)"""
        inc = 0
        outc = 0
        one = np.zeros(1)
        while True:
            outc += len(self.process(one))
            if outc > ReqOutPos:
                self.clear()
                return inc
            inc += 1

    def getMaxOutLen(self, MaxInLen=0):
        return self._b.max_out_len

    def getLatencyFrac(self):
        """reference CDSPResampler.h:491-494"""
        return self._b.getLatencyFrac()

    def getLatency(self):
        return 0

    def clear(self):
        self._b.clear()

    def process(self, ip0):
        x = np.ascontiguousarray(ip0, dtype=np.float64).reshape(1, -1)
        if self.SrcSampleRate == self.DstSampleRate:
            return x[0].copy()
        return self._b.process_host(x)[0]

    def oneshot(self, ip, oplen):
        """reference CDSPResampler.h:592-651."""
        ip = np.asarray(ip, dtype=np.float64)
        out = []
        got = 0
        pos = 0
        while got < oplen:
            if pos < len(ip):
                blk = ip[pos:pos + self.MaxInLen]
                pos += len(blk)
            else:
                blk = np.zeros(self.MaxInLen)
            y = self.process(blk)
            y = y[:oplen - got]
            out.append(y)
            got += len(y)
        self.clear()
        return np.concatenate(out) if out else np.zeros(0)


class CDSPResampler16(CDSPResampler):
    def __init__(self, SrcSampleRate, DstSampleRate, aMaxInLen, ReqTransBand=2.0, **kw):
        super().__init__(SrcSampleRate, DstSampleRate, aMaxInLen, ReqTransBand, 136.45, **kw)


class CDSPResampler16IR(CDSPResampler):
    def __init__(self, SrcSampleRate, DstSampleRate, aMaxInLen, ReqTransBand=2.0, **kw):
        super().__init__(SrcSampleRate, DstSampleRate, aMaxInLen, ReqTransBand, 109.56, **kw)


class CDSPResampler24(CDSPResampler):
    def __init__(self, SrcSampleRate, DstSampleRate, aMaxInLen, ReqTransBand=2.0, **kw):
        super().__init__(SrcSampleRate, DstSampleRate, aMaxInLen, ReqTransBand, 180.15, **kw)


class DLLResampler(_Base):
    """The five drop-in symbols exactly as a C host would call them (reference DLL/r8bsrc.h)."""

    r8brr16, r8brr16IR, r8brr24 = 0, 1, 2

    def __init__(self, SrcSampleRate, DstSampleRate, MaxInLen, ReqTransBand=2.0, Res=2, lib=None):
        super().__init__(lib)
        self._h = self._lib.r8b_create(SrcSampleRate, DstSampleRate, int(MaxInLen), ReqTransBand,
                                       int(Res))
        if not self._h:
            raise RuntimeError(self._err())

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.r8b_delete(self._h)
            self._h = None

    def inlen(self, n):
        return self._lib.r8b_inlen(self._h, int(n))

    def clear(self):
        self._lib.r8b_clear(self._h)

    def process(self, ip0):
        x = np.ascontiguousarray(ip0, dtype=np.float64)
        op = _capi.dp()
        n = self._lib.r8b_process(self._h, _dptr(x), len(x), C.byref(op))
        return np.ctypeslib.as_array(op, shape=(n,)).copy() if n > 0 else np.zeros(0)
