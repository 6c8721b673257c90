"""The census of the PCM twin: r8b_kernels.hip is compiled a second time (-DR8B_PCM_VARIANT) into a complete second copy
of k_conv, k_conv_big, k_whole, k_poly, k_poly_tiled, k_hbup, k_hbdown, k_hbcascade, k_hbdcascade and k_tail whose
src_load / dst_store decode and encode planar S16 / S24 / S32 / F32 caller buffers in place.  A planar PCM side also
sends the engine down paths no fp64 call takes: every single-sample load through the branchy src_load, the pair / vector
/ linear store forms off, last_block() answering kBlockAgain, the history copy always a k_tail launch that decodes PCM
into the ring.  Shared by the emulation tier (CPU) and the GPU tier (tests/test_pcm_twin.py) and, through --dump, by the
sanitizer program tests/cxx_pcm_twin.cpp.  Built on stage_census.py / kernel_census.py.

ENTRIES is written out below, each entry with the kernel whose twin it must run (`kernel`: the symbol of the chain's
first or last stage, whichever the entry is about); _complete() compares the names with the launch_symbol_note() names
of r8b_kernels.hip, so a kernel added to the twin's launchers fails the census until it has an entry.  k_tail has no
entry of its own: every entry asserts the counter tail_launches on its PCM-input pairs.

The stream of an entry: three rows of splitmix noise -- row 0 at the entry's `level` (authored so that the ORACLE's
output, fp64 rows in, passes full scale in some samples and in fewer than 5 % of them: --levels), row 1 at 2^-10, row
2 silent -- quantised to the input format first, so that decoding is exact.  Row 0 carries the input format's edge codes
once (EDGE_CODES).  The other two rows do not: the silent row is there to stay silent, and the bound of the quiet row is
2^-10 of full scale -- one full-scale code in it and the rounding error around that sample, 1e-16 of full scale, is 1e-13
of the row's level, the bound itself.  FLT_MAX stays with check_codec_edges for the same reason.  An integer format clips
a level above full scale, so its rows are that noise clipped.  Buffers are allocated to the byte: a row stride of the
call's length + 3 elements (S24 rows on every byte alignment, S16 rows on odd element strides), the last row without its
gap, an 8-byte guard behind it, gaps and guard filled with SENTINEL.

check_entry() states what an id asserts; check_codec_edges() the exact codec cases.

python tests/pcm_twin_cases.py --dump     one object per kernel as lines what|kind|a|b|c|d|i0|i1|maxin|options|first|last
python tests/pcm_twin_cases.py --levels   row 0's saturating share per entry with the oracle alone (authoring aid)"""
import math
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stage_census as S  # noqa: E402
from kernel_census import first_cut  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# r8b_pcm_format (include/r8bsrc.h)
F64, F32, S16, S24, S32 = 0, 1, 2, 3, 4
NAME = {F64: "F64", F32: "F32", S16: "S16", S24: "S24", S32: "S32"}
BYTES = {F64: 8, F32: 4, S16: 2, S24: 3, S32: 4}
SCALE = {S16: 32768.0, S24: 8388608.0, S32: 2147483648.0}
# each wide format on each side of every kernel, each side fp64 once (the twin's other branch of src_load / dst_store)
PAIRS = ((S16, S24), (S24, S32), (S32, F32), (F32, S16), (F64, S24), (S16, F64))
SENTINEL = 0xA5
GUARD = 8
NCH = S.NCH
QUIET = 2.0 ** -10
SEED = 977
# excused integer samples (check_entry 3.) per row: a condition, not a measurement
EXCUSED_CAP = {S16: 0.0, S24: 0.0, S32: 0.001}
assert NCH == 3 and S.LOUD == (0, 1)

TWIN_KERNELS = ("k_conv", "k_conv_big", "k_whole", "k_poly", "k_poly_tiled", "k_hbup", "k_hbdown", "k_hbcascade",
                "k_hbdcascade", "k_tail")

_FLT_MIN, _FLT_MAX, _DEN_MIN, _DEN_MAX = 2.0 ** -126, (2.0 - 2.0 ** -23) * 2.0 ** 127, 2.0 ** -149, 2.0 ** -126 - 2.0 ** -149


def _s24(u):
    return u - (1 << 24) if u >= 1 << 23 else u


# storage values a row carries once: integer codes, float values
EDGE_CODES = {
    S16: (-32768, 32767, -1, 1),
    S24: tuple(_s24(u) for u in (0x7FFFFF, 0x800000, 0xFFFFFF, 0x000000, 0x00FF00, 0xFF0000, 0x0000FF, 0x800001)),
    S32: (-(1 << 31), (1 << 31) - 1, -1, 1),
    F32: (0.0, -0.0, _DEN_MIN, _DEN_MAX, _FLT_MIN, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24),
    F64: (),
}
F32_CODEC_EDGES = EDGE_CODES[F32] + (-_DEN_MIN, _FLT_MAX, -_FLT_MAX)

# ---- the entries --------------------------------------------------------------------------------------------------------
# stand-alone convolvers (r8b_batch_create_stage kind 0: normalised frequency, transition band, attenuation, gain, up,
# down), option fast_conv = 0: the generic kernel at both edges at once
CONV_STAGES = (("1to1", (0, 0.459375, 2.0, 180.15, 1.0, 1, 1)), ("up2", (0, 0.5, 2.0, 180.15, 2.0, 2, 1)),
               ("down2", (0, 0.5, 2.0, 180.15, 1.0, 1, 2)), ("up3", (0, 1.0 / 3.0, 2.0, 136.45, 3.0, 3, 1)))
CONV_MAXIN = 1024
# the shortest and the longest bank of each family (stage_census part C)
BANKS = ((0, 8), (0, 30), (1, 6), (1, 24))
CASCADE_K = (3, 9, 10)             # cascades of 2, 8 and 8 + 1 half-band stages (stage_census part B)
CASCADE_ATTS = (109.56, 180.15)
# row 0 of the decimating chains: white noise keeps 2^-k of its power behind a decimation by 2^k, so a level that brings
# the output to full scale is one only the float formats hold; the integer formats' rows are that noise clipped
DOWN_LEVEL = {3: 2.1, 9: 17.0, 10: 24.0}


def _stage(kernel, desc, maxin, opts, tag, oracle, level, **kw):
    return dict(what="stage", kernel=kernel, desc=desc, maxin=maxin, opts=opts, id="%s-%s" % (kernel, tag), oracle=oracle,
                level=level, first=kernel, last=kernel, **kw)


def _chain(kernel, src, dst, maxin, tb, att, opts, tag, level, first, last, **kw):
    return dict(what="chain", kernel=kernel, src=src, dst=dst, maxin=maxin, tb=tb, att=att, opts=opts,
                id="%s-%s" % (kernel, tag), oracle="chain", level=level, first=first, last=last, **kw)


def _entries():
    es = []
    # k_hbup, k_hbdown: one row per tap count 1, 4, 5, 8, 9, 14 -- the three widths and their edges
    for col in S.A_COLUMNS:
        for kind in ("hbup", "hbdown"):
            a = [e for e in S.PART_A if e["kind"] == kind and e["ntaps"] == col["ntaps"]][0]
            es.append(_stage("k_" + kind, S.hb_descriptor(a), S.A_MAXIN, {}, "t%d" % a["ntaps"], kind,
                             1.02 if kind == "hbup" else 0.55, hb=a))
    # k_whole, k_poly_tiled (both fetch forms), k_poly
    for third, taps in BANKS:
        for c in S.PART_C:
            if (c["third"], c["taps"]) != (third, taps):
                continue
            if c["symbol"] == "k_whole" and (c["src"] == 88200.0) != (taps in (8, 24)):
                continue        # (one whole-step ratio per bank: up-sampling on two of them, decimating on the others)
            if c["symbol"] == "k_poly" and c["src"] != 96000.0:
                continue
            if c["symbol"] == "k_poly_tiled" and c["src"] == 44100.0:
                continue        # (96000 -> 44101: front fetch, 192000 -> 44101: the other form)
            es.append(_stage(c["symbol"], S.bank_descriptor(c), S.C_MAXIN, dict(c["opts"]), c["id"], "frac", 0.8, bank=c))
    # k_conv
    for tag, desc in CONV_STAGES:
        es.append(_stage("k_conv", desc, CONV_MAXIN, {"fast_conv": 0}, tag, "conv", 1.2 if desc[5] == 1 else 0.8))
    # (48000 -> 32000 is one 2 / 3 convolver; it takes the pair kernel by default, so the option here too)
    es.append(_chain("k_conv", 48000.0, 32000.0, 1024, 2.0, 136.45, {"fast_conv": 0}, "48000-32000", 0.8, "k_conv", "k_conv"))
    # k_conv_big: the two re-blocked ratios, planar PCM on both sides
    es.append(_chain("k_conv_big", 32000.0, 48000.0, 5000, 0.5, 180.15, {}, "32000-48000", 0.8, "k_conv_big", "k_conv_big"))
    es.append(_chain("k_conv_big", 64000.0, 48000.0, 7000, 0.6, 180.15, {}, "64000-48000", 0.8, "k_conv_big", "k_conv_big"))
    # k_hbcascade at the end of a chain, k_hbdcascade at its head; the convolver at the other end is the generic one
    # (fast_conv = 0), which takes its PCM side itself: no staging rows
    for k in CASCADE_K:
        for att in CASCADE_ATTS:
            u = [e for e in S.PART_B_UP if e["id"] == "up-k%d-a%g" % (k, att)][0]
            last = "k_hbcascade" if u["runs"][-1] > 1 else "k_hbup"
            # (8 + 1: the run of eight writes the ring of the ninth stage, a lone k_hbup, which is the stage that encodes)
            es.append(dict(_chain(last, u["src"], u["dst"], u["maxin"], S.TB, att, dict(u["opts"], fast_conv=0),
                                  u["id"], 0.8, "k_conv", last, part=u), id="k_hbcascade-" + u["id"]))
            d = [e for e in S.PART_B_DOWN if e["id"] == "down-k%d-a%g" % (k, att)][0]
            es.append(_chain("k_hbdcascade", d["src"], d["dst"], d["maxin"], S.TB, att, dict(d["opts"], fast_conv=0),
                             d["id"], DOWN_LEVEL[k], "k_hbdcascade", "k_conv", part=d))
    return es


ENTRIES = _entries()
# one stream per kernel with calls alternately fp64 and PCM (check_entry 5.)
ALTERNATING = ("k_hbup-t14", "k_hbdown-t9", "k_whole-bank2-t30-96000-44100", "k_poly_tiled-bank3-t24-96000-44101-tiled1",
               "k_poly-bank2-t8-96000-44101-tiled0", "k_conv-down2", "k_conv_big-32000-48000", "k_hbcascade-up-k9-a180.15",
               "k_hbdcascade-down-k9-a180.15")


def twin_launcher_symbols():
    """the kernels the twin's launchers start: the launch_symbol_note("k_...") names of the R8B_LAUNCH(...) functions of
    r8b_kernels.hip, which are compiled into both builds"""
    with open(os.path.join(ROOT, "r8brain-free-src_amd", "csrc", "r8b_kernels.hip")) as f:
        text = f.read()
    names = set()
    for m in re.finditer(r"void R8B_LAUNCH\((\w+)\)\([^)]*\)\s*\{(.*?)\n\}", text, re.S):
        names |= set(re.findall(r'launch_symbol_note\("(k_\w+)"\)', m.group(2)))
    return names


def _complete():
    """the written-out kernel names against the twin's launchers, both ways; the lists the issue asks for"""
    got = twin_launcher_symbols()
    assert got == set(TWIN_KERNELS) and len(TWIN_KERNELS) == 10, \
        "r8b_kernels.hip launches kernels the PCM census does not list (or the reverse): %s" % sorted(got ^ set(TWIN_KERNELS))
    assert {e["kernel"] for e in ENTRIES} == set(TWIN_KERNELS) - {"k_tail"}
    ids = [e["id"] for e in ENTRIES]
    assert len(set(ids)) == len(ids) and set(ALTERNATING) <= set(ids)
    assert {e["kernel"] for e in ENTRIES if e["id"] in ALTERNATING} == set(TWIN_KERNELS) - {"k_tail"}
    for kind in ("k_hbup", "k_hbdown"):
        assert [e["hb"]["ntaps"] for e in ENTRIES if e["kernel"] == kind and "hb" in e] == list(S.COLUMN_TAPS)
    for kernel, count in (("k_whole", 4), ("k_poly", 4), ("k_poly_tiled", 8), ("k_conv", 5), ("k_conv_big", 2),
                          ("k_hbcascade", 6), ("k_hbdcascade", 6)):
        assert sum(e["id"].startswith(kernel + "-") for e in ENTRIES) == count, kernel
    assert {(e["bank"]["third"], e["bank"]["taps"]) for e in ENTRIES if "bank" in e} == set(BANKS)
    assert {e["bank"]["front"] for e in ENTRIES if e["kernel"] == "k_poly_tiled"} == {True, False}
    assert [tuple(e["part"]["runs"]) for e in ENTRIES if e["id"].startswith("k_hbcascade-") and e["att"] == 109.56] == \
        [(2,), (8,), (8, 1)]
    # (the 180.15 dB decimating cascades are where down_runs cuts the run for LDS)
    assert any(e["part"]["runs"] != S.runs_of(e["part"]["nhb"]) for e in ENTRIES if e["kernel"] == "k_hbdcascade")
    assert {f for p in PAIRS for f in p} == {F64, F32, S16, S24, S32}
    assert all(sum(p[0] == f for p in PAIRS) >= 1 and sum(p[1] == f for p in PAIRS) >= 1 for f in (F32, S16, S24, S32))
    assert sum(p[0] == F64 for p in PAIRS) == 1 and sum(p[1] == F64 for p in PAIRS) == 1


_complete()


# ---- the numpy codec (tests/test_pcm.py) and byte-exact buffers ------------------------------------------------------------
def _codec():
    import test_pcm as P
    return P


def quantise(x, fmt):
    """x rounded to the format -> (storage values, the doubles they decode to)"""
    import numpy as np
    P = _codec()
    if fmt == F64:
        return x, x
    if fmt == F32:
        st = x.astype(np.float32)
        return st, st.astype(np.float64)
    st = P.np_encode(x, fmt)
    return st, P.np_decode(st, fmt)


def encode(v, fmt):
    """fp64 values -> storage values, by the documented convention"""
    import numpy as np
    if fmt == F32:
        with np.errstate(over="ignore"):
            return v.astype(np.float32)
    return _codec().np_encode(v, fmt)


def decode(st, fmt):
    import numpy as np
    return st.astype(np.float64) if fmt in (F32, F64) else _codec().np_decode(st, fmt)


_NP = {F64: "<f8", F32: "<f4", S16: "<i2", S32: "<i4"}


def to_bytes(st, fmt):
    """storage values [rows, n] -> uint8 [rows, n * bytes]"""
    import numpy as np
    if fmt == S24:
        return _codec().pack24(st).reshape(st.shape[0], -1)
    return np.ascontiguousarray(st.astype(_NP[fmt])).view(np.uint8).reshape(st.shape[0], -1)


def from_bytes(rows, fmt):
    import numpy as np
    if fmt == S24:
        return _codec().unpack24(rows.reshape(rows.shape[0], -1, 3))
    return np.ascontiguousarray(rows).view(_NP[fmt])


class Buffer:
    """`rows` rows of n elements on a stride of n + 3 elements, to the byte: the last row has no gap, GUARD bytes follow
    it; 8-byte aligned at its start as an fp64 view must be"""

    def __init__(self, rows, n, fmt, data=None):
        import numpy as np
        self.rows, self.n, self.bs, self.stride = rows, n, BYTES[fmt], n + 3
        self.size = ((rows - 1) * self.stride + n) * self.bs + GUARD
        self.host = np.empty(self.size // 8 + 1, dtype=np.float64).view(np.uint8)[:self.size]
        assert self.host.ctypes.data % 8 == 0
        self.host[:] = SENTINEL
        if data is not None:
            for c in range(rows):
                self.host[self._at(c):self._at(c) + n * self.bs] = data[c]

    def _at(self, c):
        return c * self.stride * self.bs

    def read(self, host, what):
        """-> the rows' bytes; every sentinel byte must be untouched"""
        import numpy as np
        mask = np.ones(self.size, dtype=bool)
        out = []
        for c in range(self.rows):
            mask[self._at(c):self._at(c) + self.n * self.bs] = False
            out.append(host[self._at(c):self._at(c) + self.n * self.bs])
        bad = np.nonzero(mask & (host != SENTINEL))[0]
        assert bad.size == 0, "%s: %d bytes outside the rows were written, first at byte %d of %d (row bytes %d, stride %d)" % (
            what, bad.size, bad[0], self.size, self.n * self.bs, self.stride * self.bs)
        return np.stack(out) if self.n else np.zeros((self.rows, 0), dtype=np.uint8)


class HostIO:
    """the emulation's "device memory" is host memory"""
    def __init__(self, tier):
        self.tier, self.stream = tier, 0

    def put(self, buf):
        return buf.host, buf.host.ctypes.data

    def back(self, h):
        return h


class DeviceIO(HostIO):
    def __init__(self, tier):
        self.tier, self.t = tier, tier.t
        self.stream = tier.t.cuda.current_stream().cuda_stream

    def put(self, buf):
        d = self.t.from_numpy(buf.host).to("cuda:0")
        return d, d.data_ptr()

    def back(self, h):
        return h.cpu().numpy()


def io_of(tier):
    return DeviceIO(tier) if tier.gpu else HostIO(tier)


def pcm_stream(io, b, st, fin, fout, lens, counts, what, fmts=None, checkpoint=None):
    """the storage values st [NCH, n] through process_pcm_ptr in calls of `lens`, planar both ways, every buffer to the
    byte; counts: the outputs every call must return.  fmts: per call (fin, fout, storage values) where the formats change
    from call to call.  checkpoint: (index of the call after which the state moves into a fresh object, its maker).
    -> (the output rows' bytes per call, the symbols every stage ran)"""
    pos, held, seen = 0, [], None
    for k, l in enumerate(lens):
        f_in, f_out, s_in = fmts[k] if fmts else (fin, fout, st)
        ib = Buffer(NCH, l, f_in, to_bytes(s_in[:, pos:pos + l], f_in))
        ob = Buffer(NCH, counts[k], f_out)
        ih, ip = io.put(ib)
        oh, op = io.put(ob)
        n = b.process_pcm_ptr(ip, f_in, False, ib.stride, l, op, f_out, False, ob.stride, io.stream)
        assert n == counts[k], "%s: call %d of %d samples returned %d outputs, the fp64 object %d" % (what, k, l, n, counts[k])
        if seen is None:
            seen = [set() for _ in b.stage_symbols()]
        for s, sym in zip(seen, b.stage_symbols()):
            s.add(sym)
        held.append((ob, oh, ih, ib, f_in))
        pos += l
        if checkpoint is not None and k == checkpoint[0]:
            blob = b.state_dict(io.stream)
            b = checkpoint[1]()
            b.load_state_dict(blob, io.stream)
    assert pos == (fmts[0][2] if fmts else st).shape[1]
    out = []
    for k, (ob, oh, ih, ib, f_in) in enumerate(held):
        out.append(ob.read(io.back(oh), "%s, output of call %d" % (what, k)))
        if io.tier.gpu and k < 2:
            ib.read(io.back(ih), "%s, input of call %d" % (what, k))      # (nobody writes the caller's input)
    return out, [s - {""} for s in seen], b


# ---- inputs and oracles ---------------------------------------------------------------------------------------------------
_INPUT = {}


def twin_input(n, level, fmt):
    """-> (storage values [NCH, n], the doubles they decode to): noise at (level, 2^-10, silence) quantised to `fmt`,
    row 0 carrying EDGE_CODES[fmt] once, from sample 211 on, 13 samples apart"""
    import numpy as np
    import r8b_oracle as O
    key = (n, level, fmt)
    if key not in _INPUT:
        x = np.stack([lv * O.splitmix_uniform(SEED + c, n) for c, lv in enumerate((level, QUIET, 0.0))])
        st, _ = quantise(x, fmt)
        st = np.array(st)
        for i, code in enumerate(EDGE_CODES[fmt]):
            if 211 + 13 * i < n:
                st[0, 211 + 13 * i] = code
        xd = np.array(decode(st, fmt))
        if len(_INPUT) >= 12:
            _INPUT.pop(next(iter(_INPUT)))
        st.setflags(write=False)
        xd.setflags(write=False)
        _INPUT[key] = (st, xd)
    return _INPUT[key]


_ORACLE = {}


def oracle_stream(e, x, lens, refwrap, key):
    """the entry's operation on the rows x through the calls `lens` by code that is not the code under test -> [NCH, total]:
    the longdouble formulas (half-band stages), RefStage / the numpy oracle's stage (banks, stand-alone convolvers), the
    compiled reference chain / the numpy oracle's (chains).  Shared by both tiers"""
    import numpy as np
    key = (e["id"], key, tuple(lens), refwrap is not None)
    if key in _ORACLE:
        return _ORACLE[key]
    kind = e["oracle"]
    if kind in ("hbup", "hbdown"):
        row = S.tables()["hb"][e["hb"]["fam"]][e["hb"]["steep"]][e["hb"]["row"]]
        f = S.hbup_formula if kind == "hbup" else S.hbdown_formula
        yo = np.stack([f(x[c].astype(np.longdouble), row["taps"]).astype(np.float64) for c in range(NCH)])
    elif kind in ("frac", "conv") and refwrap is not None:
        yo, _ = S._ref_stage_stream(refwrap, kind, e["desc"][1:], x, lens)
    else:
        import r8b_oracle as O
        rows = []
        for c in S.LOUD:
            if kind == "frac":
                st = O.make_stage(("frac", e["desc"][1], e["desc"][2], e["desc"][3], bool(e["desc"][5])))
            elif kind == "conv":
                st = O.ConvStage(*e["desc"][1:])
            elif refwrap is not None:
                st = refwrap.RefResampler(e["src"], e["dst"], e["maxin"], e["tb"], e["att"])
            else:
                st = O.OracleResampler(e["src"], e["dst"], e["maxin"], e["tb"], e["att"])
            ys, pos = [], 0
            for l in lens:
                ys.append(st.process(x[c, pos:pos + l]))
                pos += l
            rows.append(np.concatenate(ys))
        yo = np.stack(rows + [np.zeros(len(rows[0]))])
    if len(_ORACLE) >= 10:
        _ORACLE.pop(next(iter(_ORACLE)))
    _ORACLE[key] = yo
    return yo


class Tally:
    """what profiles/pcm_twin_census.txt records: excused ties and worst errors per output format"""

    def __init__(self):
        self.excused, self.samples, self.worst = {}, {}, {}

    def note_int(self, fmt, excused, samples, worst_lsb):
        self.excused[fmt] = self.excused.get(fmt, 0) + excused
        self.samples[fmt] = self.samples.get(fmt, 0) + samples
        self.worst[fmt] = max(self.worst.get(fmt, 0.0), worst_lsb)

    def note_float(self, fmt, peak):
        self.worst[fmt] = max(self.worst.get(fmt, 0.0), peak)

    def __str__(self):
        parts = []
        for f in sorted(self.worst):
            if f in SCALE:
                parts.append("%s excused %d of %d, worst |code - oracle * scale| %.9g LSB" % (
                    NAME[f], self.excused[f], self.samples[f], self.worst[f]))
            else:
                parts.append("%s worst own-level peak over tol_scale %.3g" % (NAME[f], self.worst[f]))
        return "; ".join(parts)


def judge_pcm(tally, got, yo, fout, levels, what):
    """3. the decoded / raw output `got` (storage values [NCH, n]) against the oracle yo.  Float formats: the values within
    RMS_TOL / PEAK_TOL times the row's level times tol_scale of the oracle rounded to the format.  Integer formats: the
    code is rint(oracle * scale), saturated; where oracle * scale lies within delta of a half-integer -- the saturation
    thresholds are two of them -- either neighbour; delta is the peak bound in LSBs; at most EXCUSED_CAP of a row"""
    import numpy as np
    from cases import PEAK_TOL, RMS_TOL, tol_scale
    assert got.shape == yo.shape, (what, got.shape, yo.shape)
    assert not np.any(got[2] != 0), "%s: silence in, code %r out" % (what, got[2][np.nonzero(got[2])[0][:1]])
    for c in S.LOUD:
        lv = levels[c]
        sc = tol_scale(float(np.sum((yo[c] / lv) ** 2)), yo.shape[1])
        if fout in SCALE:
            s = SCALE[fout]
            v = yo[c] * s
            want = np.clip(np.rint(v), -s, s - 1.0)
            delta = PEAK_TOL * lv * sc * s
            off = np.nonzero(got[c] != want)[0]
            lo = np.floor(v[off])
            near = np.abs(v[off] - lo - 0.5) <= delta
            either = (got[c][off] == np.clip(lo, -s, s - 1.0)) | (got[c][off] == np.clip(lo + 1.0, -s, s - 1.0))
            ok = near & either
            inside = np.abs(v) < s - 1.0
            worst = float(np.abs(got[c][inside] - v[inside]).max()) if inside.any() else 0.0
            tally.note_int(fout, int(ok.sum()), yo.shape[1], worst)
            assert ok.all(), "%s row %d -> %s: %d codes are not rint(oracle * scale), first at output %d: code %d, oracle * " \
                "scale %.17g (delta %.3g LSB)" % (what, c, NAME[fout], int((~ok).sum()), off[~ok][0], got[c][off[~ok][0]],
                                                  v[off[~ok][0]], delta)
            assert ok.sum() <= EXCUSED_CAP[fout] * yo.shape[1], "%s row %d -> %s: %d excused samples of %d" % (
                what, c, NAME[fout], int(ok.sum()), yo.shape[1])
        else:
            ref = encode(yo[c], fout).astype(np.float64)
            d = (got[c].astype(np.float64) - ref) / lv
            rr, pp = math.sqrt(float(np.mean(d * d))), float(np.abs(d).max())
            tally.note_float(fout, pp / sc)
            assert rr <= RMS_TOL * sc and pp <= PEAK_TOL * sc, "%s row %d -> %s: rms %.3g peak %.3g of its level, scale " \
                "%.2f, first at output %d" % (what, c, NAME[fout], rr, pp, sc, int(np.argmax(np.abs(d) > PEAK_TOL * sc)))


def saturating_share(yo):
    """share of row 0's oracle outputs an integer format saturates (|v| >= 1)"""
    import numpy as np
    return float(np.mean(np.abs(yo[0]) >= 1.0))


# ---- an entry -----------------------------------------------------------------------------------------------------------------
def maker(r8b, e, lib_kw):
    def make():
        if e["what"] == "stage":
            b = r8b.BatchResampler(0, 0, e["maxin"], nch=NCH, stage=e["desc"], **lib_kw)
        else:
            b = r8b.BatchResampler(e["src"], e["dst"], e["maxin"], e["tb"], e["att"], nch=NCH, **lib_kw)
        for k, v in e["opts"].items():
            b.set_option(k, v)
        b.set_option("timing", 1)
        return b
    return make


def entry_lens(b, e):
    """at least two whole calls; the convolver entries six blocks of their convolver at least, the chains enough behind
    their latency for a few hundred outputs (stage_census up_lens / down_lens)"""
    maxin = e["maxin"]
    if e["oracle"] in ("hbup", "hbdown"):
        return S.a_lens()
    if e["oracle"] == "frac":
        return [maxin, maxin] + first_cut(1500, maxin)
    if e["kernel"] in ("k_conv", "k_conv_big"):
        m = re.search(r"BlockConvolver: .* in_len=(\d+) io=(\d+)/\d+", b.describe())
        assert m, b.describe()
        per_block = int(m.group(1)) / int(m.group(2))
        n = max(int(math.ceil(6.5 * per_block)) + b.getInLenBeforeOutPos(0), 2 * maxin + 59)
        return [maxin, maxin] + first_cut(n - 2 * maxin, maxin)
    n = S.up_lens(b, e["part"])[0] if e["part"]["part"] == "Bup" else \
        b.getInLenBeforeOutPos(0) + 200 * e["part"]["ratio"] + 13
    return first_cut(max(n, 2 * maxin + 7), maxin)


def _expect(e, tier):
    """(first, last) symbols; the emulator's launcher reports both forms of the generic convolver as k_conv: there the
    re-blocked form shows in describe() (asserted in check_entry)"""
    f = lambda s: "k_conv" if s == "k_conv_big" and not tier.gpu else s      # noqa: E731
    return f(e["first"]), f(e["last"])


def _edges(seen):
    """the one symbol of the first and of the last stage that launched (a member of a cascade run launches nothing of its
    own: the run reports at its first stage)"""
    ran = [s for s in seen if s]
    assert ran and len(ran[0]) == 1 and len(ran[-1]) == 1, seen
    return next(iter(ran[0])), next(iter(ran[-1]))


def check_entry(r8b, tier, e, lib_kw, refwrap=None):
    """One entry with its six format pairs, planar both ways, on a three-row object with timing on.  Per pair:
      1. the twin ran: the edge stages' symbols are the entry's (`first` / `last`, one of them the entry's kernel); counter
         pcm_staged_sides stays 0 -- with a planar non-fp64 side and no staging the launcher's format dispatch can only have
         taken the _pcm build --; per-call output counts equal the fp64 object's; a PCM input leaves tail_launches > 0;
      2. bitwise against the fp64 path: an identical object fed the numpy-decoded rows through process(), its output
         encoded with the numpy codec of tests/test_pcm.py: every output byte equal, every sentinel and guard byte untouched;
      3. against an oracle that is not this code (oracle_stream, judge_pcm);
      4. another cut of the stream into calls (stage_census.second_cut) gives the same bytes -- except on the polynomial
         path (k_poly, k_poly_tiled), whose position counter restarts at call boundaries in the reference as here
         (stage_census.check_bank 3.): there the second cut's bytes are the encoded fp64 object's through the same calls;
      5. entries of ALTERNATING: one more stream whose calls are alternately fp64 and S16 -> S24, a checkpoint taken after
         a PCM call and loaded into a fresh object: the fp64 calls return the bits of the uninterrupted fp64 stream, the
         PCM calls their encoding.
    Row 0's level is held to its purpose with the oracle alone: on the pairs whose input format can hold it unclipped
    (F32, F64) the oracle's output passes full scale in some samples and in fewer than 5 % of them.
    Returns the Tally."""
    import numpy as np
    make = maker(r8b, e, lib_kw)
    io = io_of(tier)
    levels = (e["level"], QUIET, 0.0)
    b0 = make()
    lens = entry_lens(b0, e)
    n = sum(lens)
    if e["kernel"] == "k_conv_big":
        assert re.search(r"BlockConvolver: .* fft=32768/", b0.describe()), b0.describe()
    assert lens.count(e["maxin"]) >= 2 and 1 in lens and 2 in lens, (e["id"], lens)
    lens2 = S.second_cut(n, e["maxin"], lens, n - e["maxin"] - e["maxin"] // 3 - 5)
    tally, counts, fp64, fp64b = Tally(), None, {}, {}
    poly = "bank" in e and not e["bank"]["whole"]
    for fin, fout in PAIRS:
        what = "%s %s->%s" % (e["id"], NAME[fin], NAME[fout])
        st, x = twin_input(n, e["level"], fin)
        if fin not in fp64:
            b = b0 if not fp64 else make()
            yd, cn, seen = S.stream(tier, b, tier.put(x), lens)
            assert counts is None or cn == counts, (what, cn, counts)
            counts = cn
            assert _edges(seen) == _expect(e, tier), (what, seen)
            assert b.stat("pcm_staged_sides") == 0
            fp64[fin] = tier.host(yd)
            del yd
        y = fp64[fin]
        assert y.shape[1] == sum(counts) > 0 and np.isfinite(y).all() and not y[2].any(), what
        # 1., 2.
        b = make()
        got, seen, _ = pcm_stream(io, b, st, fin, fout, lens, counts, what)
        assert _edges(seen) == _expect(e, tier) and e["kernel"] in (e["first"], e["last"]), (what, seen)
        assert b.stat("pcm_staged_sides") == 0, (what, b.stat("pcm_staged_sides"))
        if fin != F64:
            assert b.stat("tail_launches") > 0, what
        if e["kernel"] == "k_poly_tiled":
            assert (b.stat("poly_front") > 0) == e["bank"]["front"], what
        got = np.concatenate(got, axis=1)
        want = to_bytes(encode(y, fout), fout)
        if not np.array_equal(got, want):
            c, j = np.nonzero(from_bytes(got, fout) != from_bytes(want, fout))
            raise AssertionError("%s: the twin's bytes are not the encoded fp64 path's, first (row, output): (%d, %d) of %d: %r "
                                 "against %r" % (what, c[0], j[0], len(c), from_bytes(got, fout)[c[0], j[0]],
                                                 from_bytes(want, fout)[c[0], j[0]]))
        # 3.
        yo = oracle_stream(e, x, lens, refwrap, fin)
        share = saturating_share(yo)
        assert share < 0.05 and (share > 0.0 or fin not in (F32, F64)), "%s: row 0 saturates in %.3g of its samples" % (what, share)
        judge_pcm(tally, from_bytes(got, fout), yo, fout, levels, what)
        # 4.
        if fin not in fp64b and (not fp64b or poly):
            y2d, c2, _ = S.stream(tier, make(), tier.put(x), lens2)
            fp64b[fin] = (tier.host(y2d) if poly else None, c2)
            assert sum(c2) == sum(counts)
        counts2 = next(iter(fp64b.values()))[1]
        got2, seen2, _ = pcm_stream(io, make(), st, fin, fout, lens2, counts2, what + ", second cut")
        assert _edges(seen2) == _expect(e, tier), (what, seen2)
        want2 = to_bytes(encode(fp64b[fin][0], fout), fout) if poly else got
        assert np.array_equal(np.concatenate(got2, axis=1), want2), "%s: the bytes depend on the cut into calls" % what
    # 5.
    if e["id"] in ALTERNATING:
        check_alternating(io, make, e, lens, counts, fp64[S16], n)
    return tally


def check_alternating(io, make, e, lens, counts, y, n):
    """5. calls alternately fp64 -> fp64 and S16 -> S24 on one object: the history copy alternates between the carried form
    / fold_tail and k_tail's decoding twin, the last block between ahead / parked and kBlockAgain; a checkpoint after the
    fourth call (a PCM one) moves the stream into a fresh object"""
    import numpy as np
    tier = io.tier
    what = e["id"] + ", formats alternating"
    st, x = twin_input(n, e["level"], S16)
    fmts = [(S16, S24, st) if k & 1 else (F64, F64, x) for k in range(len(lens))]
    assert len(lens) > 6 and fmts[3][0] == S16
    b = make()
    got, seen, last = pcm_stream(io, b, None, None, None, lens, counts, what, fmts=fmts, checkpoint=(3, make))
    assert last is not b and last.stat("pcm_staged_sides") == 0 and b.stat("pcm_staged_sides") == 0
    assert last.stat("tail_launches") > 0 and _edges(seen) == _expect(e, tier), (what, seen)
    pos = 0
    for k, cn in enumerate(counts):
        piece = y[:, pos:pos + cn]
        fout = fmts[k][1]
        want = to_bytes(encode(piece, fout), fout) if cn else np.zeros((NCH, 0), dtype=np.uint8)
        assert np.array_equal(got[k], want), "%s: call %d (%s) differs from the uninterrupted fp64 stream" % (what, k, NAME[fout])
        pos += cn


# ---- codec edges ------------------------------------------------------------------------------------------------------------
def encode_vector(fmt):
    """the vector of test_pcm_rounding_and_saturation scaled to the format: ties to even on both signs, +-1.0, 2.0, -3.0,
    scale - 1.5, -0.0; F32: a double that rounds to a denormal, one that overflows to infinity, the tie at FLT_MAX's
    upper edge, half-way cases between two floats"""
    import numpy as np
    if fmt == F32:
        return np.array([1.0, -1.0, 2.0, -3.0, -0.0, 1e-40, -3e-42, 2.0 ** -150, 3.0 * 2.0 ** -150, 3.5e38, -3.5e38,
                         _FLT_MAX + 2.0 ** 102, _FLT_MAX + 2.0 ** 102 - 2.0 ** 60, 1.0 + 2.0 ** -24, 1.0 + 3.0 * 2.0 ** -24,
                         -1.0 - 2.0 ** -24, 1.0 - 2.0 ** -25, 0.1, _FLT_MIN - 2.0 ** -150])
    s = SCALE[fmt]
    return np.array([0.5 / s, 1.5 / s, 2.5 / s, -0.5 / s, -1.5 / s, -2.5 / s, 1.0, -1.0, 2.0, -3.0, (s - 1.5) / s, -0.0,
                     0.25 / s, (s - 0.5) / s, -(s + 0.5) / s, (s - 1.0) / s, 0.4999999999 / s, 0.5000000001 / s])


def decode_codes(fmt):
    import numpy as np
    if fmt == S16:
        return np.arange(-32768, 32768, dtype=np.int64)
    if fmt == F32:
        return np.array(F32_CODEC_EDGES, dtype=np.float32)
    return np.array(EDGE_CODES[fmt], dtype=np.int64)


def check_codec_edges(r8b, tier, e, lib_kw):
    """A half-band up-sampler copies its input to its even outputs (stage_census.hbup_formula: y[2n] = x[n]), so the codec
    alone shows there, exactly, without an oracle.  Decode: every code of decode_codes(format) in, F64 out, the even
    outputs are np_decode of the codes bit for bit.  Encode: encode_vector(format) as F64 in, the format out, the even
    outputs are np_encode of the vector.  All inputs finite.  One row carries the values, one their negation where the
    format has it (floats), one is silent"""
    import numpy as np
    from nonfinite_cases import _bits
    assert e["kernel"] == "k_hbup"
    make, io, T, maxin = maker(r8b, e, lib_kw), io_of(tier), e["hb"]["ntaps"], e["maxin"]

    def run(st, fin, fout):
        m = st.shape[1]
        lens = [min(maxin, m - p) for p in range(0, m, maxin)]
        counts = S._counts(S.hbup_total, lens, T)
        b = make()
        got, seen, _ = pcm_stream(io, b, st, fin, fout, lens, counts, "%s codec %s->%s" % (e["id"], NAME[fin], NAME[fout]))
        assert seen == [{"k_hbup"}] and b.stat("pcm_staged_sides") == 0
        return from_bytes(np.concatenate(got, axis=1), fout)

    for fmt in (S16, S24, S32, F32):
        codes = decode_codes(fmt)
        pad = np.zeros(T + 5, dtype=codes.dtype)
        row = np.concatenate([codes, pad])
        st = np.stack([row, row[::-1].copy() if fmt != S16 else np.roll(row, 1), np.zeros_like(row)])
        y = run(st, fmt, F64)
        for c in (0, 1):
            want = decode(st[c][:len(row) - T], fmt)
            assert np.array_equal(_bits(y[c, 0:2 * len(want):2]), _bits(want)), "%s: %s codes decode wrongly, first %r" % (
                e["id"], NAME[fmt], st[c][np.nonzero(_bits(y[c, 0:2 * len(want):2]) != _bits(want))[0][:1]])
        assert not y[2].any()
        v = encode_vector(fmt)
        row = np.concatenate([v, np.zeros(T + 5)])
        x = np.stack([row, -row, np.zeros_like(row)])
        got = run(x, F64, fmt)
        for c in (0, 1):
            want = encode(x[c][:len(row) - T], fmt)
            g = got[c, 0:2 * len(want):2]
            same = np.array_equal(_bits(g.astype(np.float64)), _bits(want.astype(np.float64))) if fmt == F32 else \
                np.array_equal(g, want)
            assert same, "%s: F64 -> %s encodes %r as %r, the convention says %r" % (e["id"], NAME[fmt], x[c][:len(want)], g, want)
        assert not np.any(got[2] != 0)


# ---- the sanitizer program's table -------------------------------------------------------------------------------------------
DUMPED = ("k_hbup-t14", "k_hbdown-t9", "k_whole-bank2-t30-96000-44100", "k_poly_tiled-bank3-t24-96000-44101-tiled1",
          "k_poly-bank2-t8-96000-44101-tiled0", "k_conv-down2")
DUMPED_CHAINS = ("k_conv_big-32000-48000", "k_hbcascade-up-k9-a180.15", "k_hbdcascade-down-k9-a180.15")


def dump(out):
    """what|kind or 0|a|b|c|d|i0|i1|maxin|options|first stage's symbol|last stage's symbol"""
    def opts(o):
        return ",".join("%s=%d" % kv for kv in sorted(o.items()))
    for e in ENTRIES:
        if e["id"] in DUMPED:
            d = e["desc"]
            out.write("stage|%d|%r|%r|%r|%r|%d|%d|%d|%s|%s|%s\n" % (d[0], d[1], d[2], d[3], d[4], d[5], d[6], e["maxin"],
                                                                  opts(e["opts"]), e["first"], e["last"]))
        elif e["id"] in DUMPED_CHAINS:
            out.write("chain|0|%r|%r|%r|%r|0|0|%d|%s|%s|%s\n" % (e["src"], e["dst"], e["tb"], e["att"], e["maxin"],
                                                               opts(e["opts"]), e["first"], e["last"]))


assert {e["kernel"] for e in ENTRIES if e["id"] in DUMPED + DUMPED_CHAINS} == set(TWIN_KERNELS) - {"k_tail"}


def print_levels(out):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, ROOT)
    import importlib
    import cases
    import refwrap as R
    r8b = importlib.import_module("r8brain-free-src_amd")
    kw = {"lib": cases.emul_lib(test_hooks=True)}
    for e in ENTRIES:
        lens = entry_lens(maker(r8b, e, kw)(), e)
        _, x = twin_input(sum(lens), e["level"], F64)
        yo = oracle_stream(e, x, lens, R if R.available() else None, F64)
        out.write("%-46s level %.3g: %d calls, %d in, %d out, row 0 saturates in %.4f\n" % (
            e["id"], e["level"], len(lens), sum(lens), yo.shape[1], saturating_share(yo)))
        out.flush()


if __name__ == "__main__":
    if sys.argv[1:] == ["--dump"]:
        dump(sys.stdout)
    elif sys.argv[1:] == ["--levels"]:
        print_levels(sys.stdout)
    else:
        sys.exit("usage: python tests/pcm_twin_cases.py --dump | --levels")
