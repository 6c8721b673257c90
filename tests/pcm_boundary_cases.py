"""The census of the PCM boundary (tests/test_pcm_boundary.py): one entry per device symbol that r8b_pcm_dispatch.h can
start -- 8 ingest and 40 egress kernels of r8b_pcm.h and r8b_clip*.h -- the call of the public C ABI that reaches it, and
the numpy oracle every byte and meter is compared with.

The count, from pcm_in_dispatch / pcm_out_dispatch: ingest k_pcm_in, k_pcm_rows_in, k_clip_rows_in, k_clip_frames_in,
k_clip_mix_in and the three k_clip_packed_* forms (8); egress k_pcm_out, k_pcm_rows_out (2), <DITHER, METER> without
<false, false> of k_pcm_finish and k_pcm_rows_finish (6), all four <DITHER, METER> of k_clip_rows_out, k_clip_frames_out,
k_clip_packed_rows_out, k_clip_packed_frames_out (16), all eight <DITHER, METER, PAD> of k_clip_sched_rows_out and
k_clip_sched_frames_out (16): 48.  The build agrees (test_census_names_exactly_the_build), and NOT_REACHED is empty:
every form has a call.  What the ABI does NOT reach is a format under a form: DITHER_FORMATS says which formats TPDF
dither applies to, and r8b_capi.cpp (Batch::dithers, for batch_process_pcm and batch_resample_clips: `dither_mode != 0 &&
pcm_io_dithers(fmt)`) leaves the launch's dither clear for the others, so a <true, ...> form never meets F64, F32, mu-law
or A-law through the ABI -- such a call runs the <false, ...> sibling, which is what the ids assert for those formats
(expected_symbol).  tests/cxx_pcm_boundary.cpp starts those combinations through the launcher itself.

The oracle is the restatements the suite already holds -- pcm8_cases.decode / encode over tests/golden/g711.npz,
np_encode / np_dither of test_pcm_finish.py, np_mix of test_clip_mix.py -- and never the library: on the pass-through
leg (Src == Dst, no stage) the expected fp64 rows are the decoded, zero-padded [, mixed] input itself; behind a chain
(44100 -> 88200) they are this library's own fp64 output for those rows (F64 planar on both sides, a second object),
which the oracle then encodes.  Every comparison is exact.

Thread-to-sample maps (the lone-event sweep places its events by them; tid = 64 wave + lane, 256 threads):
  row kernels (k_pcm_rows_finish, k_clip_rows_out, k_clip_packed_rows_out, k_clip_sched_rows_out), a workgroup per
      chunk of 2048 frames of one row: frame f of the chunk on thread f mod 256 -- lane f mod 64, wave (f / 64) mod 4;
      a one-byte format on an aligned row: the four frames 4 g .. 4 g + 3 on thread g mod 256
  k_pcm_finish, a tile of 64 frames x 64 channels: element e = 64 c + f on thread e mod 256 -- lane f, wave c mod 4
  frame kernels (k_clip_frames_out, k_clip_packed_frames_out, k_clip_sched_frames_out), a tile of FT frames x K channels:
      element e = FT c + f on thread e mod 256; at K = 2 (FT = 1024) lane f mod 64, wave (f / 64) mod 4"""
import importlib

import numpy as np

import pcm8_cases as M
import test_clip_frames as F
import test_clip_mix as MX
import test_clip_packed as P
import test_pcm_finish as FIN
import r8b_oracle as O

r8b = importlib.import_module("r8brain-free-src_amd")

F64, F32, S16, S24, S32 = r8b.PCM_F64, r8b.PCM_F32, r8b.PCM_S16, r8b.PCM_S24, r8b.PCM_S32
U8, ULAW, ALAW = r8b.PCM_U8, r8b.PCM_ULAW, r8b.PCM_ALAW
FORMATS = [F64, F32, S32, S24, S16, U8, ULAW, ALAW]
FMT_NAME = {F64: "f64", F32: "f32", S32: "s32", S24: "s24", S16: "s16", U8: "u8", ULAW: "ulaw", ALAW: "alaw"}
BYTES = {F64: 8, F32: 4, S32: 4, S24: 3, S16: 2, U8: 1, ULAW: 1, ALAW: 1}
BITS = FIN.BITS
DITHER_FORMATS = (S16, S24, S32, U8)     # pcm_io_dithers (r8b_launch.h), restated
SENTINEL, SEED = 0xA5, FIN.SEED
FIRST_CHANNEL = 5
GUARD = 64                               # sentinel bytes in front of and behind every output buffer
DROP, ORDER = 1, 2
PASS, CHAIN = (44100.0, 44100.0), (44100.0, 88200.0)
LEGS = {"pass": PASS, "chain": CHAIN}
ATT = 136.45


# ---------------------------------------------------------------- the table
def _sym(name, *args):
    return name + ("<%s>" % ", ".join("true" if a else "false" for a in args) if args else "")


def _form(symbol, side, family, tiles, addr="strided", dither=False, meter=False, pad=False, mix=False):
    return {"symbol": symbol, "side": side, "family": family, "tiles": tiles, "addr": addr, "dither": dither,
            "meter": meter, "pad": pad, "mix": mix}


def _table():
    t = [_form("k_pcm_in", "in", "plain", True), _form("k_pcm_rows_in", "in", "plain", False),
         _form("k_clip_rows_in", "in", "clip", False), _form("k_clip_frames_in", "in", "clip", True),
         _form("k_clip_mix_in", "in", "clip", True, mix=True),
         _form("k_clip_packed_rows_in", "in", "clip", False, "packed"),
         _form("k_clip_packed_frames_in", "in", "clip", True, "packed"),
         _form("k_clip_packed_mix_in", "in", "clip", True, "packed", mix=True),
         _form("k_pcm_out", "out", "plain", True), _form("k_pcm_rows_out", "out", "plain", False)]
    dm = [(False, False), (False, True), (True, False), (True, True)]
    for name, tiles in (("k_pcm_finish", True), ("k_pcm_rows_finish", False)):
        t += [_form(_sym(name, d, m), "out", "finish", tiles, dither=d, meter=m) for d, m in dm[1:]]
    for name, tiles, addr in (("k_clip_rows_out", False, "strided"), ("k_clip_frames_out", True, "strided"),
                              ("k_clip_packed_rows_out", False, "packed"), ("k_clip_packed_frames_out", True, "packed")):
        t += [_form(_sym(name, d, m), "out", "clip", tiles, addr, d, m, pad=addr == "strided") for d, m in dm]
    for name, tiles in (("k_clip_sched_rows_out", False), ("k_clip_sched_frames_out", True)):
        t += [_form(_sym(name, d, m, p), "out", "clip", tiles, "sched", d, m, p) for d, m in dm for p in (False, True)]
    return t


FORMS = _table()
SYMBOLS = [f["symbol"] for f in FORMS]
assert len(FORMS) == len(set(SYMBOLS)) == 48
# a form no call of include/r8bsrc.h reaches: {"symbol", "reason", "cite"}.  None.
NOT_REACHED = []
# (20, not the 19 a first reading of the dispatch gives: 2 x 2 finishing, 4 x 2 clip and 2 x 4 scheduled instances)
METERED = [f for f in FORMS if f["meter"]]
assert len(METERED) == 20


def expected_symbol(form, fmt):
    """the form a call with the entry's settings runs in format `fmt`: its own, or -- DITHER set and a format dither does
    not apply to -- the <false, ...> sibling (r8b_capi.cpp clears the launch's dither), which without meters is the
    plain kernel on the non-clip side"""
    if not form["dither"] or fmt in DITHER_FORMATS:
        return form["symbol"]
    name = form["symbol"].split("<")[0]
    if form["family"] == "finish":
        return _sym(name, False, True) if form["meter"] else name.replace("_finish", "_out")
    return _sym(name, False, form["meter"], form["pad"]) if form["addr"] == "sched" else _sym(name, False, form["meter"])


def emul_name(member, args):
    """the symbol an EmulPcm member instance notes (tests/emul/emul_pcm.cpp), from its name and template arguments as
    `nm -C` prints them"""
    b = {"true": True, "false": False}
    if member.startswith("pcm_"):
        return _sym("k_" + member, *[b[a] for a in args])
    kind = member[len("clip_"):]
    base, rest = args[0].split("::")[-1], [b[a] for a in args[1:]]
    if not rest:
        return "k_clip_" + ("packed_" if base == "ClipPacked" else "") + kind
    pad, d, m = rest
    if base == "ClipSched":
        return _sym("k_clip_sched_" + kind, d, m, pad)
    return _sym("k_clip_" + ("packed_" if base == "ClipPacked" else "") + kind, d, m)


def tile_frames(K):
    """frames of a clip tile of K channels: the largest power of two with FT K <= 2048, 64 at least"""
    ft = 64
    while 2 * ft * K <= 2048:
        ft *= 2
    return ft


ROW_CHUNK = 2048


def odd4(s):
    """s rounded up to 1 mod 4: planar rows that far apart start on every byte alignment of a one-byte format"""
    return s + (1 - s) % 4


# ---------------------------------------------------------------- the oracle
def to_units(q, fmt):
    """sample values (ints of an integer format, floats) [...] -> bytes [..., B]"""
    if fmt == S24:
        return F.pack24(q)
    if fmt in (U8, ULAW, ALAW):
        return np.asarray(q, dtype=np.uint8)[..., None]
    dt = {F64: "<f8", F32: "<f4", S16: "<i2", S32: "<i4"}[fmt]
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.ascontiguousarray(np.asarray(q).astype(dt))
    return a.view(np.uint8).reshape(a.shape + (BYTES[fmt],))


def decode_units(u, fmt):
    """bytes [..., B] -> fp64 [...]"""
    u = np.ascontiguousarray(u)
    if fmt in (U8, ULAW, ALAW):
        return M.decode(u[..., 0], fmt)
    if fmt == S24:
        return FIN.unpack24(u).astype(np.float64) / float(1 << 23)
    dt = {F64: "<f8", F32: "<f4", S16: "<i2", S32: "<i4"}[fmt]
    a = u.view(dt).reshape(u.shape[:-1])
    return a.astype(np.float64) / float(1 << (BITS[fmt] - 1)) if fmt in BITS else a.astype(np.float64)


def encode_units(v, fmt, d=None):
    """fp64 [...] -> (bytes [..., B], clipped flags); d: dither in LSB or None"""
    with np.errstate(invalid="ignore", over="ignore"):
        if fmt in (U8, ULAW, ALAW):
            q, clipped = M.encode(v, fmt, d)
        else:
            q, clipped = FIN.np_encode(v, fmt, d if fmt in BITS else None)
    return to_units(q, fmt), clipped


def dither_of(form, fmt, first_row, nrows, j0, n):
    """[nrows, n]: the dither of object channels FIRST_CHANNEL + first_row .. at clip / stream frames j0 .., or None"""
    if not form["dither"] or fmt not in DITHER_FORMATS:
        return None
    return FIN.np_dither(SEED, FIRST_CHANNEL + first_row, nrows, j0, n)


def meters_of(v, lens, fmt, d):
    """the meters of fp64 rows v [nch, >= max(lens)], frames below lens[c], encoded to `fmt` with dither d (or None)"""
    nch = v.shape[0]
    peak, clipped, nonfinite = np.zeros(nch), np.zeros(nch, dtype=np.int64), np.zeros(nch, dtype=np.int64)
    for c in range(nch):
        w = v[c, :lens[c]]
        a = np.abs(w[~np.isnan(w)])
        peak[c] = a.max() if a.size else 0.0
        clipped[c] = np.count_nonzero(encode_units(w, fmt, None if d is None else d[c, :lens[c]])[1])
        nonfinite[c] = np.count_nonzero(~np.isfinite(w))
    return {"peak": peak, "clipped": clipped, "nonfinite": nonfinite}


def assert_meters(got, want, what):
    for name in ("peak", "clipped", "nonfinite"):
        assert np.array_equal(got[name].view(np.int64), want[name].view(np.int64)), (what, name, got[name], want[name])


def assert_bytes(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "bytes differing", bad.size, "first at", int(bad[0]), "of", got.size)


# ---------------------------------------------------------------- samples
def edges(fmt):
    """the loud row's head: the codec's edges, half a step either side of saturation, and what is no number"""
    s = float(1 << (BITS[fmt] - 1)) if fmt in BITS else 128.0 if fmt == U8 else 32768.0
    return np.array([1.0, -1.0, 1.0 - 1.0 / s, -(1.0 - 1.0 / s), (s - 1.0 + 0.49) / s, (s - 1.0 + 0.51) / s,
                     -(s + 0.49) / s, -(s + 0.51) / s, (s - 0.5) / s, -(s + 0.5) / s, 0.0, -0.0, np.inf, -np.inf, np.nan,
                     1e300, -1e300, 5e-324, 2.0 ** -1030, 0.75, 2.0])


_NOISE = {}


def noise(nrows, n, seed=700):
    """-6 dBFS noise [nrows, n], computed once per shape and left unchanged"""
    k = (nrows, n, seed)
    if k not in _NOISE:
        x = 0.5 * np.stack([O.splitmix_uniform(seed + c, max(n, 1)) for c in range(nrows)])[:, :n]
        x.setflags(write=False)
        _NOISE[k] = x
    return _NOISE[k]


def egress_values(nrows, n, fmt, finite, loud_row=0):
    """fp64 rows for an egress form: the noise, and a loud row -- the format's edges (pass-through leg) or the noise
    times 2.5, which saturates (behind a chain, where every sample must stay a finite number)"""
    x = np.array(noise(nrows, n))
    if finite:
        x[loud_row] *= 2.5
    else:
        e = edges(fmt)[:n]
        x[loud_row, :len(e)] = e
    return x


def ingest_units(nrows, n, fmt, finite, seed=41):
    """bytes [nrows, n, B] of an ingest form's input in `fmt`: every code of an integer format at random (row 0 opens with
    all 256 codes of a one-byte format), the float formats as egress_values"""
    if fmt in (F64, F32):
        return to_units(egress_values(nrows, n, fmt, finite), fmt)
    u = np.random.RandomState(seed + fmt).randint(0, 256, size=(nrows, n, BYTES[fmt])).astype(np.uint8)
    if BYTES[fmt] == 1:
        k = min(n, 256)
        u[0, :k, 0] = np.arange(256, dtype=np.uint8)[:k]
    else:
        s = 1 << (BITS[fmt] - 1)
        e = to_units(np.array([-s, s - 1, 0, -1, 1]), fmt)[:n]
        u[0, :len(e)] = e
    return u


def garbage(fmt):
    """the sample that fills what a call must not read: NaN, or the format's largest code"""
    if fmt in (F64, F32):
        return to_units(np.array(np.nan), fmt)
    if fmt in BITS:
        return to_units(np.array((1 << (BITS[fmt] - 1)) - 1), fmt)
    return np.array([M.LARGEST[fmt]], dtype=np.uint8)


# ---------------------------------------------------------------- tiers and buffers
class Tier(M.Tier):
    """pcm8_cases.py's tiers; objects are kept per (channels, leg, MaxInLen) -- a clip call leaves its object as clear()
    does, the streaming ids clear() theirs -- with "timing" on, and the finish settings are made per call"""

    def __init__(self, lib):
        super().__init__(lib)
        self._objects = {}

    def obj(self, nch, leg, chunk, form=None, tag=None):
        k = (nch, leg, chunk, tag)
        if k not in self._objects:
            a = self.make(nch, LEGS[leg][0], LEGS[leg][1], chunk, att=ATT)
            a.set_option("timing", 1)
            self._objects[k] = a
        a = self._objects[k]
        a.clear()
        dither = form is not None and form["dither"]
        meter = form is not None and form["meter"]
        a.set_dither(r8b.DITHER_TPDF if dither else r8b.DITHER_NONE, SEED, FIRST_CHANNEL)
        a.enable_meters(meter)
        if meter:
            a.read_meters(reset=True)
        return a

    def guarded(self, nbytes, lead=0):
        """(the whole allocation, its view of nbytes bytes): sentinels everywhere, GUARD bytes around the view, `lead`
        more in front (the view's byte alignment)"""
        whole = self.sentinels(GUARD + lead + nbytes + GUARD)
        return whole, self.view(whole, GUARD + lead, GUARD + lead + nbytes)

    def check_guarded(self, whole, want, lead, what):
        got = self.host(whole)
        full = np.full(got.size, SENTINEL, dtype=np.uint8)
        full[GUARD + lead:GUARD + lead + want.size] = want
        assert_bytes(got, full, what)


# ---------------------------------------------------------------- the plain and the finishing forms
PLAIN_ROWS = {"pass": (4, 4099, [0, 1, 2047, 2048, 2049, 4097, 5, 9, 12]), "chain": (3, 1499, [1499, 1499, 1, 1498, 3])}
PLAIN_TILES = {"pass": ([1, 63, 64, 65, 70], 131, [1, 63, 64, 65, 129]), "chain": ([65], 1499, [1499, 1499, 1, 63, 129])}


def _lay_plain(rows, interleaved, stride):
    """[nch, n, B] -> the buffer's bytes: frame-major [n, nch], or planar rows `stride` samples apart, garbage between"""
    nch, n, B = rows.shape
    if interleaved:
        return np.ascontiguousarray(rows.transpose(1, 0, 2)).reshape(-1)
    buf = np.empty((nch, stride, B), dtype=np.uint8)
    buf[:] = rows[0, 0] if n else 0
    buf[:, :n] = rows
    return buf.reshape(-1)


def check_plain(tier, form, fmt, leg):
    """one plain / finishing form in one format on one leg: a stream of calls on one object.  Asserted per call: both
    symbols, every byte of the output buffer and of the GUARD bytes around it (planar rows lie `n + 1`, `n + 2` ...
    samples apart so that one-byte rows start on every byte alignment, and the slack keeps its sentinels), the meters"""
    ingest = form["side"] == "in"
    chans, chunk, lengths = (PLAIN_TILES if form["tiles"] else PLAIN_ROWS)[leg]
    want_sym = expected_symbol(form, fmt)
    for nch in (chans if form["tiles"] else [chans]):
        a = tier.obj(nch, leg, chunk, form)
        b = tier.obj(nch, leg, chunk, tag="fp64") if leg == "chain" else None      # (the fp64 path: a second object)
        frame0, lead = 0, 0
        for l in lengths:
            in_fmt, out_fmt = (fmt, F64) if ingest else (F64, fmt)
            units = ingest_units(nch, l, fmt, leg == "chain") if ingest else to_units(
                egress_values(nch, l, fmt, leg == "chain", nch - 1), F64)
            v = decode_units(units, in_fmt)
            in_il = ingest and form["tiles"]
            in_stride = nch if in_il else odd4(l + 1)
            xin = tier.buf(_lay_plain(units, in_il, in_stride))
            if b is None:
                y = v
            else:
                x64 = tier.buf(np.ascontiguousarray(v))
                cap = max(b.max_out_len, 1)
                o64 = tier.buf(np.zeros((nch, cap)))
                nb = b.process_pcm_ptr(tier.ptr(x64), F64, False, l, l, tier.ptr(o64), F64, False, cap)
                y = tier.host(o64).view(np.float64).reshape(nch, cap)[:, :nb].copy()
            n = y.shape[1]
            out_il = (not ingest) and form["tiles"]
            out_stride = nch if out_il else odd4(n + 1)
            d = None if ingest else dither_of(form, fmt, 0, nch, frame0, n)
            enc, _ = encode_units(y, out_fmt, d)
            B = BYTES[out_fmt]
            if out_il:
                want = np.ascontiguousarray(enc.transpose(1, 0, 2)).reshape(-1)
            else:
                w = np.full((nch, out_stride, B), SENTINEL, dtype=np.uint8)
                w[:, :n] = enc
                want = w.reshape(-1)[:((nch - 1) * out_stride + n) * B] if nch else w.reshape(-1)
            lead = (lead + 1) % 4 if B == 1 else 0
            whole, out = tier.guarded(max(want.size, 8), lead * B)
            what = (form["symbol"], FMT_NAME[fmt], leg, "channels", nch, "frames", l)
            got_n = a.process_pcm_ptr(tier.ptr(xin), in_fmt, in_il, in_stride, l, tier.ptr(out), out_fmt, out_il, out_stride)
            assert got_n == n, (what, got_n, n)
            pad = np.full(max(want.size, 8), SENTINEL, dtype=np.uint8)
            pad[:want.size] = want
            sym = a.boundary_symbols()
            if l == 0:
                assert sym == ("", ""), (what, sym)
            elif leg == "pass":
                assert sym == ((want_sym, "k_pcm_rows_out") if ingest else ("k_pcm_rows_in", want_sym if n else "")), (what, sym)
            else:
                # (behind a chain a planar side may be converted by the stage itself: then nothing is launched for it.
                # An interleaved side, a one-byte format, meters and a dither that applies always launch)
                must = form["tiles"] or BYTES[fmt] == 1 or form["meter"] or (form["dither"] and fmt in DITHER_FORMATS)
                mine = sym[0 if ingest else 1]
                assert mine == want_sym or (not must and mine == "") or (n == 0 and not ingest), (what, sym)
                assert sym[1 if ingest else 0] == "", (what, sym)
            tier.check_guarded(whole, pad, lead * B, what)
            if form["meter"]:
                assert_meters(a.read_meters(reset=True), meters_of(y, [n] * nch, fmt, d), what)
            frame0 += n
        assert frame0 > 100, (form["symbol"], leg, frame0)


# ---------------------------------------------------------------- the clip forms
NCLIPS = 6
CLIP_KS = {False: [1, 3], True: [2, 3, 7, 15, 16, 17, 31, 32, 33, 64]}      # by form["tiles"]
MIX_KS = [(2, 1), (6, 2), (64, 2), (6, 1)]                                # (Kin, K)


def clip_lengths(FT, leg):
    """(in_len, out_len) of the six clips around a tile (or row chunk) of FT frames: clips that end one short of, at and
    one past a tile's end; outputs shorter and longer than what the input yields -- padding begins inside a tile (FT - 2),
    at a tile's first frame with a whole tile of padding behind it (FT), and an empty clip asked for three frames"""
    in_len = [0, 1, FT - 1, FT, FT + 1, 2 * FT + 1]
    if leg == "pass":
        return in_len, [3, 2 * FT + 1, FT - 2, FT, FT + 1, 2 * FT + 1]
    return in_len, [3, 4 * FT + 1, FT - 2, FT, 2 * FT + 2, 4 * FT + 2]


def mix_matrix(K, Kin):
    """gains of 0, +-1/4 and +-1/2 (every product exact: multiply-then-add and fma agree), a zero in every row"""
    j = (np.arange(K * Kin) * 3 + 1) % 5 - 2
    return (j / 4.0).reshape(K, Kin)


_REF64 = {}


def chain_rows(tier, K, v, in_len, out_len, chunk, key):
    """this library's fp64 output [nch, P] for the zero-padded fp64 rows v behind the chain: planar F64 on both sides,
    flags 0, a second object; once per tier and case"""
    k = (tier.gpu, K, key, tuple(in_len), tuple(out_len), chunk)
    if k not in _REF64:
        nch, Pmax = v.shape[0], max(out_len)
        b = tier.obj(nch, "chain", chunk)
        T = v.shape[1]
        xin, out = tier.buf(np.ascontiguousarray(v)), tier.buf(np.zeros((nch, Pmax)))
        assert b.resample_clips_sched_ptr(0, K, None, tier.ptr(xin), F64, False, T, None, in_len, tier.ptr(out), F64, False,
                                          Pmax, None, out_len) == Pmax
        y = tier.host(out).view(np.float64).reshape(nch, Pmax).copy()
        y.setflags(write=False)
        _REF64[k] = y
    return _REF64[k]


def _lay_clips(units, Kc, interleaved, packed, lengths):
    """the input buffer of a clip call: (bytes, stride, offsets or None); garbage wherever no clip's valid frame lies"""
    if packed:
        buf, off = P.pack_in(units, Kc, interleaved, lengths)
        return buf, 0, off
    buf, stride = F.lay_in(units, Kc, interleaved)
    return buf, stride, None


def _want_clips(ref, K, B, interleaved, packed, out_len, pad_unit):
    """the expected output buffer: (bytes, stride, offsets or None) from the rows' bytes ref [nch, P, B] (valid frames
    only are read).  A strided side: padding (`pad_unit`) up to P, then sentinels in the stride's slack; a packed side:
    the regions alone, sentinels in the gaps"""
    nch, Pmax = ref.shape[0], max(out_len)
    nclips = nch // K
    if packed:
        off, total = P.pack_offsets([n * K for n in out_len], P.ORDER[::-1], P.GAPS[::-1])
        return P.pack_out(ref.reshape(nch, Pmax * B), K, B, interleaved, out_len, off, total), 0, off
    full = np.empty((nch, Pmax, B), dtype=np.uint8)
    full[:] = pad_unit
    for i, n in enumerate(out_len):
        full[i * K:(i + 1) * K, :n] = ref[i * K:(i + 1) * K, :n]
    if interleaved:
        stride = Pmax * K + 37
        w = np.full((nclips, stride, B), SENTINEL, dtype=np.uint8)
        w[:, :Pmax * K] = full.reshape(nclips, K, Pmax, B).transpose(0, 2, 1, 3).reshape(nclips, Pmax * K, B)
    else:
        stride = odd4(Pmax + 37)
        w = np.full((nch, stride, B), SENTINEL, dtype=np.uint8)
        w[:, :Pmax] = full
    return w.reshape(-1), stride, None


def check_clip(tier, form, fmt, leg, K, Kin=0):
    """one clip form in one format on one leg at K channels per clip (Kin: a mixing ingest's input channels): one call of
    r8b_batch_resample_clips_sched on six clips.  The side under test has the form's layout and addressing, the other
    side is planar strided F64.  Asserted: both symbols, every byte of the output buffer and the GUARD bytes around it,
    the meters."""
    ingest = form["side"] == "in"
    sched = form["addr"] == "sched"
    Kc = Kin if form["mix"] else K
    unit = ROW_CHUNK if not form["tiles"] else tile_frames(Kc)
    # (a mixing ingest whose layout is planar runs the same tile kernel: Kin == 6 into K == 1 takes it)
    in_len, out_len = clip_lengths(unit, leg)
    chunk = unit // 2 + 3
    nch, Pmax, T = NCLIPS * K, max(out_len), (max(in_len) + 4) // 4 * 4
    flags = (ORDER | DROP) if sched else 0
    fin = leg == "chain"
    what = (form["symbol"], FMT_NAME[fmt], leg, "K", K, "Kin", Kin)
    # the input side
    if ingest:
        il = form["tiles"] and not (form["mix"] and (Kin, K) == (6, 1))
        units = ingest_units(NCLIPS * Kc, T, fmt, fin)
        in_fmt, out_fmt = fmt, F64
    else:
        il = False
        units = to_units(egress_values(NCLIPS * Kc, T, fmt, fin, 5 * K), F64)
        in_fmt, out_fmt = F64, fmt
    v = decode_units(units, in_fmt)
    for r, n in enumerate(F.rows_of(in_len, Kc)):
        v[r, n:] = 0.0
        units[r, n:] = garbage(in_fmt)
    Mx = mix_matrix(K, Kin) if form["mix"] else None
    if Mx is not None:
        v = MX.np_mix(v, Mx)
    xb, in_stride, in_off = _lay_clips(units, Kc, il, ingest and form["addr"] == "packed", in_len)
    # the fp64 rows the egress encodes
    if leg == "pass":
        y = np.zeros((nch, Pmax))
        y[:, :min(Pmax, T)] = v[:, :min(Pmax, T)]
    else:
        # (an ordered call lets the clips ride longest first, ties by index, and a pair kernel rounds a channel with its
        # partner: the fp64 path is GIVEN the clips in that order, as tests/test_clip_sched.py does)
        order = sorted(range(NCLIPS), key=lambda i: -out_len[i]) if sched else list(range(NCLIPS))
        rows = [i * K + k for i in order for k in range(K)]
        y = chain_rows(tier, K, v[rows], [in_len[i] for i in order], [out_len[i] for i in order], chunk,
                       (form["side"], FMT_NAME[fmt] if ingest else "egress", Kin))[np.argsort(rows)]
    # the output side
    out_il = (not ingest) and form["tiles"]
    out_packed = (not ingest) and (form["addr"] == "packed" or (sched and not form["pad"]))
    d = None if ingest else dither_of(form, fmt, 0, nch, 0, Pmax)
    ref, _ = encode_units(y, out_fmt, d)
    want, out_stride, out_off = _want_clips(ref, K, BYTES[out_fmt], out_il, out_packed, out_len,
                                            encode_units(np.zeros(1), out_fmt)[0][0])
    a = tier.obj(nch, leg, chunk, form)
    xin = tier.buf(xb)
    whole, out = tier.guarded(want.size)
    p = a.resample_clips_sched_ptr(Kin if form["mix"] else 0, K, Mx, tier.ptr(xin), in_fmt, il, in_stride, in_off, in_len,
                                   tier.ptr(out), out_fmt, out_il, out_stride, out_off, out_len, flags)
    assert p == Pmax, what
    # (the symbols first: a launch sent to another form is named even where that form writes the same bytes)
    sym = a.boundary_symbols()
    if ingest:
        assert sym == (form["symbol"], "k_clip_rows_out<false, false>"), (what, sym)
    else:
        # (an ordered call hands its strided input over with bases: the packed row ingest)
        assert sym == ("k_clip_packed_rows_in" if sched else "k_clip_rows_in", expected_symbol(form, fmt)), (what, sym)
    tier.check_guarded(whole, want, 0, what)
    if form["meter"]:
        assert_meters(a.read_meters(reset=True), meters_of(y, F.rows_of(out_len, K), fmt, d), what)


def check_form(tier, form):
    """an id of the census: the form in all eight formats, alone and behind the chain, at every shape of its family"""
    for leg in ("pass", "chain"):
        for fmt in FORMATS:
            if form["family"] != "clip":
                check_plain(tier, form, fmt, leg)
            elif form["mix"]:
                for Kin, K in MIX_KS:
                    # (the planar layout of the mixing ingest is the (6, 1) case; behind the chain two of the four)
                    if leg == "pass" or Kin in (2, 64):
                        check_clip(tier, form, fmt, leg, K, Kin)
            else:
                for K in CLIP_KS[form["tiles"]]:
                    # (behind the chain: both pad rules, a non-power-of-two walk and the 64-frame tile)
                    if leg == "pass" or K in (1, 3, 7, 16, 33):
                        check_clip(tier, form, fmt, leg, K)


# ---------------------------------------------------------------- the lone event (PcmMeterCommit's wave reduction)
LANE_ROWS = 256
LANE_FORMATS = [S16, F32, U8]             # an integer, a float and a one-byte format
LANE_CHUNK = 4099                         # MaxInLen: every call below is one step, one window from frame 0


def event_value(r):
    """2.0 (peak, clipped), NaN (nonfinite: no peak) and 0.75 (a peak only) in a third of the rows each"""
    return (2.0, np.nan, 0.75)[r % 3]


def event_frame(form, fmt, r):
    """where row r's lone event lies so that lane r mod 64 of wave (r / 64) mod 4 converts it, by the maps of the module
    docstring; rows alternate between the first and the second workgroup of their row or clip.  k_pcm_finish's wave is
    the channel's (c mod 4): there the lane is (r + r / 64) mod 64, so that the 256 rows still meet every (lane, wave)"""
    lane, wave = r % 64, (r // 64) % 4
    if form["family"] == "finish" and form["tiles"]:
        return (r + r // 64) % 64 + 64 * (r % 2)
    if form["tiles"]:                     # K = 2: a tile of 1024 frames, thread = f mod 256
        return lane + 64 * wave + 256 * ((r // 2) % 4) + 1024 * ((r // 8) % 2)
    unit = 4 if BYTES[fmt] == 1 else 1    # (aligned one-byte rows: four frames per thread)
    return unit * (lane + 64 * wave) + (r % unit) + 2048 * (r % 2)


def _lane_call(tier, form, fmt, y, out_len, K):
    """the form's call on fp64 rows y [LANE_ROWS, n] (pass-through leg) -> (meters, the egress symbol)"""
    nch, n = y.shape
    a = tier.obj(nch, "pass", LANE_CHUNK, form)
    xin = tier.buf(np.ascontiguousarray(y))
    B = BYTES[fmt]
    if form["family"] == "finish":
        il = form["tiles"]
        stride = nch if il else n
        whole, out = tier.guarded(nch * n * B)
        assert a.process_pcm_ptr(tier.ptr(xin), F64, False, n, n, tier.ptr(out), fmt, il, stride) == n
    else:
        nclips, il = nch // K, form["tiles"]
        packed = form["addr"] == "packed" or (form["addr"] == "sched" and not form["pad"])
        off, pos = [0] * nclips, 0
        for i in reversed(range(nclips)):         # (regions end to end, last clip first: every base a multiple of four)
            off[i] = pos
            pos += out_len[i] * K
        stride = n * K if il else n
        whole, out = tier.guarded(nch * n * B)
        flags = (ORDER | DROP) if form["addr"] == "sched" else 0
        assert a.resample_clips_sched_ptr(0, K, None, tier.ptr(xin), F64, False, n, None, [n] * nclips, tier.ptr(out), fmt, il,
                                          0 if packed else stride, off if packed else None, out_len, flags) == max(out_len)
    got = tier.host(whole)
    assert np.all(got[:GUARD] == SENTINEL) and np.all(got[-GUARD:] == SENTINEL)
    return a.read_meters(reset=True), a.boundary_symbols()[1]


def check_meter_lanes(tier, form):
    """an id of the lone-event sweep: per format of LANE_FORMATS, 256 quiet rows (|v| <= 0.25) with one event each, placed
    by event_frame; then one row with a whole chunk or tile of 2.0 and one of NaN.  Asserted: the symbol, and peak bits,
    clipped and nonfinite of every channel exactly -- the lone event being the whole difference to a quiet row"""
    clip = form["family"] == "clip"
    K = 2 if (clip and form["tiles"]) else 1
    span = 64 if (form["family"] == "finish" and form["tiles"]) else 1024 if form["tiles"] else 2048
    n = 2 * span + (4 if clip else 0)
    out_len = [n - 4 * (i % 2) for i in range(LANE_ROWS // K)] if clip else [n] * LANE_ROWS
    lens = F.rows_of(out_len, K)
    for fmt in LANE_FORMATS:
        quiet = 0.5 * np.array(noise(LANE_ROWS, n, 900))
        assert np.abs(quiet).max() <= 0.25
        # 1. the lone events
        y = quiet.copy()
        at = [event_frame(form, fmt, r) for r in range(LANE_ROWS)]
        assert max(at) < min(lens)
        for r, f in enumerate(at):
            y[r, f] = event_value(r)
        d = dither_of(form, fmt, 0, LANE_ROWS, 0, n)
        got, sym = _lane_call(tier, form, fmt, y, out_len, K)
        what = (form["symbol"], FMT_NAME[fmt])
        assert sym == expected_symbol(form, fmt), (what, sym)
        want = meters_of(y, lens, fmt, d)
        base = meters_of(quiet, lens, fmt, d)
        for r in range(LANE_ROWS):
            v = event_value(r)
            assert base["clipped"][r] == 0 and base["nonfinite"][r] == 0
            assert want["clipped"][r] == (1 if v == 2.0 else 0) and want["nonfinite"][r] == (1 if v != v else 0)
            assert want["peak"][r] == (v if v == v else base["peak"][r])
        assert_meters(got, want, what + ("lone events",))
        # 2. the opposite load: every thread of a workgroup counts, in one channel
        y = quiet.copy()
        y[7, :span] = 2.0
        y[7, span:2 * span] = np.nan
        got, _ = _lane_call(tier, form, fmt, y, out_len, K)
        want = meters_of(y, lens, fmt, d)
        assert want["clipped"][7] == span and want["nonfinite"][7] == span and want["peak"][7] == 2.0
        assert_meters(got, want, what + ("full chunk",))


# ---------------------------------------------------------------- refusals
def check_refusals(tier):
    """What the launcher refuses (r8b_pcm_dispatch.h: clip_channels_check, the mixing ingest's check, "meters need all
    three arrays") is refused by the C ABI in FRONT of it, with r8b_capi.cpp's own words: a clip_channels outside 1 .. 64 or
    one that does not divide the channel count, an in_channels outside 1 .. 64, a mix without a matrix -- and the handle
    always passes all three meter arrays.  So no call reaches a launcher's refusal, none starts a kernel, and the output
    keeps its sentinels.  (The launcher's own messages: tests/cxx_pcm_boundary.cpp.)"""
    import ctypes as C
    nch, n = 12, 40
    a = tier.obj(nch, "pass", 64)
    a.enable_meters(True)
    xin = tier.buf(np.zeros((nch, n)))
    out = tier.sentinels(nch * n * 8)

    def call(K, kin=0, mix=None, il=True, istride=n):
        nclips = max(nch // max(K, 1), 1)
        ll = (C.c_longlong * nclips)(*([n // 2] * nclips))
        m = None if mix is None else (C.c_double * len(mix))(*mix)
        return a._lib.r8b_batch_resample_clips_sched(a._h, kin, K, m, C.c_void_p(tier.ptr(xin)), F64, int(il), istride, None, ll,
                                                     C.c_void_p(tier.ptr(out)), F64, int(il), n, None, ll, 0, C.c_void_p(0))

    def refused(word, *args, **kw):
        assert call(*args, **kw) == -1, (args, kw)
        err = a._lib.r8b_last_error()
        assert word in err, (args, kw, err)
        assert np.all(tier.host(out) == SENTINEL), (args, kw)
        assert a.stat("clip_steps") == 0

    for K in (0, -1, 65):
        refused(b"clip_channels must be 1 .. 64", K)
    for K in (5, 7, 8):
        refused(b"clip_channels does not divide the object's channel count", K)
    for kin in (-1, 65):
        refused(b"in_channels must be 1 .. 64", 2, kin=kin, mix=[0.5] * 130)
    refused(b"in_channels must be 0 or clip_channels when mix is NULL", 2, kin=3)
    refused(b"mix holds a coefficient that is not finite", 2, kin=3, mix=[0.5, float("nan")] + [0.0] * 4)
    # ... and the object is as good as new: the mixing tile ingest and the metering tile egress run
    assert call(2, kin=3, mix=[0.5, 0.25, 0.0, 0.0, 0.5, 0.25], istride=3 * n // 2) == n // 2, a._lib.r8b_last_error()
    assert a.boundary_symbols() == ("k_clip_mix_in", "k_clip_frames_out<false, true>")
    assert a.read_meters(reset=True)["nonfinite"].sum() == 0
