"""The census of the table-driven stage kernels: k_hbup, k_hbdown, k_hbcascade, k_hbdcascade, k_whole, k_poly and
k_poly_tiled.  Their "instances" are chosen at run time from tables (r8b_tables.inc, mirrored in oracle/data/tables.json,
which tests/test_abi_and_design.py pins to the reference's): 67 half-band filters of 1 ... 14 taps, cascades of up to
kMaxCascade = 8 stages whose widths (4 / 8 / 14) follow the tap counts, 22 interpolator banks of 6 ... 30 taps.  Shared by
the emulation tier (CPU) and the GPU tier (tests/test_stage_census.py) and, through --dump, by the sanitizer program
tests/cxx_stage_census.cpp.

  PART_A  every half-band row as a stand-alone up-sampler and decimator (check_hb_row), A_COLUMNS: the store forms
  PART_B  every cascade depth 2 ... 8, 8 + 1, 8 + 2 in both directions at four attenuations (check_up_chain,
          check_down_chain), B_COLUMNS: the store forms of the cascade's last stage
  PART_C  every bank length of both families on k_whole, k_poly_tiled (both fetch forms) and k_poly (check_bank)

The lists below are written out, not read from the tables: _complete() compares them with tables.json, so a row added to
the tables fails the census until it is listed.

Two oracles, neither derived from the code under test: the plain formulas in numpy.longdouble over the taps of
tables.json (hbup_formula, hbdown_formula; rounded to double at the end), and the compiled reference (oracle/refwrap.py)
where oracle/_ref was built.  Tolerances: cases.RMS_TOL / PEAK_TOL times the channel's own level times cases.tol_scale.

python tests/stage_census.py --dump   the chains of part B and one row of part A per tap count as lines
                                      what|kind|a|b|c|d|i0|i1|maxin|options|stage=symbol,...   ("stage": the descriptor of
                                      a stand-alone stage object; "chain": a = src, b = dst, c = transition band, d =
                                      attenuation; a stage without a symbol is a member of the run in front of it)"""
import json
import math
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_census import DeviceTier as _DeviceTier, HostTier as _HostTier, first_cut  # noqa: E402

LEVELS = (1.0, 1e-6, 0.0)      # full scale, 1e-6 of full scale, silence
NCH = len(LEVELS)
LOUD = tuple(c for c, lv in enumerate(LEVELS) if lv > 0.0)
TB = 2.0

_TABLES = None


def tables():
    global _TABLES
    if _TABLES is None:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle", "data", "tables.json")) as f:
            _TABLES = json.load(f)
    return _TABLES


def select_hb(att, steep, third):
    """the reference's selection rule (CDSPHBUpsampler.h / CDSPHBDownsampler.h): steepness clamped to 0 ... 6, the
    first row whose attenuation reaches `att`, else the last -> (steepness, row, taps, row attenuation)"""
    s = min(max(steep, 0), 6)
    rows = tables()["hb"]["third" if third else "half"][s]
    k = 0
    while k != len(rows) - 1 and rows[k]["att"] < att:
        k += 1
    return s, k, rows[k]["taps"], rows[k]["att"]


# ---- part A: every half-band row ----------------------------------------------------------------------------------------
# tap counts per steepness index, as r8b_tables.inc has them
HB_TAPS = {
    "half": ((4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14), (2, 3, 4, 5, 6, 7, 8), (2, 3, 4, 5, 6), (1, 2, 3, 4), (1, 2, 3, 4),
             (1, 2, 3), (1, 2, 3)),
    "third": ((3, 4, 5, 6, 7, 8, 9), (2, 3, 4, 5, 6), (1, 2, 3, 4, 5), (1, 2, 3, 4), (1, 2, 3), (1, 2, 3), (1, 2, 3)),
}
# The stated exception: the one-tap up-samplers, by (family, steepness).  The reference's ring reads one element past its
# mirrored prefix there (check_hb_row), at output index 1 of the stream and nowhere else
ONE_TAP_UP = (("half", 3), ("half", 4), ("half", 5), ("half", 6),
              ("third", 2), ("third", 3), ("third", 4), ("third", 5), ("third", 6))
ONE_TAP_INDEX = 1
A_MAXIN = 5000
COLUMN_TAPS = (1, 4, 5, 8, 9, 14)


def _part_a():
    es = []
    for fam in ("half", "third"):
        for steep, counts in enumerate(HB_TAPS[fam]):
            for row, nt in enumerate(counts):
                for kind in ("hbup", "hbdown"):
                    es.append(dict(part="A", kind=kind, fam=fam, third=int(fam == "third"), steep=steep, row=row, ntaps=nt,
                                   id="%s-%s-s%d-r%d-t%d" % (kind, fam, steep, row, nt)))
    return es


PART_A = _part_a()


def _first_with_taps(nt):
    return [e for e in PART_A if e["kind"] == "hbup" and e["ntaps"] == nt][0]


A_COLUMNS = [dict(_first_with_taps(nt), part="Acol", id="cols-" + _first_with_taps(nt)["id"]) for nt in COLUMN_TAPS]

# ---- part B: every cascade depth ----------------------------------------------------------------------------------------
ATTS = (60.0, 109.56, 180.15, 218.0)
THIRD_ATTS = (109.56, 218.0)
UP_K = tuple(range(3, 12))          # 44100 -> 44100 * 2^k: a 2x convolver and k - 1 half-band up-samplers
THIRD_K = (2, 5, 8)                 # 48000 -> 48000 * 3 * 2^k: a 3x convolver and k third-band up-samplers
KMAX = 8                            # kMaxCascade (r8b_launch.h)


LDS_MAX = 160 * 1024                # kLdsMaxBytes (r8b_launch.h): the LDS a workgroup may have
HBD_MIN_TILE = 32                   # last-stage outputs per workgroup of k_hbdcascade at the least


def runs_of(n):
    """how Engine::run_len cuts n consecutive half-band stages: runs of kMaxCascade and the rest"""
    return [KMAX] * (n // KMAX) + ([n % KMAX] if n % KMAX else [])


def _width(nt):
    return 4 if nt <= 4 else (8 if nt <= 8 else 14)


def hbd_lds_bytes(taps):
    """LDS of a decimating cascade over filters of `taps` taps (first stage first) at the smallest tile: every stage's
    input of a tile stays in LDS, in two buffers that alternate; a stage reads 2 n + 2 (2 T - 1) - 1 inputs for n outputs,
    T the tap count rounded up to 4 / 8 / 14, so the halos of the later stages double stage by stage towards the front"""
    span, buf = HBD_MIN_TILE, [0, 0]
    for g in range(len(taps) - 1, -1, -1):
        span = 2 * span + 2 * (2 * _width(taps[g]) - 1) - 1
        buf[g & 1] = max(buf[g & 1], span)
    return 8 * (buf[0] + 8 + buf[1] + 8)


def down_runs(taps):
    """... and consecutive decimators: a run ends behind kMaxCascade stages or where one stage more would ask for more LDS
    than a workgroup may have -- a launch the device refuses (found by this census: eight stages with the 14-wide filter
    of 180 dB at the end need 220 KB)"""
    runs, pos = [], 0
    while pos < len(taps):
        n = min(KMAX, len(taps) - pos)
        while n > 1 and hbd_lds_bytes(taps[pos:pos + n]) > LDS_MAX:
            n -= 1
        runs.append(n)
        pos += n
    return runs


def _up(src, mult, nhb, third, att, maxin, tile, tag):
    # (the up-samplers of a chain: steepness 0, 1, ... behind the convolver -- r8b_design.cpp build_topology)
    hb = [select_hb(att, s, third)[:2] + (len(select_hb(att, s, third)[2]),) for s in range(nhb)]
    return dict(part="Bup", src=src, dst=src * mult, maxin=maxin, att=att, third=int(third), nhb=nhb, hb=hb,
                runs=runs_of(nhb), opts=({"hbc_tile": tile} if tile else {}),
                one_tap=any(h[2] == 1 for h in hb), id="up-%s-a%g%s" % (tag, att, "-tile%d" % tile if tile else ""))


def _down(src_mult, dst, nhb, third, att, span, tag):
    # (the decimators of a chain: steepness nhb - 1, ..., 0 in front of the convolver)
    hb = [select_hb(att, nhb - 1 - i, third)[:2] + (len(select_hb(att, nhb - 1 - i, third)[2]),) for i in range(nhb)]
    opts = {"fuse_hbd": 1}
    if span:
        opts["hbd_span"] = span
    return dict(part="Bdown", src=dst * src_mult, dst=dst, ratio=src_mult, maxin=50 * src_mult, att=att, third=int(third),
                nhb=nhb, hb=hb, runs=down_runs([h[2] for h in hb]), opts=opts,
                id="down-%s-a%g%s" % (tag, att, "-span%d" % span if span else ""))


def _part_b():
    ups, downs = [], []
    for k in UP_K:
        for att in ATTS:
            for tile in (0, 256):
                ups.append(_up(44100.0, 2 ** k, k - 1, False, att, 40 + 3 * (k - 3), tile, "k%d" % k))
            for span in (0, 512):
                downs.append(_down(2 ** k, 44100.0, k - 1, False, att, span, "k%d" % k))
    for k in THIRD_K:
        for att in THIRD_ATTS:
            for tile in (0, 256):
                ups.append(_up(48000.0, 3 * 2 ** k, k, True, att, 40 + 3 * k, tile, "3k%d" % k))
            for span in (0, 512):
                # (48000 * 3 * 2^k -> 48000: k third-band decimators and a convolver that decimates by 3)
                downs.append(_down(3 * 2 ** k, 48000.0, k, True, att, span, "3k%d" % k))
    return ups, downs


PART_B_UP, PART_B_DOWN = _part_b()
B_COLUMNS = [dict(e, part="Bcol", id="cols-" + e["id"]) for e in PART_B_UP
             if e["id"] in ("up-k4-a180.15", "up-k9-a180.15")]

# ---- part C: every interpolator bank ------------------------------------------------------------------------------------
BANK_TAPS = {0: (8, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28, 30), 1: (6, 8, 10, 12, 14, 16, 18, 20, 22, 24)}
C_MAXIN = 600
# (src, dst, whole stepping, option poly_tiled or None, the symbol that runs, whether the tiled kernel fetches samples and
# bank entries together -- L.front, spans up to 200 samples: 64 * src / dst + taps + 4)
RATIOS = (
    (88200.0, 96000.0, 1, None, "k_whole", None),
    (96000.0, 44100.0, 1, None, "k_whole", None),
    (44100.0, 44101.0, 0, 1, "k_poly_tiled", True),
    (44100.0, 44101.0, 0, 0, "k_poly", None),
    (96000.0, 44101.0, 0, 1, "k_poly_tiled", True),
    (96000.0, 44101.0, 0, 0, "k_poly", None),
    (192000.0, 44101.0, 0, 1, "k_poly_tiled", False),
    (192000.0, 44101.0, 0, 0, "k_poly", None),
)


def bank_att(third, taps):
    """the attenuation that selects the bank of `taps` taps (CDSPFracInterpolator.h: the first row whose attenuation
    reaches the request): the row's own, less 0.01"""
    fr = tables()["frac"]
    rows, base = fr["Coeffs3" if third else "Coeffs2"], fr["Coeffs3Base" if third else "Coeffs2Base"]
    i = (taps - base) // 2
    assert base + 2 * i == taps and 0 <= i < len(rows)
    return rows[i][2] - 0.01


def _part_c():
    es = []
    for third in (0, 1):
        for taps in BANK_TAPS[third]:
            for src, dst, whole, tiled, symbol, front in RATIOS:
                es.append(dict(part="C", third=third, taps=taps, src=src, dst=dst, whole=whole, symbol=symbol, front=front,
                               opts=({} if tiled is None else {"poly_tiled": tiled}),
                               id="bank%d-t%d-%g-%g%s" % (3 if third else 2, taps, src, dst,
                                                          "" if tiled is None else "-tiled%d" % tiled)))
    return es


PART_C = _part_c()


def _complete():
    """the lists above against tables.json, both ways"""
    t = tables()
    for fam in ("half", "third"):
        got = tuple(tuple(len(r["taps"]) for r in rows) for rows in t["hb"][fam])
        assert got == HB_TAPS[fam], "tables.json hb/%s has rows the census does not list (or the reverse): %s" % (fam, got)
    assert sum(len(c) for c in HB_TAPS["half"]) == 37 and sum(len(c) for c in HB_TAPS["third"]) == 30
    assert len(PART_A) == 134 and len({e["id"] for e in PART_A}) == 134
    one = {(fam, s) for fam in HB_TAPS for s, counts in enumerate(HB_TAPS[fam]) for nt in counts if nt == 1}
    n_one = sum(nt == 1 for fam in HB_TAPS for counts in HB_TAPS[fam] for nt in counts)
    assert set(ONE_TAP_UP) == one and len(ONE_TAP_UP) == n_one == 9, "the exception is the nine one-tap rows, no other"
    assert {e["ntaps"] for e in PART_A} == set(range(1, 15)) and [e["ntaps"] for e in A_COLUMNS] == list(COLUMN_TAPS)
    fr = t["frac"]
    for third, key in ((0, "Coeffs2"), (1, "Coeffs3")):
        got = tuple(fr[key + "Base"] + 2 * i for i in range(len(fr[key])))
        assert got == BANK_TAPS[third], "tables.json frac/%s has banks the census does not list: %s" % (key, got)
        assert {e["taps"] for e in PART_C if e["third"] == third} == set(got)
    assert sorted(set(BANK_TAPS[0]) | set(BANK_TAPS[1])) == list(range(6, 31, 2))      # 13 lengths
    # every depth, both directions, every attenuation; the cut behind 8
    want = [[2], [3], [4], [5], [6], [7], [8], [8, 1], [8, 2]]
    for part in (PART_B_UP, PART_B_DOWN):
        for att in ATTS:
            for variant in (False, True):
                got = [e["runs"] for e in part if e["att"] == att and not e["third"] and bool(
                    e["opts"].get("hbc_tile") or e["opts"].get("hbd_span")) == variant]
                # (decimating runs whose last filters are 14 wide end before the eighth stage: down_runs)
                assert got == want or (part is PART_B_DOWN and att > 110.0 and got[:5] == want[:5] and
                                       [sum(r) for r in got] == [sum(r) for r in want]), (att, variant, got)
        assert all(sum(e["runs"]) == e["nhb"] and max(e["runs"]) <= KMAX for e in part)
        assert len({e["id"] for e in part}) == len(part) == 2 * (len(UP_K) * len(ATTS) + len(THIRD_K) * len(THIRD_ATTS))
    assert any(e["runs"] != runs_of(e["nhb"]) for e in PART_B_DOWN) and hbd_lds_bytes([2, 3, 3, 3, 4, 5, 6, 11]) > LDS_MAX
    # between them the attenuations put each width 4 / 8 / 14 at the first, an inner and the last position of an
    # up-sampling run, and one-tap filters at the tail
    width = _width
    seen = set()
    for e in PART_B_UP:
        pos = 0
        for r in e["runs"]:
            for i in range(r):
                seen.add((width(e["hb"][pos + i][2]), "first" if i == 0 else ("last" if i == r - 1 else "inner")))
            pos += r
    assert seen >= {(w, p) for w in (4, 8) for p in ("first", "inner", "last")} | {(14, "first")}, sorted(seen)
    assert any(e["one_tap"] and e["hb"][-1][2] == 1 for e in PART_B_UP) and any(not e["one_tap"] for e in PART_B_UP)
    assert any(h[0] == 6 for e in PART_B_UP for h in e["hb"]) and any(e["nhb"] > 7 for e in PART_B_UP)   # index 6, its clamp
    assert len(B_COLUMNS) == 2


_complete()


# ---- the oracles --------------------------------------------------------------------------------------------------------
def _shifted(x, first, count):
    """x[first : first + count] with zeros outside the array"""
    import numpy as np
    out = np.zeros(count, dtype=x.dtype)
    lo, hi = max(first, 0), min(first + count, len(x))
    if hi > lo:
        out[lo - first:hi - first] = x[lo:hi]
    return out


def hbup_formula(x, taps):
    """y[2n] = x[n], y[2n+1] = sum_k f[k] (x[n+1+k] + x[n-k]) in longdouble, samples before the stream zero; the
    2 (len(x) - T) outputs the stage has emitted after len(x) inputs (CDSPHBUpsampler: an output waits for its last
    input).  x and the result are longdouble"""
    import numpy as np
    T, n = len(taps), max(0, len(x) - len(taps))
    y = np.zeros(2 * n, dtype=np.longdouble)
    y[0::2] = x[:n]
    acc = np.zeros(n, dtype=np.longdouble)
    for k in range(T):
        acc += np.longdouble(taps[k]) * (_shifted(x, 1 + k, n) + _shifted(x, -k, n))
    y[1::2] = acc
    return y


def hbup_total(m, T):
    return 2 * max(0, m - T)


def hbdown_formula(x, taps):
    """y[n] = x[2n] + sum_k f[k] (x[2n+1+2k] + x[2n-1-2k]) in longdouble; the len(x) // 2 - T + 1 outputs the stage has
    emitted after len(x) inputs"""
    import numpy as np
    T = len(taps)
    n = hbdown_total(len(x), T)
    xp = np.concatenate([np.zeros(2 * T, dtype=np.longdouble), x])      # (x[i] at xp[i + 2T])
    y = xp[2 * T:2 * T + 2 * n:2].copy()
    for k in range(T):
        a = 2 * T + 1 + 2 * k
        b = 2 * T - 1 - 2 * k
        y += np.longdouble(taps[k]) * (xp[a:a + 2 * n:2] + xp[b:b + 2 * n:2])
    return y


def hbdown_total(m, T):
    return max(0, m // 2 - T + 1)


def _counts(total, lens, T):
    out, m = [], 0
    for l in lens:
        out.append(total(m + l, T) - total(m, T))
        m += l
    return out


_INPUT = {}


def stage_input(n):
    """NCH rows of splitmix noise at LEVELS, computed once per length and left unchanged (the longest streams of the
    decimating chains are not kept)"""
    import numpy as np
    import r8b_oracle as O
    if n not in _INPUT:
        x = np.stack([lv * O.splitmix_uniform(411 + c, n) for c, lv in enumerate(LEVELS)])
        x.setflags(write=False)
        if n > 200000:
            return x
        _INPUT[n] = x
    return _INPUT[n]


class Worst:
    """the worst own-level (rms, peak) over tol_scale per oracle, as test_kernel_census.py prints them"""

    def __init__(self):
        self.by = {}

    def note(self, oracle, r, p):
        a = self.by.get(oracle, (0.0, 0.0))
        self.by[oracle] = (max(a[0], r), max(a[1], p))

    def __str__(self):
        return ", ".join("%s rms %.3g peak %.3g" % ((k,) + v) for k, v in sorted(self.by.items())) or "-"


def judge(worst, oracle, y, yo, what, skip=None, peak_only=False):
    """every loud channel of y against yo within RMS_TOL / PEAK_TOL times its own level times tol_scale of its stream;
    `skip`: output indices left out (the stated exception alone)"""
    import numpy as np
    from cases import PEAK_TOL, RMS_TOL, tol_scale
    assert y.shape == yo.shape, (what, oracle, y.shape, yo.shape)
    for c in LOUD:
        d = (y[c] - yo[c]) / LEVELS[c]
        if skip is not None:
            d = np.delete(d, skip)
        sc = tol_scale(float(np.sum((y[c] / LEVELS[c]) ** 2)), y.shape[1])
        rr = math.sqrt(float(np.mean(d * d))) if d.size else 0.0
        pp = float(np.abs(d).max()) if d.size else 0.0
        worst.note(oracle, rr / sc, pp / sc)
        assert (peak_only or rr <= RMS_TOL * sc) and pp <= PEAK_TOL * sc, \
            "%s against %s, channel %d (level %g): rms %.3g peak %.3g of its level, scale %.2f, first at output %d" % (
                what, oracle, c, LEVELS[c], rr, pp, sc, int(np.argmax(np.abs(d) > PEAK_TOL * sc)))


def stream(tier, b, xd, lens):
    """-> (outputs, per-call counts, the symbols every stage ran: '' for a stage that launched nothing of its own)"""
    ys, pos, seen = [], 0, [set() for _ in b.stage_symbols()]
    for l in lens:
        ys.append(tier.call(b, xd[:, pos:pos + l]))
        for s, sym in zip(seen, b.stage_symbols()):
            s.add(sym)
        pos += l
    assert pos == xd.shape[1]
    return tier.cat(ys), [int(y.shape[1]) for y in ys], [s - {""} for s in seen]


def second_cut(n, maxin, lens, at):
    """another cut of the stream into calls (nonfinite_cases._lens: a call ends at `at`, a one-sample call behind it)"""
    from nonfinite_cases import _lens
    lens2, i = _lens(n, maxin, at)
    assert i is not None and i + 1 < len(lens2)
    if lens2[i + 1] > 1:
        lens2[i + 1:i + 2] = [1, lens2[i + 1] - 1]
    assert sum(lens2) == n and 1 in lens2 and lens2 != lens and max(lens2) <= maxin
    return lens2


def assert_same_bits(tier, yd, y2d, what):
    import numpy as np
    if not tier.same_bits(yd, y2d):
        y, y2 = tier.host(yd), tier.host(y2d)
        c, j = np.nonzero(y != y2) if y.shape == y2.shape else ([-1], [-1])
        raise AssertionError("%s: the output depends on the cut into calls, first (channel, output): (%d, %d) of %d" % (
            what, c[0], j[0], len(c)))


def _finish(y, what):
    import numpy as np
    assert y.shape[0] == NCH and y.shape[1] > 0 and np.isfinite(y).all(), (what, y.shape)
    assert not y[2].any(), "%s: silence in, %g out" % (what, float(np.abs(y[2]).max()))
    assert float(np.abs(y[0]).max()) > 0.01, (what, "no signal")


def _hb_lines(desc):
    return [tuple(int(v) for v in m[:3]) + (float(m[3]),) for m in
            re.findall(r"HB(?:Up|Down)sampler: sti=(\d+) third=(\d) taps=(\d+) att=([\d.]+)", desc)]


def _ref_stage_stream(refwrap, kind, args, x, lens):
    """one reference stage object per loud channel through the calls -> (rows, per-call counts)"""
    import numpy as np
    rows, counts = [], None
    for c in range(NCH):
        if c not in LOUD:
            rows.append(None)
            continue
        rs = refwrap.RefStage(kind, *args)
        ys, pos = [], 0
        for l in lens:
            ys.append(rs.process(x[c, pos:pos + l]))
            pos += l
        cn = [len(v) for v in ys]
        assert counts is None or cn == counts
        counts = cn
        rows.append(np.concatenate(ys))
    n = len(rows[LOUD[0]])
    return np.stack([r if r is not None else np.zeros(n) for r in rows]), counts


# ---- part A -------------------------------------------------------------------------------------------------------------
def hb_descriptor(e):
    row = tables()["hb"][e["fam"]][e["steep"]][e["row"]]
    return (2 if e["kind"] == "hbup" else 3, row["att"] - 0.01, 0.0, 0.0, 0.0, e["steep"], e["third"])


def a_lens():
    lens = [A_MAXIN, A_MAXIN] + first_cut(7000, A_MAXIN)
    assert 1 in lens and any(l % 1024 not in (0, 1) for l in lens)
    return lens


def check_hb_row(make, tier, e, refwrap=None):
    """One row of the half-band tables as a stand-alone stage object (`make(descriptor)`: NCH channels, MaxInLen 5000,
    timing on), two whole calls and the ragged pattern of first_cut behind them.
      1. describe() names the row's tap count and attenuation, every launch was k_hbup / k_hbdown;
      2. per-call counts are the closed form's, every output of every loud channel is the plain formula's (longdouble,
         over the taps of tables.json) within the tolerance at the channel's own level; the silent channel is exact zeros;
      3. where the compiled reference is present: counts and every output against RefStage -- except, for the nine
         one-tap up-samplers (ONE_TAP_UP), output index 1 of the stream, which is left out and nothing else.  Cause, read
         in the reference's CDSPHBUpsampler.h: with fltt = 1 tap fll = 0, so flb = BufLen, clear() sets ReadPos = BufLen
         unmasked and its memset clears nothing; the first convolve1 call then reads rp[1] at Buf[BufLen + 1], one element
         past the flo = 1 elements the ring mirrors, which is never written.  The observed value behaves as if x[1] were 0.
         The project follows the stated formula y[2n+1] = f[0] (x[n+1] + x[n]).  With index 1 left out the reference must
         agree with the plain formula on these rows too: asserted;
      4. another cut into calls gives the same bits.
    Returns the Worst figures."""
    import numpy as np
    row = tables()["hb"][e["fam"]][e["steep"]][e["row"]]
    taps, up = row["taps"], e["kind"] == "hbup"
    assert len(taps) == e["ntaps"]
    desc = hb_descriptor(e)
    b = make(desc)
    got = _hb_lines(b.describe())
    assert len(got) == 1 and got[0][:3] == (e["steep"], e["third"], e["ntaps"]) and abs(got[0][3] - row["att"]) <= 0.0051, \
        (e["id"], b.describe())
    lens = a_lens()
    n = sum(lens)
    x = stage_input(n)
    xd = tier.put(x)
    yd, counts, seen = stream(tier, b, xd, lens)
    symbol = "k_hbup" if up else "k_hbdown"
    assert seen == [{symbol}], (e["id"], seen)
    y = tier.host(yd)
    _finish(y, e["id"])
    worst = Worst()
    # 2.
    assert counts == _counts(hbup_total if up else hbdown_total, lens, len(taps)), (e["id"], counts)
    formula = hbup_formula if up else hbdown_formula
    yo = np.stack([formula(x[c].astype(np.longdouble), taps).astype(np.float64) for c in range(NCH)])
    judge(worst, "formula", y, yo, e["id"])
    # 3.
    excepted = up and e["row"] == 0 and (e["fam"], e["steep"]) in ONE_TAP_UP     # (the one-tap row opens its group)
    assert excepted == (up and e["ntaps"] == 1)
    if refwrap is not None:
        yr, rcounts = _ref_stage_stream(refwrap, e["kind"], desc[1:], x, lens)
        assert counts == rcounts, (e["id"], counts, rcounts)
        skip = [ONE_TAP_INDEX] if excepted else None
        judge(worst, "RefStage", y, yr, e["id"], skip=skip)
        judge(Worst(), "RefStage", yo, yr, e["id"] + " (the plain formula)", skip=skip)
    # 4.
    y2d, _, seen2 = stream(tier, make(desc), xd, second_cut(n, A_MAXIN, lens, 3 * 1024 + 517))
    assert seen2 == [{symbol}]
    assert_same_bits(tier, yd, y2d, e["id"])
    return worst


def check_columns(make, tier, lens, x, what, cols=(4, 5)):
    """Every call's outputs at an even and at an odd element offset of rows filled with NaN (test_emul.
    run_output_columns_case): the placements equal each other and a column-0 caller bit for bit, and not an element
    outside the call's n outputs is touched -- guard columns on both sides"""
    import numpy as np
    from nonfinite_cases import _bits
    ref, objs = make(), [make() for _ in cols]
    cap = ref.max_out_len
    pitch = (cap + 17) & ~1
    pos, total = 0, 0
    for l in lens:
        xa = np.ascontiguousarray(x[:, pos:pos + l])
        pos += l
        yref = ref.process_host(xa)
        for col, o in zip(cols, objs):
            ip, istride, obuf, op, back = tier.buffers(xa, NCH, pitch)
            assert op % 16 == 0
            n = o.process_ptr(ip, istride, l, op + 8 * col, pitch)
            got = back(obuf)
            assert n == yref.shape[1], (what, l, col)
            assert np.array_equal(_bits(got[:, col:col + n]), _bits(yref)), (what, l, col)
            assert np.isnan(got[:, :col]).all() and np.isnan(got[:, col + n:]).all(), (what, l, col)
        total += yref.shape[1]
    assert total > 0, what
    return ref


def check_hb_columns(make, tier, e):
    """the store forms of hbup_compute: a destination row at an even element offset (pair16: the even / odd output pair
    as one 16-byte store), at an odd one (pair16b: odd output with the next even one), the scalar stores at range ends"""
    desc = hb_descriptor(e)
    lens = [A_MAXIN, 1, 1666, 2, 301, A_MAXIN - 5]
    ref = check_columns(lambda: make(desc), tier, lens, stage_input(sum(lens)), e["id"])
    assert ref.stage_symbols() == ["k_hbup"]


# ---- part B -------------------------------------------------------------------------------------------------------------
def _expected_symbols(e, first, fused, kernel, single):
    """per stage: the symbol its launches carry, None for a member of a run (no launch of its own) -- the run lengths
    and the cut behind kMaxCascade.  first: index of the first half-band stage"""
    out = {}
    pos = first
    for r in (e["runs"] if fused else [1] * e["nhb"]):
        out[pos] = kernel if r > 1 else single
        for i in range(1, r):
            out[pos + i] = None
        pos += r
    return out


def _assert_runs(b, seen, e, first, fused, kernel, single):
    want = _expected_symbols(e, first, fused, kernel, single)
    timings = b.stage_timings()
    for s, sym in want.items():
        assert seen[s] == ({sym} if sym else set()), (e["id"], s, seen)
        assert (timings[s][2] > 0) == (sym is not None), (e["id"], s, timings[s])
    return want


def _assert_plan(b, e):
    """describe() lists the half-band stages the tables give for the chain"""
    got = _hb_lines(b.describe())
    assert [g[2] for g in got] == [h[2] for h in e["hb"]], (e["id"], got, e["hb"])
    # (the engine prints the requested steepness index; the tables' row is selected with the index clamped to 6)
    want_sti = list(range(e["nhb"])) if e["part"] != "Bdown" else list(range(e["nhb"] - 1, -1, -1))
    assert [g[0] for g in got] == want_sti and all(g[1] == e["third"] for g in got), (e["id"], got)
    assert all(abs(g[3] - tables()["hb"]["third" if e["third"] else "half"][h[0]][h[1]]["att"]) <= 0.0051
               for g, h in zip(got, e["hb"])), (e["id"], got)


_COMPOSED = {}


def composed_up_oracle(e, x, lens, refwrap):
    """the chain's convolver as the compiled reference's stage object (RefStage("conv"), its descriptor from
    refwrap.topology; the numpy oracle's convolver where oracle/_ref is absent), behind it the plain-formula up-samplers
    in longdouble, stage by stage; the formula has no delay, so the streams align at index 0.  Shared by the entries of a
    chain (tile variants, both tiers)"""
    import numpy as np
    key = (e["src"], e["dst"], e["att"], e["maxin"], refwrap is not None)
    if key not in _COMPOSED:
        up = 3 if e["third"] else 2
        if refwrap is not None:
            top = refwrap.topology(e["src"], e["dst"], e["maxin"], TB, e["att"])
            # (the filter's own line is printed only where the reference designs it anew: the header and the convolver's)
            m = re.search(r"CDSPResampler: src=([\d.]+) dst=([\d.]+) len=\d+ tb=([\d.]+) att=([\d.]+) ph=0", top)
            io = re.search(r"CDSPBlockConvolver: .*io=(\d+)/(\d+)", top)
            assert m and io and (int(io.group(1)), int(io.group(2))) == (up, 1), top
            assert (float(m.group(1)), float(m.group(2)), float(m.group(3))) == (e["src"], e["dst"], TB) and \
                abs(float(m.group(4)) - e["att"]) < 0.006, top
            f = re.search(r"CDSPFIRFilter: .* nfreq=([\d.]+) tb=([\d.]+) att=[\d.]+ gain=([\d.]+)", top)
            assert f is None or (abs(float(f.group(1)) - 1.0 / up) < 1e-4 and float(f.group(2)) == TB and
                                 float(f.group(3)) == up), top
            assert top.count("CDSPHBUpsampler") == e["nhb"], top
            conv, _ = _ref_stage_stream(refwrap, "conv", (1.0 / up, TB, e["att"], float(up), up, 1), x, lens)
        else:
            import r8b_oracle as O
            rows = []
            for c in range(NCH):
                st = O.ConvStage(1.0 / up, TB, e["att"], float(up), up, 1)
                pos, ys = 0, []
                for l in lens:
                    ys.append(st.process(x[c, pos:pos + l]))
                    pos += l
                rows.append(np.concatenate(ys))
            conv = np.stack(rows)
        rows = []
        for c in range(NCH):
            v = conv[c].astype(np.longdouble)
            for s, r, nt in e["hb"]:
                taps = tables()["hb"]["third" if e["third"] else "half"][s][r]["taps"]
                assert len(taps) == nt
                v = hbup_formula(v, taps)
            rows.append(v.astype(np.float64))
        if len(_COMPOSED) >= 3:
            _COMPOSED.pop(next(iter(_COMPOSED)))
        _COMPOSED[key] = np.stack(rows)
    return _COMPOSED[key]


def up_lens(b, e):
    n = b.getInLenBeforeOutPos(0) + 3 * e["maxin"] + 7
    return n, first_cut(n, e["maxin"])


def check_up_chain(make, tier, e, refwrap=None):
    """An up-sampling chain: a 2x (3x) convolver and e["nhb"] half-band up-samplers, `make(options)` -> NCH channels,
    timing on.  Enough ragged calls for three whole calls of output behind the latency.
      0. describe() lists the filters the tables give; the stages report k_hbcascade in runs of e["runs"] -- the cut
         behind kMaxCascade = 8 -- and a run of one k_hbup;
      1. per-call counts equal RefResampler's;
      2. every output against the composed oracle (composed_up_oracle);
      3. every output against the compiled reference chain, unless the chain holds a one-tap up-sampler (e["one_tap"],
         computed from the tables: the stated exception of check_hb_row at the head of that stage's stream);
      4. the unfused twin (option fuse_hb = 0: k_hbup stage by stage, which sums in another order) to PEAK_TOL;
      5. another cut into calls gives the same bits."""
    import numpy as np
    b = make(e["opts"])
    _assert_plan(b, e)
    n, lens = up_lens(b, e)
    x = stage_input(n)
    xd = tier.put(x)
    yd, counts, seen = stream(tier, b, xd, lens)
    _assert_runs(b, seen, e, 1, True, "k_hbcascade", "k_hbup")
    y = tier.host(yd)
    _finish(y, e["id"])
    worst = Worst()
    # 2.
    yo = composed_up_oracle(e, x, lens, refwrap)
    assert yo.shape[1] == sum(counts), (e["id"], yo.shape, sum(counts))
    judge(worst, "composed", y, yo, e["id"])
    # 1., 3.
    if refwrap is not None:
        r, p = refwrap.batch_check(e["src"], e["dst"], e["maxin"], lens, x, y, counts, TB, e["att"])
        if not e["one_tap"]:
            from cases import PEAK_TOL, RMS_TOL, tol_scale
            for c in LOUD:
                sc = tol_scale(float(np.sum((y[c] / LEVELS[c]) ** 2)), y.shape[1])
                rr, pp = r[c] / LEVELS[c], p[c] / LEVELS[c]
                worst.note("reference chain", rr / sc, pp / sc)
                assert rr <= RMS_TOL * sc and pp <= PEAK_TOL * sc, "%s against the reference chain, channel %d: rms %.3g " \
                    "peak %.3g of its level, scale %.2f" % (e["id"], c, rr, pp, sc)
    # 4.
    t = make(dict(e["opts"], fuse_hb=0))
    ytd, tcounts, tseen = stream(tier, t, xd, lens)
    _assert_runs(t, tseen, e, 1, False, "k_hbcascade", "k_hbup")
    assert tcounts == counts
    judge(worst, "unfused twin", y, tier.host(ytd), e["id"], peak_only=True)
    # 5.
    y2d, _, _ = stream(tier, make(e["opts"]), xd, second_cut(n, e["maxin"], lens, n - 2 * e["maxin"] + 11))
    assert_same_bits(tier, yd, y2d, e["id"])
    return worst


def check_chain_columns(make, tier, e):
    """the last stage of k_hbcascade stores output pairs (HBCascadeLaunch::pair_ok) when the caller's rows are 16-byte
    aligned; at an odd element offset they are not, and it stores single outputs: both placements bit for bit"""
    b = make(e["opts"])
    n = b.getInLenBeforeOutPos(0) + 2 * e["maxin"] + 3
    lens = first_cut(n, e["maxin"])
    ref = check_columns(lambda: make(e["opts"]), tier, lens, stage_input(n), e["id"])
    assert ref.stage_symbols()[1] == "k_hbcascade"


def down_lens(b, e):
    n = b.getInLenBeforeOutPos(0) + 300 * e["ratio"] + 13
    return n, first_cut(n, e["maxin"])


def check_down_chain(make, tier, e, refwrap=None):
    """A decimating chain: e["nhb"] half-band decimators in front of the convolver, option fuse_hbd = 1 (and hbd_span = 512), about 300 outputs beyond the latency in ragged calls.
      0. describe() lists the filters the tables give; the stages report k_hbdcascade in runs of e["runs"] (down_runs: the
         cut behind eight stages, or earlier where the run would not fit the LDS), k_hbdown for a run of one;
      1. counts and samples against the compiled reference chain (where present);
      2. the unfused twin (fuse_hbd = 0) to PEAK_TOL;
      3. another cut into calls gives the same bits."""
    import numpy as np
    b = make(e["opts"])
    _assert_plan(b, e)
    n, lens = down_lens(b, e)
    x = stage_input(n)
    xd = tier.put(x)
    yd, counts, seen = stream(tier, b, xd, lens)
    _assert_runs(b, seen, e, 0, True, "k_hbdcascade", "k_hbdown")
    y = tier.host(yd)
    _finish(y, e["id"])
    assert 290 <= y.shape[1] <= 320, (e["id"], y.shape)
    worst = Worst()
    if refwrap is not None:
        from cases import PEAK_TOL, RMS_TOL, tol_scale
        r, p = refwrap.batch_check(e["src"], e["dst"], e["maxin"], lens, x, y, counts, TB, e["att"])
        for c in LOUD:
            sc = tol_scale(float(np.sum((y[c] / LEVELS[c]) ** 2)), y.shape[1])
            rr, pp = r[c] / LEVELS[c], p[c] / LEVELS[c]
            worst.note("reference chain", rr / sc, pp / sc)
            assert rr <= RMS_TOL * sc and pp <= PEAK_TOL * sc, "%s against the reference chain, channel %d: rms %.3g " \
                "peak %.3g of its level, scale %.2f" % (e["id"], c, rr, pp, sc)
    t = make(dict(e["opts"], fuse_hbd=0))
    ytd, tcounts, tseen = stream(tier, t, xd, lens)
    _assert_runs(t, tseen, e, 0, False, "k_hbdcascade", "k_hbdown")
    assert tcounts == counts
    judge(worst, "unfused twin", y, tier.host(ytd), e["id"], peak_only=True)
    del ytd
    y2d, _, _ = stream(tier, make(e["opts"]), xd, second_cut(n, e["maxin"], lens, n - 2 * e["maxin"] + 11))
    assert_same_bits(tier, yd, y2d, e["id"])
    return worst


# ---- part C -------------------------------------------------------------------------------------------------------------
def bank_descriptor(e):
    return (1, e["src"], e["dst"], bank_att(e["third"], e["taps"]), 0.0, e["third"], 0)


_BANK_REF = {}


def _bank_reference(e, desc, x, lens, refwrap):
    """RefStage("frac") through the calls, one object per loud channel (the numpy oracle's stage where oracle/_ref is
    absent), computed once per (bank, ratio, cut) and shared by the tiers and the poly_tiled variants"""
    import numpy as np
    key = (desc, tuple(lens), refwrap is not None)
    if key not in _BANK_REF:
        if refwrap is not None:
            _BANK_REF[key] = _ref_stage_stream(refwrap, "frac", desc[1:], x, lens)
        else:
            import r8b_oracle as O
            rows = []
            for c in range(NCH):
                st = O.make_stage(("frac", e["src"], e["dst"], desc[3], bool(e["third"])))
                ys, pos = [], 0
                for l in lens:
                    ys.append(st.process(x[c, pos:pos + l]))
                    pos += l
                rows.append(np.concatenate(ys))
                rcounts = [len(v) for v in ys]
            _BANK_REF[key] = (np.stack(rows), rcounts)
    return _BANK_REF[key]


def check_bank(make, tier, e, refwrap=None):
    """One interpolator bank as a stand-alone stage object (`make(descriptor, options)`: NCH channels, MaxInLen 600 --
    several tiles of 64 outputs and a partial one per call).
      1. describe() names the bank's length and the stepping; the launches carry e["symbol"]; counter poly_front tells the
         tiled kernel's two fetch forms apart (L.front: a tile's span within 200 samples);
      2. counts and samples against RefStage("frac") (the numpy oracle's stage where oracle/_ref is absent);
      3. another cut into calls gives the same bits on k_whole.  The polynomial path restarts its position counter at the
         first call that begins more than 1000 outputs after the last restart (reference CDSPFracInterpolator.h:909-917,
         at the head of process()), so its rounding depends on where calls begin, in the reference as here: there the
         other cut is held to RefStage run through the same calls (counts and samples), and a third cut that differs
         from the first only inside the first call -- before any restart is due -- gives the same bits."""
    import numpy as np
    desc = bank_descriptor(e)
    b = make(desc, e["opts"])
    m = re.search(r"FracInterpolator: .* whole=(\d) step=\S+ taps=(\d+)", b.describe())
    assert m and (int(m.group(1)), int(m.group(2))) == (e["whole"], e["taps"]), (e["id"], b.describe())
    lens = [C_MAXIN, C_MAXIN] + first_cut(1500, C_MAXIN)
    n = sum(lens)
    x = stage_input(n)
    xd = tier.put(x)
    yd, counts, seen = stream(tier, b, xd, lens)
    assert seen == [{e["symbol"]}], (e["id"], seen)
    if e["symbol"] == "k_poly_tiled":
        assert (b.stat("poly_front") > 0) == e["front"], (e["id"], b.stat("poly_front"))
    else:
        assert b.stat("poly_front") == 0 or e["opts"].get("poly_tiled") is None
    y = tier.host(yd)
    _finish(y, e["id"])
    yr, rcounts = _bank_reference(e, desc, x, lens, refwrap)
    assert counts == rcounts, (e["id"], counts, rcounts)
    worst = Worst()
    oracle = "RefStage" if refwrap is not None else "numpy oracle"
    judge(worst, oracle, y, yr, e["id"])
    lens2 = second_cut(n, C_MAXIN, lens, 2 * C_MAXIN + 333)
    y2d, counts2, seen2 = stream(tier, make(desc, e["opts"]), xd, lens2)
    assert seen2 == [{e["symbol"]}]
    if e["whole"]:
        assert_same_bits(tier, yd, y2d, e["id"])
    else:
        # 3. on the polynomial path
        yr2, rcounts2 = _bank_reference(e, desc, x, lens2, refwrap)
        assert counts2 == rcounts2, (e["id"], counts2, rcounts2)
        judge(worst, oracle + ", second cut", tier.host(y2d), yr2, e["id"])
        lens3 = [C_MAXIN // 2 + 3, 1, C_MAXIN - C_MAXIN // 2 - 4] + lens[1:]
        assert sum(counts[:1]) <= 1000 and sum(lens3) == n
        y3d, _, _ = stream(tier, make(desc, e["opts"]), xd, lens3)
        assert_same_bits(tier, yd, y3d, e["id"])
    return worst


class HostTier(_HostTier):
    def buffers(self, xa, rows, cols):
        """-> (input pointer, input row stride, output buffer object, its pointer, read-back function)"""
        import numpy as np
        obuf = np.full((rows, cols), np.nan)
        return xa.ctypes.data, xa.shape[1], obuf, obuf.ctypes.data, lambda b: b


class DeviceTier(_DeviceTier):
    def buffers(self, xa, rows, cols):
        t = self.t
        xin = t.from_numpy(xa).to("cuda:0")
        obuf = t.full((rows, cols), float("nan"), dtype=t.float64, device="cuda:0")
        t.cuda.synchronize()
        self._keep = xin

        def back(b):
            t.cuda.synchronize()
            return b.cpu().numpy()
        return xin.data_ptr(), xin.stride(0), obuf, obuf.data_ptr(), back


# ---- the sanitizer program's table --------------------------------------------------------------------------------------
def dump(out):
    def opts(o):
        return ",".join("%s=%d" % kv for kv in sorted(o.items()))
    for nt in range(1, 15):
        for kind in ("hbup", "hbdown"):
            e = [a for a in PART_A if a["kind"] == kind and a["ntaps"] == nt][0]
            d = hb_descriptor(e)
            out.write("stage|%d|%r|0|0|0|%d|%d|%d||0=%s\n" % (d[0], d[1], d[5], d[6], A_MAXIN, "k_" + kind))
    for e in PART_B_UP:
        want = _expected_symbols(e, 1, True, "k_hbcascade", "k_hbup")
        out.write("chain|0|%r|%r|%r|%r|0|0|%d|%s|%s\n" % (e["src"], e["dst"], TB, e["att"], e["maxin"], opts(e["opts"]),
                                                        ",".join("%d=%s" % (s, v or "") for s, v in sorted(want.items()))))
    for e in PART_B_DOWN:
        want = _expected_symbols(e, 0, True, "k_hbdcascade", "k_hbdown")
        out.write("chain|0|%r|%r|%r|%r|0|0|%d|%s|%s\n" % (e["src"], e["dst"], TB, e["att"], e["maxin"], opts(e["opts"]),
                                                        ",".join("%d=%s" % (s, v or "") for s, v in sorted(want.items()))))


if __name__ == "__main__":
    if sys.argv[1:] == ["--dump"]:
        dump(sys.stdout)
    else:
        sys.exit("usage: python tests/stage_census.py --dump")
