"""The taps of the 4x true-peak interpolator (include/r8bsrc.h "true peak"; csrc/r8b_truepeak.h).

Prototype, 48 taps, a Kaiser-windowed sinc (beta = 8) that is a Nyquist filter for the factor 4:
    g[i] = sinc((i - 24) / 4) * I0(8 * sqrt(1 - ((i - 24) / 24)^2)) / I0(8),   i = 0 .. 47
computed with numpy for i <= 24 and mirrored, so that the table is exactly symmetric.  Phase 0 (g[4 t]) is the unit
sample at t = 6 plus residues of 1e-17, which are dropped: phase 0 is the delayed input itself.  Phase p = 1, 2, 3 is
g[4 t + p], t = 0 .. 11.

Writes the literals as C hex floats between the markers of csrc/r8b_truepeak.h and tests/golden/true_peak_taps.json,
and prints the accuracy figures the header quotes.  The COMMITTED literals are the definition: a numpy whose sinc or i0
rounds another way must not change them (--check compares and writes nothing).
    python tools/gen_true_peak.py [--check]"""
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "r8brain-free-src_amd", "csrc", "r8b_truepeak.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "true_peak_taps.json")
BEGIN, END = "// BEGIN GENERATED (tools/gen_true_peak.py)", "// END GENERATED"
PHASES, TAPS, BETA = 4, 12, 8.0


def prototype():
    n = PHASES * TAPS
    g = np.zeros(n)
    for i in range(n // 2 + 1):
        t = (i - n // 2) / (n // 2)
        g[i] = np.sinc((i - n // 2) / PHASES) * np.i0(BETA * np.sqrt(1.0 - t * t)) / np.i0(BETA)
    for i in range(n // 2 + 1, n):
        g[i] = g[n - i]
    return g


def phases(g):
    """[3][12]: row p - 1 is g[4 t + p]"""
    return [[float(g[PHASES * t + p]) for t in range(TAPS)] for p in range(1, PHASES)]


def literals(rows):
    body = ",\n".join("\t{ " + ", ".join(float(v).hex() for v in row) + " }" for row in rows)
    return "#define R8B_TP_TAPS { \\\n" + body.replace("\n", " \\\n") + " }"


def accuracy(rows):
    """(largest over-read in dB of a stationary tone up to 0.45 fs, the frequency it is at, largest under-read in dB at
    0.4 fs): |H_p(f)| is the gain of phase p for a tone, phase 0's is 1; an ideal 4x grid under-reads by cos(pi f / 4)"""
    h = np.array(rows)
    f = np.linspace(0.0, 0.45, 4501)
    e = np.exp(-2j * np.pi * np.outer(f, np.arange(TAPS)))
    gain = np.abs(e @ h.T)
    over = 20 * np.log10(np.maximum(gain.max(axis=1), 1.0))
    k = int(np.argmax(over))
    # the under-read at 0.4 fs: a tone of amplitude 1 and phase phi on the 4x grid (five frames are a period), the phase
    # that reads lowest
    c = np.concatenate([[np.exp(-2j * np.pi * 0.4 * (TAPS // 2))], h @ np.exp(-2j * np.pi * 0.4 * np.arange(TAPS))])
    grid = np.outer(c, np.exp(2j * np.pi * 0.4 * np.arange(5))).reshape(-1)
    phi = np.exp(1j * np.linspace(0.0, 2 * np.pi, 7201))
    under = -20 * np.log10(np.abs(np.real(np.outer(phi, grid))).max(axis=1).min())
    return float(over[k]), float(f[k]), float(under)


def main():
    check = "--check" in sys.argv[1:]
    g = prototype()
    rows = phases(g)
    dropped = max(abs(float(g[PHASES * t])) for t in range(TAPS) if t != TAPS // 2)
    assert g[PHASES * TAPS // 2] == 1.0 and dropped < 1e-15, (g[PHASES * TAPS // 2], dropped)
    assert rows[0] == rows[2][::-1] and rows[1] == rows[1][::-1]
    small = min(abs(v) for row in rows for v in row)
    over, f_over, under = accuracy(rows)
    print("36 taps, smallest %.3g; phase 0 residues dropped, largest %.3g" % (small, dropped))
    print("stationary tones up to 0.45 fs over-read by at most %.4f dB (at %.4f fs)" % (over, f_over))
    print("under-read at 0.4 fs at most %.3f dB (the 4x grid's own: %.3f dB)" %
          (under, -20 * np.log10(np.cos(np.pi * 0.4 / 4))))
    golden = {"phases": PHASES, "taps": TAPS, "delay": TAPS // 2,
              "g": [[float(v).hex() for v in row] for row in rows]}
    text = open(HEADER).read()
    m = re.search(re.escape(BEGIN) + r"\n(.*?)\n" + re.escape(END), text, re.S)
    assert m, "markers missing in " + HEADER
    if check:
        assert m.group(1) == literals(rows), "csrc/r8b_truepeak.h differs from what this numpy computes"
        assert json.load(open(GOLDEN)) == golden, "tests/golden/true_peak_taps.json differs"
        print("committed literals: identical")
        return
    with open(HEADER, "w") as fh:
        fh.write(text[:m.start(1)] + literals(rows) + text[m.end(1):])
    with open(GOLDEN, "w") as fh:
        json.dump(golden, fh, indent=1)
        fh.write("\n")
    print("wrote %s and %s" % (os.path.relpath(HEADER, ROOT), os.path.relpath(GOLDEN, ROOT)))


if __name__ == "__main__":
    main()
