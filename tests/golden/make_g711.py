"""Writes tests/golden/g711.npz: the four ITU-T G.711 tables of the standard library's audioop at width 2, which
include/r8bsrc.h's statement of R8B_PCM_ULAW / R8B_PCM_ALAW is held against (tests/test_pcm8.py).  The tests read the
file and never import audioop, which newer Pythons no longer ship.

    ulaw_decode[256], alaw_decode[256]      int16: the 16-bit linear value of every code
    ulaw_encode[65536], alaw_encode[65536]  uint8: the code of every 16-bit linear value s, at index s + 32768

Run from anywhere: python tests/golden/make_g711.py"""
import audioop
import os

import numpy as np


def main():
    codes = bytes(range(256))
    linear = np.arange(-32768, 32768, dtype="<i2").tobytes()
    tables = {
        "ulaw_decode": np.frombuffer(audioop.ulaw2lin(codes, 2), dtype="<i2").astype(np.int16),
        "alaw_decode": np.frombuffer(audioop.alaw2lin(codes, 2), dtype="<i2").astype(np.int16),
        "ulaw_encode": np.frombuffer(audioop.lin2ulaw(linear, 2), dtype=np.uint8).copy(),
        "alaw_encode": np.frombuffer(audioop.lin2alaw(linear, 2), dtype=np.uint8).copy(),
    }
    assert tables["ulaw_decode"].shape == tables["alaw_decode"].shape == (256,)
    assert tables["ulaw_encode"].shape == tables["alaw_encode"].shape == (65536,)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g711.npz")
    np.savez_compressed(out, **tables)
    print("%s: %d bytes" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
