"""CPU test of the verdict-bitmap tail shared by the host-buffer calls
(cometbft_amd/csrc/verdict_bits.h, host-compiled by tests/host/bitscheck.cpp):
mask the bits past n, count the invalid verdicts, copy out, expand to bytes,
and the reverse pack -- against a plain Python reference, at one bit, one
word less / exactly / plus one bit, and two words exactly / plus one bit."""
import os
import struct
import subprocess

import numpy as np

from test_host_math import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "bitscheck.cpp")
BIN = os.path.join(ROOT, "build", "bitscheck")

SIZES = (1, 63, 64, 65, 128, 129)


def test_bitmap_tail_and_pack():
    binary = _build(SRC, BIN, ["-std=c++17"])
    rng = np.random.default_rng(65)
    cases = []
    for n in SIZES:
        for density in (0.0, 0.5, 0.9, 1.0):
            verdicts = [int(rng.random() < density) for _ in range(n)]
            words = (n + 63) // 64
            # what a kernel may leave: the verdicts below n, every bit above n set
            x = sum(v << i for i, v in enumerate(verdicts)) | ((1 << (64 * words)) - (1 << n))
            cases.append((n, verdicts, [(x >> (64 * w)) & (2**64 - 1) for w in range(words)]))
    buf = b"".join(struct.pack("<Q", n) + struct.pack(f"<{len(ws)}Q", *ws) for n, _, ws in cases)
    out = subprocess.run([binary], input=buf, capture_output=True, check=True).stdout
    pos = 0
    for n, verdicts, ws in cases:
        words = len(ws)
        padded = (n + 7) // 8 * 8
        invalid, = struct.unpack_from("<Q", out, pos)
        pos += 8
        bitmap = struct.unpack_from(f"<{words}Q", out, pos)
        pos += 8 * words
        valid = list(out[pos:pos + n])
        pos += padded
        packed = struct.unpack_from(f"<{words}Q", out, pos)
        pos += 8 * words
        want = sum(v << i for i, v in enumerate(verdicts))  # nothing at or past n
        assert valid == verdicts, n
        assert invalid == n - sum(verdicts), n
        assert sum(w << (64 * k) for k, w in enumerate(bitmap)) == want, n
        assert sum(w << (64 * k) for k, w in enumerate(packed)) == want, n
    assert pos == len(out)
