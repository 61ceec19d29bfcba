"""The secp256k1 device code on the CPU: tests/host/secpcheck.cpp compiles
cometbft_amd/csrc/secp256k1.h (fp256k1.h, sc256k1.h, sha256.h) with
CMTV_HD = inline and the headers' operand-bound assertions on.

  * the kernel's per-signature function over the whole corpus, bit-exact
  * the primitives against Python integers and hashlib, on operands at the
    stated limb bounds and on the values 0, 1, p-1, p, n-1, n, 2^256-1
"""
import hashlib
import json
import os
import random
import struct
import subprocess
import sys

import numpy as np
import pytest

from tests.host import hostbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import secp256k1_ref as S  # noqa: E402

SRC = os.path.join(ROOT, "tests", "host", "secpcheck.cpp")
BIN = os.path.join(ROOT, "build", "secpcheck")
P, N = S.P, S.N
M26, M22 = (1 << 26) - 1, (1 << 22) - 1
SPECIAL = [0, 1, P - 1, P, N - 1, N, 2**256 - 1]


@pytest.fixture(scope="module")
def secpcheck():
    return hostbuild.build(SRC, BIN, ["-std=c++17"])


def limbs_of(x):
    """Canonical limbs of a value below 2^256 (limb 9: 22 bits)."""
    return [(x >> (26 * i)) & M26 for i in range(10)]


def value_of(limbs):
    return sum(v << (26 * i) for i, v in enumerate(limbs))


def at_magnitude(m, rng=None):
    """Limbs at (rng None) or randomly below the magnitude-m bound."""
    top = [2 * m * M26] * 9 + [2 * m * M22]
    return top if rng is None else [rng.randrange(t + 1) for t in top]


def pack_limbs(limbs):
    return struct.pack("<10I", *limbs)


def run_prim(binary, records):
    inp = struct.pack("<I", len(records)) + b"".join(records)
    r = subprocess.run([binary, "prim"], input=inp, capture_output=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-400:])
    return r.stdout


def ints(out, count):
    assert len(out) == 32 * count
    return [int.from_bytes(out[32 * i: 32 * i + 32], "little") for i in range(count)]


def test_corpus_bit_exact(secpcheck):
    with open(os.path.join(ROOT, "tests", "golden", "secp256k1_corpus.json")) as f:
        vecs = json.load(f)["vectors"]
    buf = [struct.pack("<I", len(vecs))]
    for v in vecs:
        m = bytes.fromhex(v["msg"])
        buf += [bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"]), struct.pack("<I", len(m)), m]
    r = subprocess.run([secpcheck], input=b"".join(buf), capture_output=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-400:])
    got = np.frombuffer(r.stdout, np.uint8)
    exp = np.array([v["valid"] for v in vecs], np.uint8)
    assert got.shape == exp.shape
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, [(int(i), vecs[int(i)]["cat"], int(got[i])) for i in bad[:10]]


def test_field_primitives(secpcheck):
    rng = random.Random(26)
    ops = [limbs_of(x) for x in SPECIAL] + [at_magnitude(8), at_magnitude(1)] + \
          [at_magnitude(8, rng) for _ in range(6)] + [limbs_of(rng.randrange(P)) for _ in range(6)]
    recs, exp = [], []
    for a in ops:
        for b in ops:
            recs.append(struct.pack("<I", 1) + pack_limbs(a) + pack_limbs(b))
            exp.append(value_of(a) * value_of(b) % P)
        recs.append(struct.pack("<I", 2) + pack_limbs(a))
        exp.append(value_of(a) ** 2 % P)
    # subtraction: b at and below each magnitude the formulas use
    for mb in (1, 2, 3, 7):
        for b in [at_magnitude(mb), [0] * 10] + [at_magnitude(mb, rng) for _ in range(4)]:
            for a in ops[:9] + [at_magnitude(3, rng)]:
                recs.append(struct.pack("<I", 3) + pack_limbs(a) + pack_limbs(b) + struct.pack("<I", mb))
                exp.append((value_of(a) - value_of(b)) % P)
    # normalisation up to magnitude 16, and values just around p
    norm = ops + [at_magnitude(16), limbs_of(P + 1), limbs_of(P - 2), limbs_of(2**256 - 2)] + \
        [at_magnitude(16, rng) for _ in range(20)]
    for a in norm:
        recs.append(struct.pack("<I", 4) + pack_limbs(a))
        exp.append(value_of(a) % P)
    for a in ops:
        recs.append(struct.pack("<I", 5) + pack_limbs(a))
        exp.append(pow(value_of(a), (P + 1) // 4, P))
    got = ints(run_prim(secpcheck, recs), len(recs))
    bad = [i for i, (g, e) in enumerate(zip(got, exp)) if g != e]
    assert not bad, bad[:10]


def test_scalar_primitives(secpcheck):
    rng = random.Random(8)
    vals = SPECIAL + [N + 1, N - 2, S.HALF_N, S.HALF_N + 1, 2**256 - N, 2**128] + \
        [rng.randrange(2**256) for _ in range(12)]
    recs, exp = [], []
    for a in vals:
        recs.append(struct.pack("<I", 6) + a.to_bytes(32, "big"))
        exp.append(a % N)
        for b in vals:
            recs.append(struct.pack("<I", 7) + a.to_bytes(32, "big") + b.to_bytes(32, "big"))
            exp.append(a * b % N)
        recs.append(struct.pack("<I", 8) + a.to_bytes(32, "big"))
        exp.append(pow(a % N, N - 2, N))
    got = ints(run_prim(secpcheck, recs), len(recs))
    bad = [i for i, (g, e) in enumerate(zip(got, exp)) if g != e]
    assert not bad, bad[:10]


def test_sha256(secpcheck):
    rng = random.Random(256)
    lens = list(range(0, 70)) + [119, 120, 127, 128, 129, 183, 184, 300, 1000]
    msgs = [rng.randbytes(n) for n in lens]
    recs = [struct.pack("<II", 9, len(m)) + m for m in msgs]
    got = ints(run_prim(secpcheck, recs), len(recs))
    for m, g in zip(msgs, got):
        assert g == int.from_bytes(hashlib.sha256(m).digest(), "big"), len(m)


def test_fixed_table_rows(secpcheck):
    """secp_gtab_row(j, d) = [d 256^j]G, the rows the runtime's build kernel
    writes: the first, last and a few middle rows (the corpus test reads all)."""
    rows = [(0, 1), (0, 2), (0, 128), (1, 1), (7, 77), (31, 128), (32, 1), (32, 128)]
    recs = [struct.pack("<III", 10, j, d) for j, d in rows]
    got = ints(run_prim(secpcheck, recs), 3 * len(recs))
    for k, (j, d) in enumerate(rows):
        x, y, z = got[3 * k: 3 * k + 3]
        zi = pow(z, P - 2, P)
        assert z != 0 and (x * zi % P, y * zi % P) == S.to_affine(S.jmul(d * 256**j, S.G)), (j, d)
