"""The registered-key secp256k1 device code on the CPU:
tests/host/secpkeyedcheck.cpp compiles cometbft_amd/csrc/secp256k1.h with
CMTV_HD = inline and the headers' operand-bound assertions on, builds key
tables with secp_qcomb_position (the function k_secp_qcomb_build calls) and
runs secp_verify_keyed_one (the function k_verify_secp256k1_keyed calls).

  * table rows against big integers, for a random key, Q = G and a 03 key
  * rejected keys: ok = 0, every row the point at infinity, no assertion
  * the whole corpus by key index, bit-exact
  * directed u2 = r / s values at the comb's digit edges and carry row
  * the corpus again in an AddressSanitizer + UBSan build of the program
"""
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
import secp256k1_keyed_vectors as V  # noqa: E402
import secp256k1_ref as S  # noqa: E402

SRC = os.path.join(ROOT, "tests", "host", "secpkeyedcheck.cpp")
BIN = os.path.join(ROOT, "build", "secpkeyedcheck")
BIN_SAN = os.path.join(ROOT, "build", "secpkeyedcheck_san")
P = S.P
ROWS = [(0, 1), (0, 2), (0, 128), (1, 1), (7, 77), (31, 128), (32, 1), (32, 128)]


@pytest.fixture(scope="module")
def check():
    return hostbuild.build(SRC, BIN, ["-std=c++17"])


@pytest.fixture(scope="module")
def corpus():
    return V.corpus_indexed()


def keys_blob(keys):
    return struct.pack("<I", len(keys)) + b"".join(keys)


def run(binary, args, inp):
    r = subprocess.run([binary] + args, input=inp, capture_output=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-600:])
    return r.stdout


def verify(binary, keys, entries):
    """ok bytes and verdicts for entries [(key_idx, sig, msg)]."""
    buf = [keys_blob(keys), struct.pack("<I", len(entries))]
    for k, sig, m in entries:
        buf += [struct.pack("<I", k), sig, struct.pack("<I", len(m)), m]
    out = run(binary, [], b"".join(buf))
    assert len(out) == len(keys) + len(entries)
    return np.frombuffer(out[: len(keys)], np.uint8), np.frombuffer(out[len(keys):], np.uint8)


def rows_of(binary, keys, recs):
    """ok bytes, all-infinity bytes, and (X, Y, Z) for recs [(key, j, d)]."""
    inp = keys_blob(keys) + struct.pack("<I", len(recs)) + b"".join(struct.pack("<III", *r) for r in recs)
    out = run(binary, ["rows"], inp)
    nk = len(keys)
    assert len(out) == 2 * nk + 96 * len(recs)
    vals = [int.from_bytes(out[2 * nk + 32 * i: 2 * nk + 32 * i + 32], "little") for i in range(3 * len(recs))]
    return out[:nk], out[nk: 2 * nk], [tuple(vals[3 * i: 3 * i + 3]) for i in range(len(recs))]


def test_table_rows(check):
    """Row (j, d) of a key's table = [d 256^j]Q."""
    rng = random.Random(33)
    k03 = next(pk for pk in (S.pubkey_from_priv(rng.randbytes(32)) for _ in range(64)) if pk[0] == 3)
    keys = [S.pubkey_from_priv(rng.randbytes(32)), S.encode_point(S.G), k03]
    recs = [(k, j, d) for k in range(len(keys)) for j, d in ROWS]
    ok, inf, pts = rows_of(check, keys, recs)
    assert ok == b"\x01\x01\x01" and inf == b"\x00\x00\x00"
    for (k, j, d), (x, y, z) in zip(recs, pts):
        q = S.parse_pubkey(keys[k])
        zi = pow(z, P - 2, P)
        assert z != 0 and (x * zi % P, y * zi % P) == S.to_affine(S.jmul(d * 256**j, (q[0], q[1], 1))), (k, j, d)


def rejected_keys():
    rng = random.Random(34)
    good = S.pubkey_from_priv(rng.randbytes(32))
    off_curve = next(x for x in range(1, 100) if S.lift_x(x, 0) is None)
    return good, [bytes([4]) + good[1:], bytes([0]) + good[1:],        # bad prefix
                  bytes([2]) + S.P.to_bytes(32, "big"), bytes([3]) + (2**256 - 1).to_bytes(32, "big"),  # x >= p
                  bytes([2]) + off_curve.to_bytes(32, "big")]           # x^3 + 7 not a square


def test_rejected_keys(check):
    """Bad prefix, x >= p, off the curve: ok = 0, every row is (0 : 1 : 0), no
    bound assertion fires (the run exits 0), and a signature valid under the
    good neighbour is invalid under each."""
    good, bad = rejected_keys()
    keys = [bad[0], good] + bad[1:]
    recs = [(k, j, d) for k in range(len(keys)) for j, d in ROWS[:2] + ROWS[-1:]]
    ok, inf, pts = rows_of(check, keys, recs)
    assert ok == bytes([0, 1, 0, 0, 0, 0]) and inf == bytes([1, 0, 1, 1, 1, 1])
    for (k, _, _), pt in zip(recs, pts):
        assert (pt == (0, 1, 0)) == (k != 1)
    priv = random.Random(34).randbytes(32)
    assert S.pubkey_from_priv(priv) == good
    msg = b"under a rejected key"
    sig = S.sign(priv, msg)
    ok2, got = verify(check, keys, [(k, sig, msg) for k in range(len(keys))])
    assert bytes(ok2) == ok
    assert got.tolist() == [0, 1, 0, 0, 0, 0]
    assert [int(S.verify(pk, msg, sig)) for pk in keys] == got.tolist()


def corpus_entries(corpus):
    keys, idx, vecs = corpus
    return keys, [(k, bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"])) for k, v in zip(idx, vecs)]


def assert_corpus(binary, corpus):
    keys, entries = corpus_entries(corpus)
    vecs = corpus[2]
    ok, got = verify(binary, keys, entries)
    exp = np.array([v["valid"] for v in vecs], np.uint8)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, [(int(i), vecs[int(i)]["cat"], int(got[i])) for i in bad[:10]]
    # ok is the key's own verdict: what the reference's parser says
    assert ok.tolist() == [int(S.parse_pubkey(pk) is not None) for pk in keys]


def test_corpus_bit_exact(check, corpus):
    keys, _, vecs = corpus
    assert len(vecs) == 776 and len(keys) == 95
    assert sum(v["cat"] == "exceptional" for v in vecs) == 512
    assert_corpus(check, corpus)


def test_directed_u2(check):
    """u2 = 1, n - 1, 0x7F, 0x80 and both sides of the carry digit: each
    signature verifies, and does not over another message."""
    vecs = V.directed_vectors()
    assert len(vecs) == 12
    keys = [v[0] for v in vecs[::2]]
    _, got = verify(check, keys, [(i // 2, sig, msg) for i, (_, sig, msg, _) in enumerate(vecs)])
    assert got.tolist() == [v[3] for v in vecs] == [1, 0] * 6


def test_corpus_under_sanitizers(corpus):
    """The same program, AddressSanitizer + UBSan, over the corpus: a plain
    executable on the CPU."""
    san = hostbuild.build(SRC, BIN_SAN, ["-std=c++17", "-g", "-fsanitize=address,undefined",
                                         "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    assert_corpus(san, corpus)
