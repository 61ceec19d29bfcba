"""The secp256k1 signing code on the CPU: tests/host/secpsigncheck.cpp compiles
cometbft_amd/csrc/secp256k1_sign.h (and fp256k1.h, sc256k1.h, sha256.h,
secp256k1.h under it) with CMTV_HD = inline, the headers' operand-bound
assertions on, and AddressSanitizer + UBSan; every result is compared
bit-exact with tests/secp256k1_sign_ref.py, hmac, hashlib and Python integers.
"""
import hashlib
import hmac
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
import secp256k1_sign_cases as C  # noqa: E402
import secp256k1_sign_ref as R  # noqa: E402

from cometbft_amd.ripemd160 import ripemd160  # noqa: E402

SRC = os.path.join(ROOT, "tests", "host", "secpsigncheck.cpp")
BIN = os.path.join(ROOT, "build", "secpsigncheck")
P, N = S.P, S.N
M26, M22 = (1 << 26) - 1, (1 << 22) - 1


@pytest.fixture(scope="module")
def check():
    return hostbuild.build(SRC, BIN, ["-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def run(binary, mode, inp):
    r = subprocess.run([binary, mode], input=inp, capture_output=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-600:])
    return r.stdout


def run_prim(binary, records):
    return run(binary, "prim", struct.pack("<I", len(records)) + b"".join(records))


def be(x):
    return x.to_bytes(32, "big")


def test_whole_signatures_match_the_restatement(check):
    idx, msgs = C.sign_inputs()
    ks = C.keys(C.N_SIGN_KEYS)
    inp = struct.pack("<I", len(msgs)) + b"".join(ks[i] + struct.pack("<I", len(m)) + m for i, m in zip(idx, msgs))
    out = np.frombuffer(run(check, "sign", inp), np.uint8).reshape(len(msgs), 65)
    assert out[:, 0].all()
    exp, negated = C.expected_signatures()
    bad = np.nonzero((out[:, 1:] != exp).any(axis=1))[0]
    assert bad.size == 0, bad[:10]
    kat = C.KAT["signature"]
    assert out[0, 1:].tobytes().hex() == kat["r"] + kat["s"] and idx[0] == 0
    assert 64 <= negated <= 193


def test_pinned_nonce_and_signature():
    """The restatement itself against the pinned vector."""
    kat = C.KAT["signature"]
    sig, k, neg = R.sign_detail(bytes.fromhex(kat["priv"]), kat["msg"].encode())
    assert (be(k).hex(), sig.hex(), neg) == (kat["k"], kat["r"] + kat["s"], kat["low_s_negated"])
    assert S.verify(R.pubkey(bytes.fromhex(kat["priv"])), kat["msg"].encode(), sig)
    key = C.KAT["key"]
    assert R.pubkey(bytes.fromhex(key["priv"])).hex() == key["pub"]
    assert R.address(bytes.fromhex(key["pub"])).hex() == key["address"]
    for v in C.KAT["ripemd160"]:
        assert ripemd160(v["msg"].encode()).hex() == v["digest"]


def test_public_keys_and_addresses(check):
    n = 80
    inp = struct.pack("<I", n) + b"".join(C.keys(n))
    out = np.frombuffer(run(check, "pub", inp), np.uint8).reshape(n, 53)
    pk, addr = C.expected_pubkeys(257)
    assert np.array_equal(out[:, :33], pk[:n]) and np.array_equal(out[:, 33:], addr[:n])
    key = C.KAT["key"]
    i = C.SPECIAL_KEYS.index(int(key["priv"], 16))
    assert out[i, :33].tobytes().hex() == key["pub"] and out[i, 33:].tobytes().hex() == key["address"]


def test_hmac_for_each_data_length(check):
    rng = random.Random(32)
    recs, exp = [], []
    for n in (32, 33, 97):
        for key in [bytes(32), b"\xff" * 32, b"\x36" * 32, b"\x5c" * 32] + [rng.randbytes(32) for _ in range(6)]:
            for data in [bytes(n), b"\xff" * n, b"\x80" * n, rng.randbytes(n), rng.randbytes(n)]:
                recs.append(struct.pack("<II", 1, n) + key + data)
                exp.append(hmac.new(key, data, hashlib.sha256).digest())
    assert run_prim(check, recs) == b"".join(exp)


def test_nonce_steps_with_and_without_rejection(check):
    rng = random.Random(97)
    recs, exp = [], []
    for d in [1, N - 1] + [rng.randrange(1, N) for _ in range(4)]:
        for h1 in [bytes(32), be(N - 1), be(N), b"\xff" * 32, rng.randbytes(32)]:
            for retries in [(0,), (0, 1), (0, 1, 1, 1), (0, 0, 1, 0), (1, 1)]:
                h = be(int.from_bytes(h1, "big") % N)
                recs.append(struct.pack("<I", 2) + be(d) + h + struct.pack("<I", len(retries)) + bytes(retries))
                g = R.Nonce(d, h1)
                for r in retries:
                    exp.append(g.next(bool(r)) + g.K + g.V)
    assert run_prim(check, recs) == b"".join(exp)


def test_candidate_acceptance(check):
    vals = [0, 1, N - 1, N, 2**256 - 1, N + 1, 2**255]
    got = run_prim(check, [struct.pack("<I", 3) + be(v) for v in vals])
    assert list(got) == [int(R.candidate_ok(be(v))) for v in vals] == [0, 1, 1, 0, 0, 0, 1]


def test_x_to_r(check):
    xs = [N - 1, N, N + 1, P - 1, 0, 1, P - N, P - N - 1]
    got = run_prim(check, [struct.pack("<I", 4) + be(x) for x in xs])
    assert got == b"".join(be(R.r_from_x(x)) for x in xs)
    assert [R.r_from_x(x) for x in xs[:4]] == [N - 1, 0, 1, P - 1 - N]


def test_sign_with_chosen_nonces(check):
    """k at the comb's edges: every digit -128 (0x80..), 127 after the bias
    (0x7f..), digits that carry through every position into the carry row
    (0xff..fe, n - 1), alternating 0 / -1 digits. The device code takes k not
    reduced; the restatement works mod n."""
    rng = random.Random(5)
    ks = [1, N - 1, int("80" * 32, 16), int("7f" * 32, 16), 2**256 - 2, int("00ff" * 16, 16), int("ff00" * 16, 16),
          2, 2**255, 0]
    recs, exp = [], []
    for k in ks:
        for d, e in [(1, 0), (N - 1, N - 1), (rng.randrange(1, N), rng.randrange(N))]:
            recs.append(struct.pack("<I", 5) + be(d) + be(e) + be(k))
            got = R.sign_with_nonce(d, e, k % N) if k % N else None
            exp.append((got[0] if got else None))
    out = run_prim(check, recs)
    assert len(out) == 65 * len(recs)
    for i, e in enumerate(exp):
        ok, sig = out[65 * i], out[65 * i + 1: 65 * i + 65]
        assert (ok == 1) == (e is not None), i
        if e is not None:
            assert sig == e, i
    # r = 0 is the only rejection reachable by choosing k: k = 0
    assert [e is None for e in exp] == [False] * 27 + [True] * 3


def test_sign_with_nonce_rejects_s_zero(check):
    """s = 0 exactly when e = -r d: chosen so for a few k."""
    recs = []
    for k in (1, 2, 12345):
        r = S.to_affine(S.gmul(k))[0] % N
        d = 77
        recs.append(struct.pack("<I", 5) + be(d) + be((-r * d) % N) + be(k))
    out = run_prim(check, recs)
    assert [out[65 * i] for i in range(3)] == [0, 0, 0]


def limbs_of(x):
    return [(x >> (26 * i)) & M26 for i in range(10)]


def test_fp_invert(check):
    rng = random.Random(26)
    top = [2 * 8 * M26] * 9 + [2 * 8 * M22]  # the stated bound: magnitude 8
    ops = [limbs_of(x) for x in (0, 1, P - 1, 2, P - 2, P, 2**256 - 1)] + [top] + \
        [[rng.randrange(t + 1) for t in top] for _ in range(12)] + [limbs_of(rng.randrange(P)) for _ in range(12)]
    got = run_prim(check, [struct.pack("<I", 6) + struct.pack("<10I", *a) for a in ops])
    vals = [sum(v << (26 * i) for i, v in enumerate(a)) % P for a in ops]
    assert got == b"".join(be(pow(v, P - 2, P)) for v in vals)
    assert [pow(v, P - 2, P) for v in vals[:3]] == [0, 1, P - 1]


def test_ripemd160_of_a_digest(check):
    rng = random.Random(160)
    # of the golden vectors only the key's address has the 32-byte shape
    key = C.KAT["key"]
    digests = [hashlib.sha256(bytes.fromhex(key["pub"])).digest()] + [rng.randbytes(32) for _ in range(64)] + \
        [bytes(32), b"\xff" * 32]
    got = run_prim(check, [struct.pack("<I", 7) + d for d in digests])
    assert got == b"".join(ripemd160(d) for d in digests)
    assert got[:20].hex() == key["address"]


def test_private_key_range_and_derivation(check):
    vals = [0, 1, N - 1, N, N + 1, 2**256 - 1, 2**255]
    got = run_prim(check, [struct.pack("<I", 8) + be(v) for v in vals])
    assert list(got) == [0, 1, 1, 0, 0, 0, 1]
    cs = [0, 1, N - 3, N - 2, N - 1, N, N + 1, 2**256 - 1, 2**255]
    got = run_prim(check, [struct.pack("<I", 9) + be(c) for c in cs])
    assert got == b"".join(be(c % (N - 1) + 1) for c in cs)
