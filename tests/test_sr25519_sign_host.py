"""The sr25519 signing code on the CPU: tests/host/srsigncheck.cpp compiles
cometbft_amd/csrc/sr25519_sign.h (and sr25519.h, merlin.h, sha512.h, quad.h
under it) with CMTV_HD = inline, the headers' operand-bound assertions on, and
AddressSanitizer + UBSan; every result is compared bit-exact with
oracle/sr25519_ref.py, hashlib and Python integers."""
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
import sr25519_sign_cases as C  # noqa: E402

from oracle import sr25519_ref as S  # noqa: E402

SRC = os.path.join(ROOT, "tests", "host", "srsigncheck.cpp")
BIN = os.path.join(ROOT, "build", "srsigncheck")
P, L = S.P, S.L
# the 4-torsion of edwards25519: what ristretto255 quotients out
TORSION = [(0, P - 1), (S.SQRT_M1, 0), (P - S.SQRT_M1, 0)]


@pytest.fixture(scope="module")
def check():
    return hostbuild.build(SRC, BIN, ["-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def run(binary, mode, inp):
    r = subprocess.run([binary, mode], input=inp, capture_output=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-600:])
    return r.stdout


def run_prim(binary, records):
    return run(binary, "prim", struct.pack("<I", len(records)) + b"".join(records))


def le(x):
    return x.to_bytes(32, "little")


def affine(p):
    zi = pow(p[2], P - 2, P)
    return p[0] * zi % P, p[1] * zi % P


def point_record(x, y, z=1):
    return struct.pack("<I", 1) + le(x) + le(y) + le(z)


def msg_field(m):
    return struct.pack("<I", len(m)) + m


def test_whole_signatures_match_the_restatement(check):
    idx, msgs = C.sign_inputs()
    ks = C.keys(C.N_SIGN_KEYS)
    inp = struct.pack("<I", len(msgs)) + b"".join(ks[i] + msg_field(m) for i, m in zip(idx, msgs))
    out = np.frombuffer(run(check, "sign", inp), np.uint8).reshape(len(msgs), 64)
    bad = np.nonzero((out != C.expected_signatures()).any(axis=1))[0]
    assert bad.size == 0, bad[:10]
    assert (out[:, 63] & 0x80).all()
    assert sorted(set(len(m) for m in msgs)) == C.MSG_LENGTHS


def test_public_keys_and_addresses(check):
    n = 80
    out = np.frombuffer(run(check, "pub", struct.pack("<I", n) + b"".join(C.keys(n))), np.uint8).reshape(n, 52)
    pk, addr = C.expected_pubkeys(257)
    assert np.array_equal(out[:, :32], pk[:n]) and np.array_equal(out[:, 32:], addr[:n])


def test_encode_of_the_pinned_multiples(check):
    """RFC 9496 appendix A.1: the encodings of [i]B, i = 0 .. as far as the corpus pins them."""
    with open(os.path.join(ROOT, "tests", "golden", "sr25519_corpus.json")) as f:
        pins = json.load(f)["pins"]["ristretto255_multiples"]
    assert len(pins) >= 8 and pins[0] == "00" * 32
    got = run_prim(check, [struct.pack("<I", 2) + le(i) for i in range(len(pins))])
    assert got == b"".join(bytes.fromhex(h) for h in pins)
    # and through the point form, from the restatement's coordinates
    pts = [affine(S.scalar_mult(i, S.B)) for i in range(len(pins))]
    assert run_prim(check, [point_record(x, y) for x, y in pts]) == got


def test_encode_edge_cases(check):
    # the identity's coset: all four encode to zero
    recs = [point_record(0, 1)] + [point_record(x, y) for x, y in TORSION]
    assert run_prim(check, recs) == bytes(32) * 4
    # P + T encodes as P, and the four representatives take both values of
    # rotate and of the y negation
    Pt = S.scalar_mult(12345, S.B)
    reps = [Pt] + [S.point_add(Pt, (x, y, 1, x * y % P)) for x, y in TORSION]
    want = S.ristretto_encode(Pt)
    assert all(S.ristretto_encode(r) == want for r in reps)
    br = [C.encode_branches(r) for r in reps]
    assert {b[0] for b in br} == {False, True} and {b[1] for b in br} == {False, True}
    recs = [point_record(*affine(r)) for r in reps]
    # the same points with Z != 1
    rng = random.Random(9496)
    zs = [2, P - 1, rng.randrange(2, P), rng.randrange(2, P)]
    recs += [point_record(*affine(r), z) for r, z in zip(reps, zs)]
    assert run_prim(check, recs) == want * 8


def test_synthetic_keys_take_every_encode_branch(check):
    """rotate, the y negation and the final absolute value: all eight
    combinations occur among the first 64 synthetic keys (whose encodings the
    other tests compare), so no select of ristretto_encode goes one way only."""
    minis = C.keys(66)[2:]
    combos = [C.encode_branches(S.scalar_mult(S.expand_mini(m)[0], S.B)) for m in minis]
    counts = {c: combos.count(c) for c in set(combos)}
    print("encode branches (rotate, negate, abs) over 64 keys:", sorted(counts.items()))
    assert len(counts) == 8, counts


def test_key_expansion(check):
    minis = C.keys(34)
    got = run_prim(check, [struct.pack("<I", 3) + m for m in minis])
    exp = b""
    for m in minis:
        key, nonce = S.expand_mini(m)
        assert 2**251 <= key < 2**252 < L
        exp += le(key) + nonce
    assert got == exp


def test_witness_at_each_message_length(check):
    rng = random.Random(57)
    recs, exp = [], []
    for n in C.MSG_LENGTHS:
        for nonce in (bytes(32), b"\xff" * 32, rng.randbytes(32), rng.randbytes(32)):
            m = rng.randbytes(n)
            recs.append(struct.pack("<I", 4) + nonce + msg_field(m))
            exp.append(le(C.witness(nonce, m)))
    assert run_prim(check, recs) == b"".join(exp)
    # the witness is sign()'s: one whole signature's R is ENCODE([r]B)
    mini, m = C.keys(3)[2], b"witness"
    r = C.witness(S.expand_mini(mini)[1], m)
    assert S.sign(mini, m)[:32] == S.ristretto_encode(S.scalar_mult(r, S.B))


def test_sign_with_chosen_key_and_witness(check):
    """r = 0 (R the identity, encoded as zeros), 1 and L - 1, and seeded ones."""
    rng = random.Random(5)
    recs, exp = [], []
    for r in (0, 1, L - 1, rng.randrange(L), rng.randrange(L)):
        for a in (S.expand_mini(C.keys(3)[2])[0], 1, L - 1, rng.randrange(L)):
            m = rng.randbytes(rng.choice(C.MSG_LENGTHS))
            pk = S.ristretto_encode(S.scalar_mult(a, S.B))
            r_enc = S.ristretto_encode(S.scalar_mult(r, S.B))
            recs.append(struct.pack("<I", 5) + le(a) + le(r) + pk + msg_field(m))
            exp.append(S.sign_encoded(a, r, m, pk, r_enc))
            assert S.verify(pk, m, exp[-1])
    out = run_prim(check, recs)
    assert out == b"".join(exp)
    assert out[:32] == bytes(32)
