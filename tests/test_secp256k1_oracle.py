"""CPU pins of the secp256k1 oracle (tests/secp256k1_ref.py, the big-integer
restatement of crypto/secp256k1/secp256k1.go:192-217), of the corpus generated
from it and of the pure-Python RIPEMD-160 behind Secp256k1PubKey.address().

Parity with btcec itself is unpinned (no Go toolchain): DESIGN.md section 2.
"""
import hashlib
import json
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_secp256k1_corpus as GEN  # noqa: E402
import secp256k1_ref as S  # noqa: E402

from cometbft_amd.ripemd160 import ripemd160  # noqa: E402


@pytest.fixture(scope="module")
def kat():
    with open(os.path.join(ROOT, "tests", "golden", "secp256k1_kat.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def corpus_doc():
    with open(os.path.join(ROOT, "tests", "golden", "secp256k1_corpus.json")) as f:
        return json.load(f)


def test_reference_key_vector(kat):
    """secp256k1_test.go:24-30: priv -> pub -> address."""
    k = kat["key"]
    pub = S.pubkey_from_priv(bytes.fromhex(k["priv"]))
    assert pub.hex() == k["pub"]
    assert ripemd160(hashlib.sha256(pub).digest()).hex() == k["address"]


def test_ripemd160_strings(kat):
    for v in kat["ripemd160"]:
        assert ripemd160(v["msg"].encode()).hex() == v["digest"], v["msg"]


def test_group_order_and_endomorphism():
    assert S.jmul(S.N - 1, S.G) is not None and S.jadd(S.jmul(S.N - 1, S.G), S.G) is None
    assert S.gmul(S.N) is None
    rng = random.Random(1)
    for _ in range(4):
        x, y = S.to_affine(S.gmul(rng.randrange(1, S.N)))
        assert S.to_affine(S.jmul(S.LAMBDA, (x, y, 1))) == (S.BETA * x % S.P, y)
    assert pow(S.LAMBDA, 3, S.N) == 1 and pow(S.BETA, 3, S.P) == 1


def test_sign_then_verify_50_keys():
    rng = random.Random(50)
    for i in range(50):
        priv = rng.randbytes(32)
        pk = S.pubkey_from_priv(priv)
        msg = rng.randbytes(rng.randrange(0, 200))
        sig = S.sign(priv, msg)
        assert int.from_bytes(sig[32:], "big") <= S.HALF_N
        assert S.verify(pk, msg, sig)
        assert not S.verify(pk, msg + b"x", sig)
        s = int.from_bytes(sig[32:], "big")
        assert not S.verify(pk, msg, sig[:32] + (S.N - s).to_bytes(32, "big")), "high-S twin"


def test_corpus_is_what_the_generator_produces(corpus_doc):
    """The committed file equals the generator's output, whose verdicts are
    secp256k1_ref.verify's (asserted per vector against the category inside
    build())."""
    assert GEN.build() == corpus_doc


def test_every_category_present_with_its_verdict(corpus_doc):
    cats = {}
    for v in corpus_doc["vectors"]:
        cats.setdefault(v["cat"], set()).add(v["valid"])
    assert set(cats) == GEN.VALID_CATS | GEN.INVALID_CATS
    for c, verdicts in cats.items():
        assert verdicts == {1 if c in GEN.VALID_CATS else 0}, c
    ex = [v for v in corpus_doc["vectors"] if v["cat"] == "exceptional"]
    assert len(ex) == 64 * len(GEN.EXCEPTIONAL_D)
    assert {v["pk"] for v in ex} == {S.pubkey_from_priv(d.to_bytes(32, "big")).hex() for d in GEN.EXCEPTIONAL_D}
    honest_lens = {len(v["msg"]) // 2 for v in corpus_doc["vectors"] if v["cat"] == "honest"}
    assert honest_lens == set(GEN.LENGTHS)
    # the shuffle: every full wavefront of the corpus order mixes both verdicts
    valid = [v["valid"] for v in corpus_doc["vectors"]]
    for w in range(len(valid) // 64):
        assert 0 < sum(valid[64 * w: 64 * w + 64]) < 64, w


def test_infinity_vectors_discriminate(corpus_doc):
    """[u1]G + [u2]Q is the point at infinity in every `infinity` vector:
    rejected by the oracle, accepted by the verifier without the Z != 0 test
    (X = 0 = r * 0), both recomputed from the committed JSON; several r, one of
    them with r + n < p, both key parities, s at and below (n - 1) / 2."""
    vecs = [v for v in corpus_doc["vectors"] if v["cat"] == "infinity"]
    assert len(vecs) >= 8
    rs, ss = set(), set()
    for v in vecs:
        pk, msg, sig = bytes.fromhex(v["pk"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"])
        r, s = int.from_bytes(sig[:32], "big") % S.N, int.from_bytes(sig[32:], "big")
        w = pow(s, S.N - 2, S.N)
        assert S.jadd(S.gmul(S.msg_scalar(msg) * w), S.jmul(r * w, S.parse_pubkey(pk))) is None
        assert v["valid"] == 0 and not S.verify(pk, msg, sig) and S.verify_without_z_test(pk, msg, sig), v
        rs.add(r)
        ss.add(s)
    assert len(rs) >= 8 and any(r + S.N < S.P for r in rs) and any(r + S.N >= S.P for r in rs)
    assert {S.HALF_N, S.HALF_N - 1} <= ss and max(ss) == S.HALF_N
    assert {v["pk"][:2] for v in vecs} == {"02", "03"}
    # the lenient verifier is the oracle everywhere else
    for v in corpus_doc["vectors"][::9]:
        if v["cat"] != "infinity":
            args = bytes.fromhex(v["pk"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"])
            assert S.verify_without_z_test(*args) == bool(v["valid"])


def test_constructed_edge_vectors(corpus_doc):
    """The constructed vectors are what their categories say: byte values at
    or above n in reduce_quirk, a nonce point with x in [n, p) in x_ge_n."""
    for v in corpus_doc["vectors"]:
        sig = bytes.fromhex(v["sig"])
        r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
        if v["cat"] == "reduce_quirk":
            assert r >= S.N or s >= S.N
        if v["cat"] == "x_ge_n":
            q = S.parse_pubkey(bytes.fromhex(v["pk"]))
            w = pow(s % S.N, S.N - 2, S.N)
            x = S.to_affine(S.jadd(S.gmul(S.msg_scalar(bytes.fromhex(v["msg"])) * w), S.jmul(r % S.N * w, q)))[0]
            assert S.N <= x < S.P and x - S.N == r % S.N
    assert S.lift_x(1, 0) is not None and S.lift_x(S.N + 1, 0) is None and S.lift_x(S.N + 2, 0) is not None
