"""Vectors for the registered-key secp256k1 tests (CPU host build and GPU):
the corpus with its keys indexed in order of first appearance, and directed
signatures whose u2 = r / s takes a chosen value, computed with
tests/secp256k1_ref.py."""
import json
import os
import random

import secp256k1_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# u + 0x8080..80 carries out of bit 255 from this u on: the comb's digit 32
CARRY_FROM = 2**256 - int.from_bytes(b"\x80" * 32, "big")
# u2 values: digit +1 alone; n - 1; digit +127; digit -128 with its borrow
# into digit 1; the last value without the carry digit and the first with it
DIRECTED_U2 = [1, S.N - 1, 0x7F, 0x80, CARRY_FROM - 1, CARRY_FROM]


def corpus_indexed():
    """(keys, key_idx, vectors): the corpus's distinct keys in order of first
    appearance and each vector's index into them."""
    with open(os.path.join(ROOT, "tests", "golden", "secp256k1_corpus.json")) as f:
        vecs = json.load(f)["vectors"]
    keys, where, idx = [], {}, []
    for v in vecs:
        pk = bytes.fromhex(v["pk"])
        if pk not in where:
            where[pk] = len(keys)
            keys.append(pk)
        idx.append(where[pk])
    return keys, idx, vecs


def directed(t, msg, rng):
    """(pk, sig) valid for msg with r / s = t mod n."""
    assert 0 < t < S.N
    ti = pow(t, S.N - 2, S.N)
    for _ in range(200):
        k = rng.randrange(1, S.N)
        rpoint = S.gmul(k)
        x, _ = S.to_affine(rpoint)
        r = x
        if not 0 < r < S.N:
            continue
        s = r * ti % S.N
        if not 0 < s <= S.HALF_N:
            continue
        q = S.recover_key(rpoint, r, s, msg)
        if q is None:
            continue
        pk = S.encode_point(q)
        sig = r.to_bytes(32, "big") + s.to_bytes(32, "big")
        assert S.verify(pk, msg, sig) and not S.verify(pk, msg + b"x", sig)
        return pk, sig
    raise AssertionError(f"no signature with u2 = {t:#x}")


def directed_vectors():
    """[(pk, sig, msg, valid)]: for each DIRECTED_U2 the valid signature, then
    the same signature over msg + b"x"."""
    rng = random.Random(0x5EC9)
    out = []
    for i, t in enumerate(DIRECTED_U2):
        msg = b"directed u2 %d" % i
        pk, sig = directed(t, msg, rng)
        out += [(pk, sig, msg, 1), (pk, sig, msg + b"x", 0)]
    return out
