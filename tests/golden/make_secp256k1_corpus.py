"""Generate the secp256k1 edge-case corpus (tests/golden/secp256k1_corpus.json).

Every vector holds (pk, sig, msg) and the verdict of
secp256k1.PubKey.VerifySignature (crypto/secp256k1/secp256k1.go:192-217 of
the reference) computed by the big-integer restatement tests/secp256k1_ref.py.

Categories:
  honest          valid signatures over message lengths 0, 1, 55, 56, 63, 64,
                  65, 119, 120, 127, 128, 300 (the SHA-256 padding boundaries)
  flip_r, flip_s, flip_msg, flip_pkx
                  each honest signature with one bit flipped in r, in s, in the
                  message (not the empty one) and in the key's x
  high_s          s -> n - s: invalid (the lower-S rule)
  r_zero, s_zero, r_is_n, s_is_n          invalid
  r_max, s_max    r bytes / s bytes = 2^256 - 1: invalid, through the reduction
  reduce_quirk    VALID: r bytes = r + n and / or s bytes = s + n (values
                  >= n are reduced, not rejected). Built by key recovery: R
                  with a small on-curve x (from x = 1), a small s, a message,
                  Q = r^-1 (s R - e G)
  x_ge_n          VALID: R with x in [n, p) (from n + 2), so r = x - n and only
                  the comparison with r + n accepts; same construction
  x_ge_n_twin     the same with another r: invalid
  key_prefix      prefix byte 0x00, 0x04, 0x05: invalid
  key_x_ge_p      x = p and x = p + 1: invalid, not reduced
  key_off_curve   x^3 + 7 not a square: invalid
  key_parity      the right x with the other parity byte: the wrong key
  exceptional     keys Q = [d]G for d in {1, 2, 3, n-1, n-2, n-3, lambda,
                  n-lambda}, 64 honest signatures each: all VALID; windowed and
                  comb accumulators meet table entries equal to themselves or
                  to their negatives under these keys
  infinity        keys Q = [-e / r]G for a chosen r and message: [u1]G + [u2]Q is
                  the point at infinity for every s. Invalid, and VALID for a
                  verifier that compares X = r Z without the Z != 0 test
                  (secp256k1_ref.verify_without_z_test; both asserted here and
                  in tests/test_secp256k1_oracle.py). r = 1, 5, p - n - 1 (the
                  last with r + n < p), p - n, n - 1, bytes n + 5 and random;
                  s = (n - 1) / 2, one below it, 1 and random; both key parities
The vectors are then shuffled with a fixed seed, so valid and invalid lanes
share wavefronts.

    python tests/golden/make_secp256k1_corpus.py [--out tests/golden/secp256k1_corpus.json]
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import secp256k1_ref as S  # noqa: E402

SEED = 256
LENGTHS = [0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 300]
EXCEPTIONAL_D = [1, 2, 3, S.N - 1, S.N - 2, S.N - 3, S.LAMBDA, S.N - S.LAMBDA]
VALID_CATS = {"honest", "reduce_quirk", "x_ge_n", "exceptional"}
INVALID_CATS = {"flip_r", "flip_s", "flip_msg", "flip_pkx", "high_s", "r_zero", "s_zero", "r_is_n", "s_is_n",
                "r_max", "s_max", "x_ge_n_twin", "key_prefix", "key_x_ge_p", "key_off_curve", "key_parity", "infinity"}


def b32(x: int) -> bytes:
    return x.to_bytes(32, "big")


def on_curve_from(x: int):
    """The first x' >= x with x'^3 + 7 a square, and its even-y point."""
    while S.lift_x(x, 0) is None:
        x += 1
    return x, S.lift_x(x, 0)


def build() -> dict:
    rng = random.Random(SEED)
    vecs = []

    def add(cat, pk, msg, sig):
        vecs.append({"cat": cat, "pk": bytes(pk).hex(), "msg": bytes(msg).hex(), "sig": bytes(sig).hex()})

    privs = [rng.randbytes(32) for _ in range(6)]
    pks = [S.pubkey_from_priv(p) for p in privs]
    honest = []
    for i, n in enumerate(LENGTHS):
        for j in range(2):
            k = (2 * i + j) % len(privs)
            m = rng.randbytes(n)
            sig = S.sign(privs[k], m, seed=bytes([j]))
            honest.append((pks[k], m, sig))
            add("honest", pks[k], m, sig)
    for pk, m, sig in honest:
        for cat, lo in (("flip_r", 0), ("flip_s", 32)):
            s2 = bytearray(sig)
            s2[lo + rng.randrange(32)] ^= 1 << rng.randrange(8)
            add(cat, pk, m, s2)
        if m:
            m2 = bytearray(m)
            m2[rng.randrange(len(m))] ^= 1 << rng.randrange(8)
            add("flip_msg", pk, m2, sig)
        p2 = bytearray(pk)
        p2[1 + rng.randrange(32)] ^= 1 << rng.randrange(8)
        add("flip_pkx", pk=p2, msg=m, sig=sig)
    for pk, m, sig in honest[:8]:
        r, s = sig[:32], int.from_bytes(sig[32:], "big")
        add("high_s", pk, m, r + b32(S.N - s))
        add("r_zero", pk, m, bytes(32) + sig[32:])
        add("s_zero", pk, m, r + bytes(32))
        add("r_is_n", pk, m, b32(S.N) + sig[32:])
        add("s_is_n", pk, m, r + b32(S.N))
        add("r_max", pk, m, b"\xff" * 32 + sig[32:])
        add("s_max", pk, m, r + b"\xff" * 32)

    # valid signatures by key recovery from a chosen nonce point R
    x = 1
    for i in range(6):
        x, rpoint = on_curve_from(x)
        r, s = x, 3 + 2 * i
        m = rng.randbytes(LENGTHS[i % len(LENGTHS)] + 7)
        pk = S.encode_point(S.recover_key(rpoint, r, s, m))
        assert r + S.N < 2**256 and s + S.N < 2**256
        add("reduce_quirk", pk, m, b32(r + S.N) + b32(s + S.N))
        add("reduce_quirk", pk, m, b32(r + S.N) + b32(s))
        add("reduce_quirk", pk, m, b32(r) + b32(s + S.N))
        x += 1
    x = S.N + 1  # r = x - n must not be 0
    for i in range(6):
        x, rpoint = on_curve_from(x)
        assert S.N <= x < S.P
        r, s = x - S.N, rng.randrange(1, S.HALF_N)
        m = rng.randbytes(20 + i)
        pk = S.encode_point(S.recover_key(rpoint, r, s, m))
        add("x_ge_n", pk, m, b32(r) + b32(s))
        add("x_ge_n", pk, m, b32(x) + b32(s))  # r's bytes = r + n: reduced to r
        add("x_ge_n_twin", pk, m, b32(r + 1 + i) + b32(s))
        x += 1

    # keys
    for j, (pk, m, sig) in enumerate(honest[:6]):
        for prefix in (0x00, 0x04, 0x05):
            add("key_prefix", bytes([prefix]) + pk[1:], m, sig)
        add("key_x_ge_p", bytes([2 + (j & 1)]) + b32(S.P + (j & 1)), m, sig)
        add("key_x_ge_p", bytes([3 - (j & 1)]) + b32(S.P + 1), m, sig)
        xo = int.from_bytes(pk[1:], "big")
        while S.lift_x(xo, 0) is not None:
            xo += 1
        add("key_off_curve", pk[:1] + b32(xo), m, sig)
        add("key_parity", bytes([pk[0] ^ 1]) + pk[1:], m, sig)

    for d in EXCEPTIONAL_D:
        priv = b32(d)
        pk = S.pubkey_from_priv(priv)
        for i in range(64):
            m = b"exceptional %d " % i + rng.randbytes(i % 24)
            add("exceptional", pk, m, S.sign(priv, m))

    # [u1]G + [u2]Q = infinity: the signer picks r and the message and takes the
    # private key d = -e / r, so u1 + u2 d = (e + r d) / s = 0 for any s
    irng = random.Random(SEED + 1)  # its own stream: the vectors above stay what they were
    inf_r = [1, 5, S.P - S.N - 1, S.P - S.N, S.N - 1, S.N + 5] + [irng.randrange(1, S.N) for _ in range(6)]
    inf_s = [S.HALF_N, S.HALF_N - 1, 1]
    parities = set()
    for i, r in enumerate(inf_r):
        m = b"infinity %d " % i + irng.randbytes(LENGTHS[i % len(LENGTHS)])
        d = -S.msg_scalar(m) * pow(r % S.N, S.N - 2, S.N) % S.N
        pk = S.pubkey_from_priv(b32(d))
        parities.add(pk[0])
        s = inf_s[i] if i < len(inf_s) else irng.randrange(1, S.HALF_N)
        add("infinity", pk, m, b32(r) + b32(s))
    assert parities == {2, 3} and any(r + S.N < S.P for r in inf_r)

    rng.shuffle(vecs)
    for v in vecs:
        v["valid"] = int(S.verify(bytes.fromhex(v["pk"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"])))
        assert v["valid"] == (v["cat"] in VALID_CATS), v
        assert v["cat"] in VALID_CATS | INVALID_CATS
        if v["cat"] == "infinity":  # discriminating: only the Z != 0 test rejects it
            assert S.verify_without_z_test(bytes.fromhex(v["pk"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"])), v
    assert len(vecs) % 64 != 0  # the GPU tests' last bitmap word stays ragged
    summary = {}
    for v in vecs:
        s = summary.setdefault(v["cat"], {"n": 0, "valid": 0})
        s["n"] += 1
        s["valid"] += v["valid"]
    return {"generator": "tests/golden/make_secp256k1_corpus.py (tests/secp256k1_ref.py)", "seed": SEED,
            "summary": summary, "vectors": vecs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "secp256k1_corpus.json"))
    args = ap.parse_args()
    doc = build()
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=0)
    print(json.dumps(doc["summary"]))


if __name__ == "__main__":
    main()
