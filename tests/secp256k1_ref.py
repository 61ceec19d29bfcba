"""Python-integer restatement of secp256k1.PubKey.VerifySignature
(crypto/secp256k1/secp256k1.go:192-217 of the reference; btcec v2.2.1 /
dcrd secp256k1 underneath). Test infrastructure: the oracle of the secp256k1
corpus and of the GPU parity tests.

Verdict for a 33-byte key pk, a 64-byte signature sig, a message msg:
  1. pk[0] in {2, 3}; x = pk[1:33] big-endian, x < p (not reduced);
     y^2 = x^3 + 7 a square; y of parity pk[0] & 1 -> Q
  2. r = sig[0:32] mod n, s = sig[32:64] mod n (bytes >= n are reduced);
     reject r = 0, s = 0, s > (n - 1) / 2
  3. e = SHA-256(msg) mod n
  4. w = 1/s; X = [e w]G + [r w]Q; reject infinity; accept iff X.x mod n = r

Points are Jacobian (X, Y, Z), x = X/Z^2, y = Y/Z^3; None is infinity.
"""
from __future__ import annotations

import hashlib

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
GX = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
GY = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8
HALF_N = (N - 1) // 2
# the endomorphism (x, y) -> (BETA x, y) = [LAMBDA](x, y)
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE

G = (GX, GY, 1)


def jdouble(p):
    if p is None:
        return None
    x, y, z = p
    if y == 0:
        return None
    a = x * x % P
    b = y * y % P
    c = b * b % P
    d = 2 * ((x + b) * (x + b) - a - c) % P
    e = 3 * a % P
    x3 = (e * e - 2 * d) % P
    return x3, (e * (d - x3) - 8 * c) % P, 2 * y * z % P


def jadd(p, q):
    if p is None:
        return q
    if q is None:
        return p
    x1, y1, z1 = p
    x2, y2, z2 = q
    z1z1 = z1 * z1 % P
    z2z2 = z2 * z2 % P
    u1 = x1 * z2z2 % P
    u2 = x2 * z1z1 % P
    s1 = y1 * z2 * z2z2 % P
    s2 = y2 * z1 * z1z1 % P
    if u1 == u2:
        return jdouble(p) if s1 == s2 else None
    h = (u2 - u1) % P
    r = (s2 - s1) % P
    h2 = h * h % P
    h3 = h * h2 % P
    v = u1 * h2 % P
    x3 = (r * r - h3 - 2 * v) % P
    return x3, (r * (v - x3) - s1 * h3) % P, h * z1 * z2 % P


def jneg(p):
    return None if p is None else (p[0], (-p[1]) % P, p[2])


def jmul(k, p):
    k %= N
    r = None
    for bit in bin(k)[2:] if k else "":
        r = jdouble(r)
        if bit == "1":
            r = jadd(r, p)
    return r


_G_POW2: list = []


def gmul(k):
    """[k]G over a cached table of [2^i]G: additions only."""
    if not _G_POW2:
        p = G
        for _ in range(256):
            x, y = to_affine(p)
            _G_POW2.append((x, y, 1))
            p = jdouble(p)
    k %= N
    r = None
    i = 0
    while k:
        if k & 1:
            r = jadd(r, _G_POW2[i])
        k >>= 1
        i += 1
    return r


def to_affine(p):
    if p is None:
        return None
    x, y, z = p
    zi = pow(z, P - 2, P)
    return x * zi * zi % P, y * zi * zi * zi % P


def lift_x(x, odd):
    """The curve point with this x and y parity, or None."""
    if x >= P:
        return None
    y2 = (x * x * x + 7) % P
    y = pow(y2, (P + 1) // 4, P)
    if y * y % P != y2:
        return None
    if (y & 1) != odd:
        y = P - y
    return x, y, 1


def parse_pubkey(pk: bytes):
    if len(pk) != 33 or pk[0] not in (2, 3):
        return None
    return lift_x(int.from_bytes(pk[1:], "big"), pk[0] & 1)


def encode_point(p) -> bytes:
    x, y = to_affine(p)
    return bytes([2 + (y & 1)]) + x.to_bytes(32, "big")


def pubkey_from_priv(priv: bytes) -> bytes:
    return encode_point(gmul(int.from_bytes(priv, "big")))


def msg_scalar(msg: bytes) -> int:
    return int.from_bytes(hashlib.sha256(msg).digest(), "big") % N


def verify(pk: bytes, msg: bytes, sig: bytes) -> bool:
    if len(sig) != 64:
        return False
    q = parse_pubkey(pk)
    if q is None:
        return False
    r = int.from_bytes(sig[:32], "big") % N
    s = int.from_bytes(sig[32:], "big") % N
    if r == 0 or s == 0 or s > HALF_N:
        return False
    w = pow(s, N - 2, N)
    x = jadd(gmul(msg_scalar(msg) * w % N), jmul(r * w % N, q))
    if x is None:
        return False
    return to_affine(x)[0] % N == r


def verify_without_z_test(pk: bytes, msg: bytes, sig: bytes) -> bool:
    """The verdict of a verifier that compares X = r Z on homogeneous
    coordinates without first rejecting Z = 0: the point at infinity (0 : 1 : 0)
    satisfies 0 = r * 0 for every r. Everything else is verify(). Used to show
    that the corpus's `infinity` vectors discriminate."""
    if len(sig) != 64:
        return False
    q = parse_pubkey(pk)
    if q is None:
        return False
    r = int.from_bytes(sig[:32], "big") % N
    s = int.from_bytes(sig[32:], "big") % N
    if r == 0 or s == 0 or s > HALF_N:
        return False
    w = pow(s, N - 2, N)
    x = jadd(gmul(msg_scalar(msg) * w % N), jmul(r * w % N, q))
    return x is None or to_affine(x)[0] % N == r


def sign(priv: bytes, msg: bytes, seed: bytes = b"") -> bytes:
    """A deterministic lower-S signature (the nonce is a hash of the key, the
    message, the seed and a counter; not RFC 6979, which the verdict does not
    depend on)."""
    d = int.from_bytes(priv, "big") % N
    e = msg_scalar(msg)
    ctr = 0
    while True:
        k = int.from_bytes(hashlib.sha512(b"secp256k1_ref.sign" + priv + seed + ctr.to_bytes(4, "big") + msg).digest(),
                           "big") % N
        ctr += 1
        if k == 0:
            continue
        r = to_affine(gmul(k))[0] % N
        s = pow(k, N - 2, N) * (e + r * d) % N
        if r == 0 or s == 0:
            continue
        if s > HALF_N:
            s = N - s
        return r.to_bytes(32, "big") + s.to_bytes(32, "big")


def recover_key(rpoint, r: int, s: int, msg: bytes):
    """Q = r^-1 (s R - e G): the key under which (r, s) verifies msg with the
    nonce point R (whose x is r, or r + n)."""
    ri = pow(r, N - 2, N)
    return jmul(ri, jadd(jmul(s, rpoint), jneg(gmul(msg_scalar(msg)))))
