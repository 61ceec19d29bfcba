"""Restatement of the secp256k1 key derivation and signing contract
(include/cmtverify.h cmtv_privkey_secp256k1_from_secret, cmtv_pubkeys_secp256k1,
cmtv_sign_secp256k1; the reference's crypto/secp256k1/secp256k1.go:45-138),
from RFC 6979 section 3.2 with hashlib, hmac and secp256k1_ref's curve
arithmetic. Test infrastructure: the oracle of the host and GPU signing tests.

  private key  32 bytes big-endian, d in [1, n - 1]
  from secret  d = (SHA-256(secret) mod (n - 1)) + 1
  public key   0x02 | (y & 1), x big-endian: 33 bytes
  address      RIPEMD-160(SHA-256(public key))
  signature    r || s, 32 bytes big-endian each; the nonce of RFC 6979 with
               HMAC-SHA-256 and no extra data; s in the lower half

btcec's own bytes (what the reference signs with) are not in the tree and
there is no Go toolchain: parity with them is by this restatement only.
"""
from __future__ import annotations

import hashlib
import hmac
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import secp256k1_ref as S  # noqa: E402

from cometbft_amd.ripemd160 import ripemd160  # noqa: E402

N = S.N
HALF_N = S.HALF_N


def _hmac(key: bytes, data: bytes) -> bytes:
    return hmac.new(key, data, hashlib.sha256).digest()


def privkey_from_secret(secret: bytes) -> bytes:
    c = int.from_bytes(hashlib.sha256(secret).digest(), "big")
    return (c % (N - 1) + 1).to_bytes(32, "big")


def pubkey(priv: bytes) -> bytes:
    return S.pubkey_from_priv(priv)


def address(pk: bytes) -> bytes:
    return ripemd160(hashlib.sha256(pk).digest())


class Nonce:
    """RFC 6979 section 3.2, step by step: K and V after steps b-g, then
    next() per candidate."""

    def __init__(self, d: int, h1: bytes):
        x = d.to_bytes(32, "big")
        h = (int.from_bytes(h1, "big") % N).to_bytes(32, "big")  # bits2octets
        self.V = b"\x01" * 32
        self.K = b"\x00" * 32
        for tag in (b"\x00", b"\x01"):
            self.K = _hmac(self.K, self.V + tag + x + h)
            self.V = _hmac(self.K, self.V)

    def next(self, retry: bool = False) -> bytes:
        """The next candidate's 32 bytes; with retry, after the update that
        follows a rejected candidate."""
        if retry:
            self.K = _hmac(self.K, self.V + b"\x00")
            self.V = _hmac(self.K, self.V)
        self.V = _hmac(self.K, self.V)
        return self.V


def candidate_ok(v: bytes) -> bool:
    return 0 < int.from_bytes(v, "big") < N


def r_from_x(x: int) -> int:
    return x % N


def sign_with_nonce(d: int, e: int, k: int):
    """(r || s, took the low-S negation), or None when r = 0 or s = 0."""
    pt = S.to_affine(S.gmul(k))
    if pt is None:
        return None
    r = r_from_x(pt[0])
    s = pow(k % N, N - 2, N) * (e + r * d) % N
    if r == 0 or s == 0:
        return None
    neg = s > HALF_N
    if neg:
        s = N - s
    return r.to_bytes(32, "big") + s.to_bytes(32, "big"), neg


def sign_detail(priv: bytes, msg: bytes):
    """(signature, nonce k, took the low-S negation)"""
    d = int.from_bytes(priv, "big")
    assert 0 < d < N
    h1 = hashlib.sha256(msg).digest()
    e = int.from_bytes(h1, "big") % N
    g = Nonce(d, h1)
    retry = False
    while True:
        v = g.next(retry)
        retry = True
        if not candidate_ok(v):
            continue
        k = int.from_bytes(v, "big")
        got = sign_with_nonce(d, e, k)
        if got is not None:
            return got[0], k, got[1]


def sign(priv: bytes, msg: bytes) -> bytes:
    return sign_detail(priv, msg)[0]
