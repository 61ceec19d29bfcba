"""Inputs shared by the sr25519 signing tests (host checker and GPU), and their
expected outputs from oracle/sr25519_ref.py, computed once per process.

Keys: the mini secrets 32 zero bytes and 32 bytes of 0xff, then
cometbft_amd.testutil.sr25519_validator_minis (every 32-byte string is a mini
secret: there are no edge values to hit, only the expanded scalars' digits).

Signatures: 257 over the first 40 keys by a shuffled index in which some keys
sign many times. The message lengths cycle through the places where something
changes: 54/55 and 182/183, where the witness hash (57-byte prefix) gains a
SHA-512 block; 71, which fills one exactly; 165..167 around the STROBE rate;
and the neighbours of each.
"""
from __future__ import annotations

import ctypes
import functools
import hashlib
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cometbft_amd.testutil import sr25519_validator_minis  # noqa: E402
from oracle import sr25519_ref as S  # noqa: E402

P, L = S.P, S.L
MSG_LENGTHS = [0, 1, 54, 55, 56, 70, 71, 72, 116, 161, 165, 166, 167, 182, 183, 300]
N_SIGN_KEYS = 40
N_SIGS = 257


@functools.lru_cache(maxsize=None)
def keys(n: int = 257) -> tuple:
    """n mini secrets as 32-byte strings: the two specials, then the synthetic validators'."""
    out = [bytes(32), b"\xff" * 32] + [m.tobytes() for m in sr25519_validator_minis(max(0, n - 2))]
    return tuple(out[:n])


def keys_array(n: int = 257) -> np.ndarray:
    return np.frombuffer(b"".join(keys(n)), np.uint8).reshape(n, 32).copy()


@functools.lru_cache(maxsize=None)
def expected_pubkeys(n: int = 257):
    """(pk n x 32, addr n x 20) by the restatement."""
    pks = [S.pubkey_from_mini(k) for k in keys(n)]
    pk = np.frombuffer(b"".join(pks), np.uint8).reshape(n, 32)
    addr = np.frombuffer(b"".join(hashlib.sha256(p).digest()[:20] for p in pks), np.uint8).reshape(n, 20)
    return pk, addr


@functools.lru_cache(maxsize=None)
def sign_inputs():
    """(key_idx, msgs): N_SIGS signatures over the first N_SIGN_KEYS keys."""
    rng = random.Random(25519)
    idx = list(range(N_SIGN_KEYS)) + [rng.randrange(N_SIGN_KEYS) for _ in range(N_SIGS - N_SIGN_KEYS - 60)] + \
        [7] * 30 + [N_SIGN_KEYS - 1] * 30
    rng.shuffle(idx)
    msgs = [rng.randbytes(MSG_LENGTHS[i % len(MSG_LENGTHS)]) for i in range(N_SIGS)]
    assert len(idx) == N_SIGS == len(msgs)
    return tuple(idx), tuple(msgs)


@functools.lru_cache(maxsize=None)
def expected_signatures():
    """sig N_SIGS x 64 by the restatement."""
    idx, msgs = sign_inputs()
    ks = keys(N_SIGN_KEYS)
    return np.frombuffer(b"".join(S.sign(ks[i], m) for i, m in zip(idx, msgs)), np.uint8).reshape(N_SIGS, 64)


@functools.lru_cache(maxsize=None)
def expected_signatures_in_order():
    """Signature i of message i by key i, i < N_SIGN_KEYS (a call without key indices)."""
    _, msgs = sign_inputs()
    ks = keys(N_SIGN_KEYS)
    return np.frombuffer(b"".join(S.sign(ks[i], msgs[i]) for i in range(N_SIGN_KEYS)), np.uint8).reshape(-1, 64)


def witness(nonce: bytes, msg: bytes) -> int:
    """The deterministic witness of oracle/sr25519_ref.sign()."""
    return int.from_bytes(hashlib.sha512(b"cmtverify/sr25519-witness" + nonce + msg).digest(), "little") % L


def encode_branches(p):
    """(rotate, negate y, take the absolute value) as RFC 9496 4.3.2 ENCODE
    decides them for the extended point p: oracle/sr25519_ref.ristretto_encode
    with its three conditions reported."""
    x0, y0, z0, t0 = p
    u1 = (z0 + y0) * (z0 - y0) % P
    u2 = x0 * y0 % P
    _, invsqrt = S.sqrt_ratio_m1(1, u1 * u2 % P * u2 % P)
    den1, den2 = invsqrt * u1 % P, invsqrt * u2 % P
    z_inv = den1 * den2 % P * t0 % P
    rotate = S._is_neg(t0 * z_inv)
    if rotate:
        x, y, den_inv = y0 * S.SQRT_M1 % P, x0 * S.SQRT_M1 % P, den1 * S.INVSQRT_A_MINUS_D % P
    else:
        x, y, den_inv = x0, y0, den2
    negate = S._is_neg(x * z_inv)
    if negate:
        y = (-y) % P
    return rotate, negate, S._is_neg(den_inv * (z0 - y))


# ---------------------------------------------------------------- refused calls
CANARY = 0xA5
u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)


def p8(a):
    return a.ctypes.data_as(u8p)


def p32(a):
    return a.ctypes.data_as(u32p)


def refused_calls(ctx):
    """Every call the header says is CMTV_EINVAL, as (name, thunk, outputs):
    run with ctx = None here and with a live context on the GPU."""
    from cometbft_amd import _native as N

    lib = N.lib()
    n = 4
    mini = keys_array(n).reshape(-1)
    pk = np.full(32 * n, CANARY, np.uint8)
    addr = np.full(20 * n, CANARY, np.uint8)
    sig = np.full(64 * n, CANARY, np.uint8)
    msg = np.arange(64, dtype=np.uint8)
    off = np.array([0, 10, 10, 40, 64], np.uint32)
    idx = np.array([3, 0, 0, 2], np.uint32)
    outs = (pk, addr, sig)
    cases = [
        ("pub null mini", lambda: lib.cmtv_pubkeys_sr25519(ctx, n, None, p8(pk), p8(addr))),
        ("pub null out", lambda: lib.cmtv_pubkeys_sr25519(ctx, n, p8(mini), None, p8(addr))),
        ("pub n > 2^31", lambda: lib.cmtv_pubkeys_sr25519(ctx, 2**31 + 1, p8(mini), p8(pk), p8(addr))),
        ("sign null mini", lambda: lib.cmtv_sign_sr25519(ctx, n, None, n, p32(idx), p8(msg), p32(off), p8(sig))),
        ("sign null off", lambda: lib.cmtv_sign_sr25519(ctx, n, p8(mini), n, p32(idx), p8(msg), None, p8(sig))),
        ("sign null out", lambda: lib.cmtv_sign_sr25519(ctx, n, p8(mini), n, p32(idx), p8(msg), p32(off), None)),
        ("sign null msg", lambda: lib.cmtv_sign_sr25519(ctx, n, p8(mini), n, p32(idx), None, p32(off), p8(sig))),
        ("sign n > 2^31", lambda: lib.cmtv_sign_sr25519(ctx, n, p8(mini), 2**31 + 1, p32(idx), p8(msg), p32(off),
                                                       p8(sig))),
        ("sign no idx, n != n_keys", lambda: lib.cmtv_sign_sr25519(ctx, n, p8(mini), n - 1, None, p8(msg), p32(off),
                                                                  p8(sig))),
    ]
    bad_off = off.copy()
    bad_off[2] = 9
    cases.append(("sign decreasing off", lambda: lib.cmtv_sign_sr25519(ctx, n, p8(mini), n, p32(idx), p8(msg),
                                                                      p32(bad_off), p8(sig))))
    for j in (0, n - 1):
        bad_idx = idx.copy()
        bad_idx[j] = n
        cases.append((f"sign idx[{j}] = n_keys", lambda b=bad_idx: lib.cmtv_sign_sr25519(
            ctx, n, p8(mini), n, p32(b), p8(msg), p32(off), p8(sig))))
    return cases, outs


def assert_refused(ctx):
    from cometbft_amd import _native as N

    cases, outs = refused_calls(ctx)
    for name, call in cases:
        assert call() == N.CMTV_EINVAL, name
        for o in outs:
            assert (o == CANARY).all(), name
