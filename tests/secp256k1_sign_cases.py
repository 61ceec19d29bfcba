"""Inputs shared by the secp256k1 signing tests (host checker and GPU), and
their expected outputs from tests/secp256k1_sign_ref.py, computed once per
process.

Keys: the specials first -- 1, 2, n-1, n-2, (n-1)/2, 2^255, the reference's
known-answer key, 32 bytes of 0x80, of 0x7f, and 0x00 / 0xff alternating, which
between them drive every signed-digit and carry case of the radix-256 comb --
then keys from a fixed seed.

Signatures: 257 over the first 40 keys by a shuffled index in which some keys
sign many times; signature 0 is the pinned "Satoshi Nakamoto" vector (key 1),
the others cycle through message lengths at every SHA-256 padding boundary a
vote can meet, and one long message.
"""
from __future__ import annotations

import ctypes
import functools
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import secp256k1_sign_ref as R  # noqa: E402

N = N_ORDER = R.N
with open(os.path.join(ROOT, "tests", "golden", "secp256k1_sign_kat.json")) as _f:
    KAT = json.load(_f)

SPECIAL_KEYS = [1, 2, N - 1, N - 2, (N - 1) // 2, 2**255, int(KAT["key"]["priv"], 16), int("80" * 32, 16),
                int("7f" * 32, 16), int("00ff" * 16, 16)]
MSG_LENGTHS = [0, 1, 54, 55, 56, 63, 64, 65, 118, 119, 120, 128, 161, 300]
N_SIGN_KEYS = 40
N_SIGS = 257


@functools.lru_cache(maxsize=None)
def keys(n: int = 257) -> tuple:
    """n private keys as 32-byte strings: the specials, then seeded ones."""
    rng = random.Random(6979)
    ds = SPECIAL_KEYS + [rng.randrange(1, N) for _ in range(max(0, n - len(SPECIAL_KEYS)))]
    return tuple(d.to_bytes(32, "big") for d in ds[:n])


def keys_array(n: int = 257) -> np.ndarray:
    return np.frombuffer(b"".join(keys(n)), np.uint8).reshape(n, 32).copy()


@functools.lru_cache(maxsize=None)
def expected_pubkeys(n: int = 257):
    """(pk n x 33, addr n x 20) by the restatement."""
    pks = [R.pubkey(k) for k in keys(n)]
    pk = np.frombuffer(b"".join(pks), np.uint8).reshape(n, 33)
    addr = np.frombuffer(b"".join(R.address(p) for p in pks), np.uint8).reshape(n, 20)
    return pk, addr


@functools.lru_cache(maxsize=None)
def sign_inputs():
    """(key_idx, msgs): N_SIGS signatures over the first N_SIGN_KEYS keys."""
    rng = random.Random(3279)
    idx = list(range(N_SIGN_KEYS)) + [rng.randrange(N_SIGN_KEYS) for _ in range(N_SIGS - N_SIGN_KEYS - 60)] + \
        [7] * 30 + [N_SIGN_KEYS - 1] * 30
    rng.shuffle(idx)
    idx[0] = 0
    msgs = [KAT["signature"]["msg"].encode()] + \
        [rng.randbytes(MSG_LENGTHS[i % len(MSG_LENGTHS)]) for i in range(N_SIGS - 1)]
    assert len(idx) == N_SIGS == len(msgs)
    return tuple(idx), tuple(msgs)


@functools.lru_cache(maxsize=None)
def expected_signatures():
    """(sig N_SIGS x 64, how many took the low-S negation) by the restatement."""
    idx, msgs = sign_inputs()
    ks = keys(N_SIGN_KEYS)
    out = [R.sign_detail(ks[i], m) for i, m in zip(idx, msgs)]
    sig = np.frombuffer(b"".join(o[0] for o in out), np.uint8).reshape(N_SIGS, 64)
    return sig, sum(1 for o in out if o[2])


@functools.lru_cache(maxsize=None)
def expected_signatures_in_order():
    """Signature i of message i by key i, i < N_SIGN_KEYS (a call without key indices)."""
    _, msgs = sign_inputs()
    ks = keys(N_SIGN_KEYS)
    return np.frombuffer(b"".join(R.sign(ks[i], msgs[i]) for i in range(N_SIGN_KEYS)), np.uint8).reshape(-1, 64)


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
    priv = np.frombuffer(b"".join((i + 1).to_bytes(32, "big") for i in range(n)), np.uint8).copy()
    pk = np.full(33 * n, CANARY, np.uint8)
    addr = np.full(20 * n, CANARY, np.uint8)
    sig = np.full(64 * n, CANARY, np.uint8)
    msg = np.arange(64, dtype=np.uint8)
    off = np.array([0, 10, 10, 40, 64], np.uint32)
    idx = np.array([3, 0, 0, 2], np.uint32)
    outs = (pk, addr, sig)

    def with_key(i, value):
        bad = priv.copy()
        bad[32 * i: 32 * i + 32] = np.frombuffer(value.to_bytes(32, "big"), np.uint8)
        return bad

    cases = [
        ("pub null priv", lambda: lib.cmtv_pubkeys_secp256k1(ctx, n, None, p8(pk), p8(addr))),
        ("pub null out", lambda: lib.cmtv_pubkeys_secp256k1(ctx, n, p8(priv), None, p8(addr))),
        ("pub n > 2^31", lambda: lib.cmtv_pubkeys_secp256k1(ctx, 2**31 + 1, p8(priv), p8(pk), p8(addr))),
        ("sign null priv", lambda: lib.cmtv_sign_secp256k1(ctx, n, None, n, p32(idx), p8(msg), p32(off), p8(sig))),
        ("sign null off", lambda: lib.cmtv_sign_secp256k1(ctx, n, p8(priv), n, p32(idx), p8(msg), None, p8(sig))),
        ("sign null out", lambda: lib.cmtv_sign_secp256k1(ctx, n, p8(priv), n, p32(idx), p8(msg), p32(off), None)),
        ("sign null msg", lambda: lib.cmtv_sign_secp256k1(ctx, n, p8(priv), n, p32(idx), None, p32(off), p8(sig))),
        ("sign n > 2^31", lambda: lib.cmtv_sign_secp256k1(ctx, n, p8(priv), 2**31 + 1, p32(idx), p8(msg), p32(off),
                                                         p8(sig))),
        ("sign no idx, n != n_keys", lambda: lib.cmtv_sign_secp256k1(ctx, n, p8(priv), n - 1, None, p8(msg), p32(off),
                                                                    p8(sig))),
    ]
    bad_off = off.copy()
    bad_off[2] = 9
    cases.append(("sign decreasing off", lambda: lib.cmtv_sign_secp256k1(ctx, n, p8(priv), n, p32(idx), p8(msg),
                                                                        p32(bad_off), p8(sig))))
    for j in (0, n - 1):
        bad_idx = idx.copy()
        bad_idx[j] = n
        cases.append((f"sign idx[{j}] = n_keys", lambda b=bad_idx: lib.cmtv_sign_secp256k1(
            ctx, n, p8(priv), n, p32(b), p8(msg), p32(off), p8(sig))))
    for i in (0, n - 1):
        for value in (0, N_ORDER, N_ORDER + 1, 2**256 - 1):
            bad = with_key(i, value)
            cases.append((f"pub key[{i}] = {value:#x}", lambda b=bad: lib.cmtv_pubkeys_secp256k1(
                ctx, n, p8(b), p8(pk), p8(addr))))
            cases.append((f"sign key[{i}] = {value:#x}", lambda b=bad: lib.cmtv_sign_secp256k1(
                ctx, n, p8(b), n, p32(idx), p8(msg), p32(off), p8(sig))))
    # a key no signature uses is checked too
    unused = with_key(1, 0)
    cases.append(("sign unused key 0", lambda: lib.cmtv_sign_secp256k1(ctx, n, p8(unused), n, p32(idx), p8(msg),
                                                                      p32(off), p8(sig))))
    return cases, outs


def assert_refused(ctx):
    from cometbft_amd import _native as N

    cases, outs = refused_calls(ctx)
    for name, call in cases:
        assert call() == N.CMTV_EINVAL, name
        for o in outs:
            assert (o == CANARY).all(), name
