#!/usr/bin/env python3
"""VerifyCommit of an all-secp256k1 validator set through
cmtv_verify_commit_typed, against what a caller had to compose before it
existed: cmtv_vote_sign_bytes per signature, the messages packed, and
cmtv_verify_secp256k1 (key bytes) or cmtv_verify_secp256k1_indexed
(registered keys) over them. Needs a GPU; there is no CPU fallback.

    python tools/bench_typed_commit.py [--sizes 150,10000] [--reps 200,40] [--warmup 10] [--real-keys]

Per size, four timed calls alternate in one loop, each a host clock around
a call that returns after its verdicts are back:
  typed_nocache   cmtv_verify_commit_typed, cmtv_keyset_cache off (key bytes)
  typed_cache     the same on a context with the cache on (registered keys;
                  the set is registered by the warm-up)
  parent_generic  cmtv_verify_secp256k1 on messages packed beforehand
  parent_keyed    cmtv_verify_secp256k1_indexed on the same
The composition's sign-bytes (parent_signbytes: n cmtv_vote_sign_bytes calls
and the packing) are timed apart, because through this binding each call
costs microseconds of Python a cgo caller would not pay; its replay of the
reference loop is left out altogether. Both favour the composition. Medians
are reported, and typed / parent ratios both without and with the sign-bytes.

Verdicts are checked before and after the timed loop: the typed calls must
return CMTV_OK on the good commit and "wrong signature (#i)" at the flipped
index of a bad one, the composed calls all-valid and exactly that index
invalid, and a sample of signatures is verified with tests/secp256k1_ref.py.
The keys are consecutive multiples of G and every signature uses one nonce
(valid ECDSA, cheap to make: the verifier's work does not depend on either).
--real-keys takes the set and the signatures from the device signer instead
(testutil.make_secp256k1_validator_set: derived keys in address order, RFC 6979
nonces); the default stays the cheap construction so recorded numbers remain
comparable.
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CHAIN = "cmtverify-bench"
HEIGHT = 1000


def make_set(n):
    """n keys d0 + i, their public keys by repeated addition of G."""
    import secp256k1_ref as S

    d0 = int.from_bytes(hashlib.sha256(b"bench-typed-commit").digest(), "big") % S.N
    p = S.gmul(d0)
    privs, pks = [], []
    for i in range(n):
        privs.append((d0 + i) % S.N)
        pks.append(S.encode_point(p))
        p = S.jadd(p, S.G)
    return privs, pks


def sign_all(privs, msgs):
    """ECDSA with one nonce for every signature: r is fixed, s is arithmetic mod n."""
    import secp256k1_ref as S

    k = int.from_bytes(hashlib.sha256(b"bench-typed-commit/nonce").digest(), "big") % S.N
    r = S.to_affine(S.gmul(k))[0] % S.N
    ki = pow(k, S.N - 2, S.N)
    out = []
    for d, m in zip(privs, msgs):
        s = ki * (S.msg_scalar(m) + r * d) % S.N
        if s > S.HALF_N:
            s = S.N - s
        out.append(r.to_bytes(32, "big") + s.to_bytes(32, "big"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="150,10000")
    ap.add_argument("--reps", default="200,40")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--real-keys", action="store_true", help="derived keys and RFC 6979 nonces from the device signer")
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",")]
    reps = [int(x) for x in args.reps.split(",")]

    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_typed_commit: needs a GPU")
    torch.cuda.init()
    import secp256k1_ref as S
    from cometbft_amd import Context, pack_messages
    from cometbft_amd import _native as N
    from cometbft_amd import testutil as TU
    from cometbft_amd import types as T

    lib = N.lib()
    u8p = ctypes.POINTER(ctypes.c_uint8)
    ctx_off, ctx_on = Context(device=0), Context(device=0)
    ctx_on.keyset_cache(2)
    for n, rep in zip(sizes, reps):
        if args.real_keys:
            sv = TU.make_secp256k1_validator_set(ctx_off, n)
            vals = sv.valset
            pks = [v.pub_key for v in vals.validators]
        else:
            privs, pks = make_set(n)
            vals = T.ValidatorSet([T.Validator(pk, 10, 0, "secp256k1") for pk in pks])
        bid = TU.block_id_for_height(HEIGHT)
        stamps = [TU.timestamp(HEIGHT, i) for i in range(n)]

        def encode_all():
            cb, keep = bid._c()
            buf = (ctypes.c_uint8 * 512)()
            cid = CHAIN.encode()
            out = []
            for sec, nanos in stamps:
                k = lib.cmtv_vote_sign_bytes(cid, len(cid), T.PRECOMMIT_TYPE, HEIGHT, 0, ctypes.byref(cb), sec, nanos,
                                             buf, 512)
                out.append(bytes(buf[:k]))
            return pack_messages(out), out

        (m, off), msgs = encode_all()
        sigs = [bytes(x) for x in ctx_off.sign_secp256k1(sv.secrets, m, off)] if args.real_keys else \
            sign_all(privs, msgs)
        for i in range(0, n, max(1, n // 50)):  # a sample against the reference verifier
            assert S.verify(pks[i], msgs[i], sigs[i]), i
        bad_at = n - 3 if n > 3 else 0
        bad = bytearray(sigs[bad_at])
        bad[40] ^= 1

        def commit_of(sig_list):
            return T.Commit(HEIGHT, 0, bid, [T.CommitSig(T.BLOCK_ID_FLAG_COMMIT, vals.validators[i].address,
                                                         stamps[i], sig_list[i]) for i in range(n)])

        vs, keep_v = vals._pack()
        kt = keep_v[5].ctypes.data_as(u8p)
        cb, keep_b = bid._c()
        cm_good, keep_g = T._pack_commit(commit_of(sigs))
        cm_bad, keep_x = T._pack_commit(commit_of(sigs[:bad_at] + [bytes(bad)] + sigs[bad_at + 1:]))
        res = N.cmtv_commit_result()
        buf = ctypes.create_string_buffer(1024)
        cid = CHAIN.encode()

        def typed(ctx, cm):
            return lib.cmtv_verify_commit_typed(ctx.handle, N.VERIFY_COMMIT, 0, cid, len(cid), ctypes.byref(vs), kt,
                                                ctypes.byref(cb), HEIGHT, ctypes.byref(cm), 0, 0, ctypes.byref(res),
                                                buf, len(buf))

        pk_arr = np.frombuffer(b"".join(pks), np.uint8).copy()
        sig_good = np.frombuffer(b"".join(sigs), np.uint8).copy()
        sig_bad = sig_good.copy()
        sig_bad[64 * bad_at + 40] ^= 1
        kidx = np.arange(n, dtype=np.uint32)
        keys = ctx_off.register_secp256k1_keys(pk_arr.reshape(n, 33))
        out_valid = np.zeros(n, np.uint8)
        p8 = lambda a: a.ctypes.data_as(u8p)  # noqa: E731
        p32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))  # noqa: E731

        def parent_generic(sg):
            return lib.cmtv_verify_secp256k1(ctx_off.handle, n, p8(pk_arr), p8(sg), p8(m), p32(off), p8(out_valid),
                                             None)

        def parent_keyed(sg):
            return lib.cmtv_verify_secp256k1_indexed(ctx_off.handle, keys._h, n, p32(kidx), p8(sg), p8(m), p32(off),
                                                     p8(out_valid), None)

        def check():
            for ctx in (ctx_off, ctx_on):
                assert typed(ctx, cm_good) == N.CMTV_OK, buf.value
                assert typed(ctx, cm_bad) == N.CMTV_ECOMMIT and res.sig_index == bad_at, (res.sig_index, buf.value)
            for call in (parent_generic, parent_keyed):
                assert call(sig_good) == N.CMTV_OK and out_valid.all()
                assert call(sig_bad) == N.CMTV_OK and list(np.nonzero(out_valid == 0)[0]) == [bad_at]

        check()  # also registers the set on ctx_on and builds the fixed table
        sides = {"typed_nocache": lambda: typed(ctx_off, cm_good), "typed_cache": lambda: typed(ctx_on, cm_good),
                 "parent_generic": lambda: parent_generic(sig_good), "parent_keyed": lambda: parent_keyed(sig_good)}
        for _ in range(args.warmup):
            for f in sides.values():
                f()
        times = {k: [] for k in sides}
        for _ in range(rep):
            for k, f in sides.items():
                t = time.perf_counter()
                f()
                times[k].append(time.perf_counter() - t)
        sb = []
        for _ in range(max(3, rep // 10)):
            t = time.perf_counter()
            encode_all()
            sb.append(time.perf_counter() - t)
        check()
        keys.free()
        med = {k: float(np.median(v)) * 1e3 for k, v in times.items()}
        sb_ms = float(np.median(sb)) * 1e3
        print(json.dumps({
            "tool": "bench_typed_commit", "real_keys": args.real_keys, "n": n, "reps": rep, "msg_len": len(msgs[0]),
            **{k + "_ms": round(v, 4) for k, v in med.items()},
            **{k + "_p90_ms": round(float(np.percentile(times[k], 90)) * 1e3, 4) for k in times},
            "parent_signbytes_ms": round(sb_ms, 4),
            "nocache_over_parent": round(med["typed_nocache"] / med["parent_generic"], 4),
            "cache_over_parent": round(med["typed_cache"] / med["parent_keyed"], 4),
            "nocache_over_parent_with_signbytes": round(med["typed_nocache"] / (med["parent_generic"] + sb_ms), 4),
            "cache_over_parent_with_signbytes": round(med["typed_cache"] / (med["parent_keyed"] + sb_ms), 4)}),
            flush=True)
    ctx_off.close()
    ctx_on.close()


if __name__ == "__main__":
    main()
