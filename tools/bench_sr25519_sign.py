#!/usr/bin/env python3
"""Times the sr25519 test-data calls, cmtv_pubkeys_sr25519 (with addresses)
and cmtv_sign_sr25519, at 150, 10,000 and 262,144 signatures over 150 keys,
beside numbers from the same box: cmtv_verify_sr25519 of the batch just
signed (and, at the sizes where that is the quad form, a second context forced
to the one-signature-per-lane form, CMTV_FORM=lane: the like-for-like kernel),
one thread of the C oracle's oracle_sr25519_sign_batch, and
VerifyCommit of an all-sr25519 and of a 3,334 / 3,333 / 3,333 mixed validator
set at 10,000 validators, built with the device signers
(testutil.make_typed_validator_set / make_typed_commit). Needs a GPU; there is
no CPU fallback.

    python tools/bench_sr25519_sign.py [--sizes 150,10000,262144] [--reps 30,15,7] [--warmup 3]
                                       [--out profiles/sr25519_sign_bench.json]

The context is opened with CMTV_TIMING=1, so every call is timed by a HIP
event pair around its launches: per call the host clock (wall_ms: staging
copies, launches, the copy back, the wait) and cmtv_stats.device_ms
(device_ms: the kernels alone) are taken, and their medians after the warm-up
reported. Messages are 116 bytes (a vote's sign-bytes on a short chain id).
Every output is checked before timing: all signatures with the device
verifier, and a sample of keys, addresses and signatures against
oracle/sr25519_ref.py (bytes, and its verify()).
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MSG_LEN = 116
N_KEYS = 150


def timed(ctx, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    wall, dev = [], []
    for _ in range(reps):
        d0 = ctx.stats()["device_ms"]
        t = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t) * 1e3)
        dev.append(ctx.stats()["device_ms"] - d0)
    return {"wall_ms": round(float(np.median(wall)), 4), "device_ms": round(float(np.median(dev)), 4)}


def commit_row(ctx, TU, counts, reps, warmup):
    """verify_commit of one synthetic commit of a set with these (ed25519, secp256k1, sr25519) counts."""
    sv = TU.make_typed_validator_set(ctx, n_ed25519=counts[0], n_secp256k1=counts[1], n_sr25519=counts[2])
    height = 7
    t = time.perf_counter()
    commit, _, _ = TU.make_typed_commit(ctx, sv, height)
    build_ms = (time.perf_counter() - t) * 1e3
    bid = TU.block_id_for_height(height)
    row = {"validators": dict(zip(("ed25519", "secp256k1", "sr25519"), counts)), "make_commit_wall_ms": round(build_ms, 2)}
    row["verify_commit"] = timed(ctx, lambda: sv.valset.verify_commit(TU.CHAIN_ID, bid, height, commit, ctx=ctx),
                                 reps, warmup)
    row["verify_commit_light"] = timed(
        ctx, lambda: sv.valset.verify_commit_light(TU.CHAIN_ID, bid, height, commit, ctx=ctx), reps, warmup)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="150,10000,262144")
    ap.add_argument("--reps", default="30,15,7")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sr25519_sign_bench.json"))
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")]
    reps = [int(x) for x in a.reps.split(",")]

    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_sr25519_sign: needs a GPU")
    torch.cuda.init()
    from cometbft_amd import Context
    from cometbft_amd import testutil as TU
    from oracle import coracle
    from oracle import sr25519_ref as S

    os.environ["CMTV_TIMING"] = "1"
    ctx = Context(device=0)
    props = torch.cuda.get_device_properties(0)
    res = {"device": props.name, "arch": getattr(props, "gcnArchName", ""), "msg_len": MSG_LEN, "n_keys": N_KEYS,
           "warmup": a.warmup, "sizes": []}
    rng = np.random.default_rng(25519)
    mini = TU.sr25519_validator_minis(N_KEYS)
    pk, addr = ctx.pubkeys_sr25519(mini, with_addresses=True)
    for i in range(0, N_KEYS, 15):
        assert pk[i].tobytes() == S.pubkey_from_mini(mini[i].tobytes()), i
        assert addr[i].tobytes() == hashlib.sha256(pk[i].tobytes()).digest()[:20], i
    small = []
    for n, rep in zip(sizes, reps):
        msg = rng.integers(0, 256, n * MSG_LEN + 1, dtype=np.uint8)
        off = (np.arange(n + 1, dtype=np.uint64) * MSG_LEN).astype(np.uint32)
        idx = (np.arange(n, dtype=np.uint32) % N_KEYS) if n <= N_KEYS else rng.integers(0, N_KEYS, n, dtype=np.uint32)
        many = TU.sr25519_validator_minis(min(n, 10000))  # the key call at the batch's size (distinct keys)

        sig = ctx.sign_sr25519(mini, msg, off, idx)
        assert ctx.verify_sr25519(pk[idx], sig, msg, off).all()
        for i in range(0, n, max(1, n // 8)):
            m = msg[i * MSG_LEN:(i + 1) * MSG_LEN].tobytes()
            assert sig[i].tobytes() == S.sign(mini[idx[i]].tobytes(), m), i
            assert S.verify(pk[idx[i]].tobytes(), m, sig[i].tobytes()), i

        row = {"n": n, "reps": rep, "pubkeys_n": int(many.shape[0]),
               "pubkeys_sr25519": timed(ctx, lambda: ctx.pubkeys_sr25519(many, with_addresses=True), rep, a.warmup),
               "sign_sr25519": timed(ctx, lambda: ctx.sign_sr25519(mini, msg, off, idx), rep, a.warmup),
               "verify_sr25519": timed(ctx, lambda: ctx.verify_sr25519(pk[idx], sig, msg, off), rep, a.warmup)}
        row["sign_over_verify_device"] = round(row["sign_sr25519"]["device_ms"] /
                                               max(row["verify_sr25519"]["device_ms"], 1e-9), 4)
        row["sign_us_per_signature"] = round(row["sign_sr25519"]["wall_ms"] * 1e3 / n, 4)
        # one thread of the C oracle on (a slice of) the same batch
        k = min(n, 2000)
        t = time.perf_counter()
        exp = coracle.sr25519_sign_batch(mini, msg[:k * MSG_LEN + 1], off[:k + 1], idx[:k])
        row["oracle_sign_us_per_signature"] = round((time.perf_counter() - t) * 1e6 / k, 2)
        assert np.array_equal(exp, sig[:k])
        res["sizes"].append(row)
        print(json.dumps(row), flush=True)
        if n < 49152:  # below it the verifier is the quad form: keep the batch for the lane form
            small.append((row, rep, pk[idx], sig, msg, off))

    # like for like at the small sizes: the verifier forced to its one-signature-per-lane kernel
    os.environ["CMTV_FORM"] = "lane"
    lane = Context(device=0)
    del os.environ["CMTV_FORM"]
    for row, rep, pks, sig, msg, off in small:
        assert lane.verify_sr25519(pks, sig, msg, off).all()
        row["verify_sr25519_lane"] = timed(lane, lambda: lane.verify_sr25519(pks, sig, msg, off), rep, a.warmup)
        row["sign_over_verify_lane_device"] = round(row["sign_sr25519"]["device_ms"] /
                                                    max(row["verify_sr25519_lane"]["device_ms"], 1e-9), 4)
        print(json.dumps({"n": row["n"], "verify_sr25519_lane": row["verify_sr25519_lane"],
                          "sign_over_verify_lane_device": row["sign_over_verify_lane_device"]}), flush=True)
    lane.close()

    res["commits"] = []
    for counts in ((0, 0, 10000), (3334, 3333, 3333)):
        row = commit_row(ctx, TU, counts, 15, a.warmup)
        res["commits"].append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
