#!/usr/bin/env python3
"""Times the secp256k1 test-data calls, cmtv_pubkeys_secp256k1 (with
addresses) and cmtv_sign_secp256k1, at 150, 10,000 and 262,144 keys /
signatures, beside three numbers from the same box: the Ed25519 pair
(cmtv_pubkeys_ed25519 / cmtv_sign_ed25519) at the same sizes, the Python
signer tests/secp256k1_ref.sign per signature, and cmtv_verify_secp256k1 on
the 10,000 signatures just made. Needs a GPU; there is no CPU fallback.

    python tools/bench_secp256k1_sign.py [--sizes 150,10000,262144] [--reps 30,15,7] [--warmup 3]
                                         [--out profiles/secp256k1_sign_bench.json]

The context is opened with CMTV_TIMING=1, so every call is timed by a HIP
event pair around its launches: per call the host clock (wall_ms: staging
copies, launches, the copy back, the wait) and cmtv_stats.device_ms
(device_ms: the kernels alone) are taken, and their medians after the warm-up
reported (the Ed25519 pair records no event pair: its device_ms is 0 and its
wall_ms the number to compare). Messages are 116 bytes (a vote's sign-bytes on a short chain id),
one key per signature. Every output is checked before timing: a sample of
keys, addresses and signatures against tests/secp256k1_sign_ref.py, and all
signatures with the device verifier.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MSG_LEN = 116


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="150,10000,262144")
    ap.add_argument("--reps", default="30,15,7")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "secp256k1_sign_bench.json"))
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")]
    reps = [int(x) for x in a.reps.split(",")]

    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_secp256k1_sign: needs a GPU")
    torch.cuda.init()
    import secp256k1_ref as S
    import secp256k1_sign_ref as R
    from cometbft_amd import Context
    from cometbft_amd import testutil as TU

    os.environ["CMTV_TIMING"] = "1"
    ctx = Context(device=0)
    props = torch.cuda.get_device_properties(0)
    res = {"device": props.name, "arch": getattr(props, "gcnArchName", ""), "msg_len": MSG_LEN, "warmup": a.warmup,
           "sizes": []}
    rng = np.random.default_rng(6979)
    for n, rep in zip(sizes, reps):
        priv = TU.secp256k1_validator_privkeys(n)
        seeds = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        msg = rng.integers(0, 256, n * MSG_LEN + 1, dtype=np.uint8)
        off = (np.arange(n + 1, dtype=np.uint64) * MSG_LEN).astype(np.uint32)

        pk, addr = ctx.pubkeys_secp256k1(priv, with_addresses=True)
        sig = ctx.sign_secp256k1(priv, msg, off)
        for i in range(0, n, max(1, n // 8)):
            p = priv[i].tobytes()
            assert pk[i].tobytes() == R.pubkey(p) and addr[i].tobytes() == R.address(R.pubkey(p)), i
            assert sig[i].tobytes() == R.sign(p, msg[i * MSG_LEN:(i + 1) * MSG_LEN].tobytes()), i
        assert ctx.verify_secp256k1(pk, sig, msg, off).all()

        row = {"n": n, "reps": rep,
               "pubkeys_secp256k1": timed(ctx, lambda: ctx.pubkeys_secp256k1(priv, with_addresses=True), rep, a.warmup),
               "sign_secp256k1": timed(ctx, lambda: ctx.sign_secp256k1(priv, msg, off), rep, a.warmup),
               "pubkeys_ed25519": timed(ctx, lambda: ctx.pubkeys(seeds), rep, a.warmup),
               "sign_ed25519": timed(ctx, lambda: ctx.sign(seeds, msg, off), rep, a.warmup)}
        if n == 10000:
            row["verify_secp256k1"] = timed(ctx, lambda: ctx.verify_secp256k1(pk, sig, msg, off), rep, a.warmup)
            row["sign_over_verify_device"] = round(row["sign_secp256k1"]["device_ms"] /
                                                   row["verify_secp256k1"]["device_ms"], 4)
        row["sign_us_per_signature"] = round(row["sign_secp256k1"]["wall_ms"] * 1e3 / n, 4)
        res["sizes"].append(row)
        print(json.dumps(row), flush=True)

    k = 20
    t = time.perf_counter()
    for i in range(k):
        S.sign((i + 1).to_bytes(32, "big"), b"bench_secp256k1_sign %d" % i)
    res["python_sign_ms_per_signature"] = round((time.perf_counter() - t) * 1e3 / k, 3)
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"written": a.out, "python_sign_ms_per_signature": res["python_sign_ms_per_signature"]}))


if __name__ == "__main__":
    main()
