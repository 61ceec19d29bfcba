#!/usr/bin/env python3
"""Throughput of secp256k1 ECDSA batch verification on one GPU.

10,000 device-resident signatures over 116-byte messages and 150 keys (the
commit shape of the Ed25519 and sr25519 10k lines), verified through
cmtv_verify_secp256k1_device. The 10,000 entries are drawn with a fixed seed
from a pool of 200 (key, signature, message) triples, 5% of them with one
flipped bit, whose verdicts tests/secp256k1_ref.py computes once; the GPU's
verdicts are checked against them before and after the timed launches.
Needs a GPU; there is no CPU fallback.

    python tools/secp256k1_bench.py [--n 10000] [--launches 200] [--warmup 20]
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--msg-len", type=int, default=116)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("secp256k1_bench: needs a GPU")
    torch.cuda.init()
    import secp256k1_ref as S
    from cometbft_amd import Context, pack_messages

    rng = random.Random(10000)
    privs = [rng.randbytes(32) for _ in range(150)]
    pks = [S.pubkey_from_priv(p) for p in privs]
    pool = []
    for i in range(200):
        k = i % len(privs)
        m = rng.randbytes(args.msg_len)
        sig = bytearray(S.sign(privs[k], m))
        if i % 20 == 7:
            sig[rng.randrange(64)] ^= 1 << rng.randrange(8)
        pool.append((pks[k], bytes(sig), m, int(S.verify(pks[k], m, bytes(sig)))))
    idx = [rng.randrange(len(pool)) for _ in range(args.n)]
    pk = np.frombuffer(b"".join(pool[i][0] for i in idx), np.uint8).copy()
    sig = np.frombuffer(b"".join(pool[i][1] for i in idx), np.uint8).copy()
    m, off = pack_messages([pool[i][2] for i in idx])
    exp = np.array([pool[i][3] for i in idx], np.uint8)

    ctx = Context(device=0)
    dev = torch.device("cuda:0")
    d_pk, d_sig, d_m = (torch.from_numpy(a).to(dev) for a in (pk, sig, m))
    d_off = torch.from_numpy(off.view(np.int32).copy()).to(dev)
    d_valid = torch.zeros(args.n, dtype=torch.uint8, device=dev)
    d_words = torch.zeros((args.n + 63) // 64, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())

    def launch(valid):
        ctx.verify_secp256k1_device(args.n, d_pk.data_ptr(), d_sig.data_ptr(), d_m.data_ptr(), d_off.data_ptr(),
                                    d_valid.data_ptr() if valid else 0, d_words.data_ptr(), stream.cuda_stream)

    def check():
        stream.synchronize()
        got = d_valid.cpu().numpy()
        bits = np.unpackbits(d_words.cpu().numpy().view(np.uint8), bitorder="little")[: args.n]
        if not (np.array_equal(got, exp) and np.array_equal(bits, exp)):
            sys.exit(f"secp256k1_bench: verdicts differ from the reference at {np.nonzero(got != exp)[0][:10]}")

    launch(True)  # builds the fixed table
    check()
    for _ in range(args.warmup):
        launch(False)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        t0.record()
        for _ in range(args.launches):
            launch(False)
        t1.record()
    stream.synchronize()
    ms = t0.elapsed_time(t1) / args.launches
    launch(True)
    check()
    print(json.dumps({"tool": "secp256k1_bench", "n": args.n, "msg_len": args.msg_len, "keys": len(privs),
                      "launches": args.launches, "invalid": int((exp == 0).sum()),
                      "ms_per_batch": round(ms, 4), "verifs_per_s": round(args.n / ms * 1e3)}))


if __name__ == "__main__":
    main()
