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

--keyed: the same device-resident inputs also go through
cmtv_verify_secp256k1_indexed_device, with the 150 keys registered
(cmtv_register_keys_secp256k1) and key indices in place of the key bytes. The
two paths alternate over the timed launches, each launch between its own pair
of events; both paths' verdicts are checked before and after. Also prints the
registration time of the 150 keys (host clock around the blocking call, after
a warm-up registration).
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time

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
    ap.add_argument("--keyed", action="store_true", help="A/B against the registered-key path")
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
    key_idx = np.array([i % len(privs) for i in idx], np.uint32)
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

    def check(what="generic"):
        stream.synchronize()
        got = d_valid.cpu().numpy()
        bits = np.unpackbits(d_words.cpu().numpy().view(np.uint8), bitorder="little")[: args.n]
        if not (np.array_equal(got, exp) and np.array_equal(bits, exp)):
            sys.exit(f"secp256k1_bench: {what} verdicts differ from the reference at {np.nonzero(got != exp)[0][:10]}")
        d_valid.zero_()
        d_words.zero_()
        torch.cuda.synchronize()

    if args.keyed:
        return keyed_ab(args, ctx, torch, stream, launch, check, pks, key_idx, (d_sig, d_m, d_off, d_valid, d_words),
                        int((exp == 0).sum()))

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
    print(json.dumps({"tool": "secp256k1_bench", "n": args.n, "msg_len": args.msg_len, "keys": len(pks),
                      "launches": args.launches, "invalid": int((exp == 0).sum()),
                      "ms_per_batch": round(ms, 4), "verifs_per_s": round(args.n / ms * 1e3)}))


def keyed_ab(args, ctx, torch, stream, launch_generic, check, pks, key_idx, bufs, invalid):
    """The generic and the registered-key path over the same buffers,
    alternating, each timed launch between its own pair of events."""
    d_sig, d_m, d_off, d_valid, d_words = bufs
    pk = np.frombuffer(b"".join(pks), np.uint8).reshape(-1, 33).copy()
    ctx.register_secp256k1_keys(pk).free()  # warm-up registration
    t = time.perf_counter()
    keys = ctx.register_secp256k1_keys(pk)
    register_ms = (time.perf_counter() - t) * 1e3
    d_idx = torch.from_numpy(key_idx.view(np.int32).copy()).to(d_sig.device)
    torch.cuda.synchronize()

    def launch_keyed(valid):
        ctx.verify_secp256k1_indexed_device(keys, args.n, d_idx.data_ptr(), d_sig.data_ptr(), d_m.data_ptr(),
                                            d_off.data_ptr(), d_valid.data_ptr() if valid else 0, d_words.data_ptr(),
                                            stream.cuda_stream)

    paths = (("generic", launch_generic), ("keyed", launch_keyed))
    for name, launch in paths:
        launch(True)
        check(name)
    for _ in range(args.warmup):
        for _, launch in paths:
            launch(False)
    events = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                     for _ in range(args.launches)] for name, _ in paths}
    with torch.cuda.stream(stream):
        for i in range(args.launches):
            for name, launch in paths:
                e0, e1 = events[name][i]
                e0.record()
                launch(False)
                e1.record()
    stream.synchronize()
    ms = {name: float(np.mean([e0.elapsed_time(e1) for e0, e1 in ev])) for name, ev in events.items()}
    p50 = {name: float(np.median([e0.elapsed_time(e1) for e0, e1 in ev])) for name, ev in events.items()}
    for name, launch in paths:
        launch(True)
        check(name)
    keys.free()
    print(json.dumps({"tool": "secp256k1_bench", "mode": "keyed", "n": args.n, "msg_len": args.msg_len,
                      "keys": len(pks), "launches": args.launches, "invalid": invalid,
                      "generic_ms_per_batch": round(ms["generic"], 4), "keyed_ms_per_batch": round(ms["keyed"], 4),
                      "generic_p50_ms": round(p50["generic"], 4), "keyed_p50_ms": round(p50["keyed"], 4),
                      "keyed_over_generic": round(ms["keyed"] / ms["generic"], 4),
                      "generic_verifs_per_s": round(args.n / ms["generic"] * 1e3),
                      "keyed_verifs_per_s": round(args.n / ms["keyed"] * 1e3),
                      "register_ms": round(register_ms, 3),
                      "table_bytes": len(pks) * 33 * 128 * 32 * 4}))


if __name__ == "__main__":
    main()
