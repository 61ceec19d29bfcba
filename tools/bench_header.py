#!/usr/bin/env python3
"""Header.Hash() and Txs.Hash() on the device (cmtv_header_hashes,
cmtv_txs_hash[es]) against the only route the library had before
(cmtv_merkle_roots over the headers' 14 leaves, encoded by the caller) and
against the same hashes on one CPU thread. Needs a GPU; there is no CPU
fallback. Writes profiles/header_bench.json.

    python tools/bench_header.py [--reps 200] [--warmup 20] [--big 100000] [--out profiles/header_bench.json]

Header shapes: 1, 16, 256, 4,096 and `--big` headers of 32-byte hashes, a
20-byte proposer address and a 15-character chain id. Per shape:
  wall_ms    p50 of a host clock around the blocking C call (arguments
             already packed, as a cgo shim holds them)
  kernel_ms  the launch's time between HIP events (CMTV_TIMING=1: every run
             is timed; cmtv_stats.device_ms), per call
  cpu_ms     the same headers hashed on one CPU thread by
             tests/host/headercheck.cpp, the host build of header.h at -O2
             without sanitizers. A PROXY for the Go loop, not the reference:
             it encodes the leaves with the same register builders and hashes
             with the same portable SHA-256 (no SHA extensions).
  upload_ms  (at `--big`) a pinned-memory torch copy of as many bytes as the
             call stages, the share of the call that is upload
  vs_items   the comparison that chose the kernel: in this process,
             alternating call by call, cmtv_header_hashes and cmtv_merkle_roots
             over the same headers' leaves (encoded before the timed window,
             which favours the items route). The whole alternation is repeated
             `rounds` times; p50_ms is the median of the rounds' p50s and
             spread_ms their range, the margin a difference has to exceed.
Transaction shapes: 1,000 transactions of 250 bytes in one block, and
`--big` blocks of 10 such transactions: wall_ms and cpu_ms.
crossover: the smallest count of a doubling sweep at which the device call's
p50 is below the proxy's, for headers per call and for transactions per call.
The roots of every timed shape are checked against hashlib on a sample first."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import header_ref as H  # noqa: E402
from tests.host import hostbuild  # noqa: E402

# a header's byte fields in staging order: chain id, LastBlockID's two hashes, eight hashes, the address
FIELD_LENS = [15, 32, 32] + [32] * 8 + [20]
STRIDE = sum(FIELD_LENS)


def p8(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def p32(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


class Headers:
    """n headers in flat arrays, one cmtv_header each pointing into them."""

    def __init__(self, n, seed=1):
        from cometbft_amd import _native as N

        rng = np.random.default_rng(seed)
        self.n = n
        self.var = rng.integers(0, 256, n * STRIDE + 4, dtype=np.uint8)
        cid = self.var[:n * STRIDE].reshape(n, STRIDE)[:, :FIELD_LENS[0]]
        cid[:] = cid % 26 + 97  # a printable chain id
        self.height = (1_000_000 + np.arange(n)).astype(np.int64)
        self.sec = (1_700_000_000 + 6 * np.arange(n)).astype(np.int64)
        self.nanos = rng.integers(0, 10**9, n, dtype=np.int32)
        self.total = rng.integers(1, 64, n, dtype=np.uint32)
        C = N.cmtv_header
        self.arr = (C * n)()
        raw = np.frombuffer(self.arr, np.uint8).reshape(n, ctypes.sizeof(C))

        def col(offset, values):
            v = np.ascontiguousarray(values)
            raw[:, offset: offset + v.itemsize] = v.view(np.uint8).reshape(n, v.itemsize)

        base = self.var.ctypes.data + STRIDE * np.arange(n, dtype=np.uint64)
        starts = np.concatenate([[0], np.cumsum(FIELD_LENS)[:-1]]).astype(np.uint64)
        bid = C.last_block_id.offset
        col(C.version_block.offset, np.full(n, 11, np.uint64))
        col(C.version_app.offset, np.full(n, 1, np.uint64))
        col(C.chain_id.offset, base + starts[0])
        col(C.chain_id_len.offset, np.full(n, FIELD_LENS[0], np.uint32))
        col(C.height.offset, self.height)
        col(C.time_seconds.offset, self.sec)
        col(C.time_nanos.offset, self.nanos)
        col(bid + N.cmtv_block_id.hash.offset, base + starts[1])
        col(bid + N.cmtv_block_id.hash_len.offset, np.full(n, 32, np.uint32))
        col(bid + N.cmtv_block_id.psh_total.offset, self.total)
        col(bid + N.cmtv_block_id.psh_hash.offset, base + starts[2])
        col(bid + N.cmtv_block_id.psh_hash_len.offset, np.full(n, 32, np.uint32))
        for f in range(9):
            col(C.field.offset + 8 * f, base + starts[3 + f])
            col(C.field_len.offset + 4 * f, np.full(n, FIELD_LENS[3 + f], np.uint32))
        self.out = (ctypes.c_uint8 * (32 * n))()
        self.staged_bytes = n * (8 * 4 + 4 * 12 + 4 * 2 + STRIDE)

    def hdr(self, h) -> H.Hdr:
        b = self.var[h * STRIDE: (h + 1) * STRIDE].tobytes()
        parts, at = [], 0
        for ln in FIELD_LENS:
            parts.append(b[at: at + ln])
            at += ln
        return H.Hdr(11, 1, parts[0], int(self.height[h]), int(self.sec[h]), int(self.nanos[h]), parts[1],
                     int(self.total[h]), parts[2], *parts[3:])

    def call(self, ctx):
        from cometbft_amd import _native as N

        N.check(N.lib().cmtv_header_hashes(ctx.handle, self.n, self.arr, self.out, None), "cmtv_header_hashes")

    def check(self, ctx, sample):
        self.call(ctx)
        raw = bytes(self.out)
        for h in sample:
            assert raw[32 * h: 32 * h + 32] == H.header_hash(self.hdr(h)), ("header root", self.n, h)


class HeaderItems:
    """The same headers as trees of 14 encoded leaves: cmtv_merkle_roots."""

    def __init__(self, hs: Headers):
        self.n = hs.n
        leaves = [leaf for h in range(hs.n) for leaf in H.leaves(hs.hdr(h))]
        self.items = np.frombuffer(b"".join(leaves) + b"\0\0\0\0", np.uint8).copy()
        self.item_off = np.zeros(len(leaves) + 1, np.uint32)
        self.item_off[1:] = np.cumsum([len(x) for x in leaves])
        self.tree_off = (14 * np.arange(hs.n + 1)).astype(np.uint32)
        self.out = (ctypes.c_uint8 * (32 * hs.n))()

    def call(self, ctx):
        from cometbft_amd import _native as N

        N.check(N.lib().cmtv_merkle_roots(ctx.handle, self.n, p32(self.tree_off), p8(self.items), p32(self.item_off),
                                          self.out), "cmtv_merkle_roots")


class Txs:
    """n_blocks blocks of n_txs transactions of tx_len bytes."""

    def __init__(self, n_blocks, n_txs, tx_len, seed=3):
        rng = np.random.default_rng(seed)
        self.n_blocks, self.n_txs, self.tx_len = n_blocks, n_txs, tx_len
        t = n_blocks * n_txs
        self.txs = rng.integers(0, 256, t * tx_len + 4, dtype=np.uint8)
        self.tx_off = (tx_len * np.arange(t + 1)).astype(np.uint32)
        self.block_off = (n_txs * np.arange(n_blocks + 1)).astype(np.uint32)
        self.out = (ctypes.c_uint8 * (32 * n_blocks))()

    def call(self, ctx):
        from cometbft_amd import _native as N

        N.check(N.lib().cmtv_txs_hashes(ctx.handle, self.n_blocks, p32(self.block_off), p8(self.txs), p32(self.tx_off),
                                        self.out), "cmtv_txs_hashes")

    def check(self, ctx, sample):
        self.call(ctx)
        raw = bytes(self.out)
        per = self.n_txs * self.tx_len
        for b in sample:
            blob = self.txs[b * per: (b + 1) * per].tobytes()
            want = H.txs_hash([blob[i * self.tx_len: (i + 1) * self.tx_len] for i in range(self.n_txs)])
            assert raw[32 * b: 32 * b + 32] == want, ("txs root", self.n_blocks, b)


def timed(ctx, shape, reps, warmup):
    for _ in range(warmup):
        shape.call(ctx)
    s0 = ctx.stats()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        shape.call(ctx)
        wall.append((time.perf_counter() - t0) * 1e3)
    s1 = ctx.stats()
    return {"wall_ms": statistics.median(wall), "wall_min_ms": min(wall), "reps": reps,
            "kernel_ms": (s1["device_ms"] - s0["device_ms"]) / reps,
            "launches_per_call": (s1["kernel_launches"] - s0["kernel_launches"]) / reps}


def alternating(ctx, a, b, reps, warmup, rounds):
    """a and b call by call, the whole alternation `rounds` times: per route
    the median of the rounds' p50s and their range."""
    for _ in range(warmup):
        a.call(ctx)
        b.call(ctx)
    p50s = ([], [])
    for _ in range(rounds):
        walls = ([], [])
        for _ in range(reps):
            for k, s in enumerate((a, b)):
                t0 = time.perf_counter()
                s.call(ctx)
                walls[k].append((time.perf_counter() - t0) * 1e3)
        for k in range(2):
            p50s[k].append(statistics.median(walls[k]))
    return [{"p50_ms": statistics.median(p), "spread_ms": max(p) - min(p), "round_p50s_ms": p} for p in p50s]


def cpu_proxy(binary, args, reps):
    r = subprocess.run([binary, "bench"] + [str(x) for x in args] + [str(reps)], capture_output=True, check=True,
                       timeout=1200)
    return json.loads(r.stdout)["p50_ms"]


def upload_ms(nbytes, reps=5):
    import torch

    src = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    ts = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dst.copy_(src, non_blocking=True)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--big", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "header_bench.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_header.py needs a GPU")
    os.environ["CMTV_TIMING"] = "1"
    from cometbft_amd import Context

    ctx = Context(device=0)
    binary = hostbuild.build(os.path.join(ROOT, "tests", "host", "headercheck.cpp"),
                             os.path.join(ROOT, "build", "headercheck_bench"), ["-std=c++17"])
    props = torch.cuda.get_device_properties(0)
    res = {"device": props.name, "arch": getattr(props, "gcnArchName", ""), "cus": props.multi_processor_count,
           "host": os.uname().nodename, "host_cpus_usable": len(os.sched_getaffinity(0)),
           "cpu_proxy": "tests/host/headercheck.cpp bench, g++ -O2, one thread; a proxy for the Go loop, not the reference",
           "vs_items": "cmtv_header_hashes and cmtv_merkle_roots over the same headers' encoded leaves, alternating; "
                       "the leaves' encoding is outside the timed window",
           "shapes": {}, "crossover": {}}
    for n in (1, 16, 256, 4096, a.big):
        big = n > 10_000
        hs = Headers(n)
        hs.check(ctx, sorted({0, n // 2, n - 1}))
        reps, warmup, rounds = (5, 1, 3) if big else (a.reps, a.warmup, a.rounds)
        r = timed(ctx, hs, reps, warmup)
        r["cpu_ms"] = cpu_proxy(binary, ["header", n], 3 if big else 50)
        items = HeaderItems(hs)
        items.call(ctx)
        assert bytes(items.out) == bytes(hs.out), ("the two routes' roots", n)
        new, old = alternating(ctx, hs, items, reps, warmup, rounds)
        r["vs_items"] = {"header_hashes": new, "merkle_roots": old,
                         "header_hashes_not_higher": new["p50_ms"] <= old["p50_ms"] + max(new["spread_ms"], old["spread_ms"])}
        r["items_kernel_ms"] = timed(ctx, items, reps, warmup)["kernel_ms"]
        if big:
            r["staged_bytes"] = hs.staged_bytes
            r["upload_ms"] = upload_ms(hs.staged_bytes)
            r["upload_share"] = r["upload_ms"] / r["wall_ms"]
        res["shapes"][f"header_hashes_{n}"] = r
        print("header_hashes", n, r, flush=True)
        del hs, items
    sweep = []
    for n in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024):
        dev = timed(ctx, Headers(n), 100, 10)["wall_ms"]
        sweep.append({"n": n, "wall_ms": dev, "cpu_ms": cpu_proxy(binary, ["header", n], 200)})
    wins = [s["n"] for s in sweep if s["wall_ms"] < s["cpu_ms"]]
    res["crossover"]["headers_per_call"] = {"sweep": sweep, "smallest_n_device_wins": wins[0] if wins else None}
    print("header crossover", wins[:1], flush=True)
    for nb, nt, reps in ((1, 1000, a.reps), (a.big, 10, 3)):
        shape = Txs(nb, nt, 250)
        shape.check(ctx, sorted({0, nb // 2, nb - 1}))
        r = timed(ctx, shape, reps, 1 if nb > 1 else a.warmup)
        r["cpu_ms"] = cpu_proxy(binary, ["txs", nb, nt, 250], 1 if nb > 10_000 else 50)
        res["shapes"][f"txs_hashes_{nb}x{nt}x250"] = r
        print("txs_hashes", nb, nt, r, flush=True)
        del shape
    sweep = []
    for n in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096):
        dev = timed(ctx, Txs(1, n, 250), 100, 10)["wall_ms"]
        sweep.append({"n": n, "wall_ms": dev, "cpu_ms": cpu_proxy(binary, ["txs", 1, n, 250], 200)})
    wins = [s["n"] for s in sweep if s["wall_ms"] < s["cpu_ms"]]
    res["crossover"]["txs_per_call"] = {"sweep": sweep, "smallest_n_device_wins": wins[0] if wins else None}
    print("txs crossover", wins[:1], flush=True)
    res["device_loses_at"] = [k for k, v in res["shapes"].items() if v["wall_ms"] >= v["cpu_ms"]]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"written": a.out, "device_loses_at": res["device_loses_at"]}))
    ctx.close()


if __name__ == "__main__":
    main()
