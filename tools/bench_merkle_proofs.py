#!/usr/bin/env python3
"""Merkle proofs on the device (cmtv_merkle_proofs, cmtv_txs_proofs,
cmtv_part_set_proofs, cmtv_merkle_proofs_verify) against the root calls on
the same trees and against one CPU thread. Needs a GPU; there is no CPU
fallback. Writes profiles/merkle_proof_bench.json.

    python tools/bench_merkle_proofs.py [--reps 50] [--warmup 5] [--out profiles/merkle_proof_bench.json]
                                        [--parts-only]

Per shape:
  wall_ms    p50 of a host clock around the blocking C call (arguments
             already packed, as a cgo shim holds them); `reps` calls after
             `warmup` calls, both recorded with the row
  kernel_ms  the launches' time between HIP events (CMTV_TIMING=1: every run
             is timed; cmtv_stats.device_ms), per call
  roots_ms   for a building row, the wall p50 of cmtv_merkle_roots /
             cmtv_txs_hashes on the same trees in the same process:
             wall_ms / roots_ms is the price of proofs over roots
  cpu_ms     the same work on one CPU thread by tests/host/
             merkleproofcheck.cpp, the host build of merkle_proof.h at -O2
             without sanitizers. A PROXY for the Go loop, not the reference:
             it runs the kernels' lane code with the same portable SHA-256
             (no SHA extensions).
crossover: the smallest leaf count of a doubling sweep at which the device
call's p50 is below the proxy's, for building one tree of 32-byte items and
for verifying that tree's proofs; crossover.part_set is the same sweep over
the number of 64 KiB parts of a part set (10 calls after 2 warm-up calls a
point; --parts-only measures that sweep alone and adds it to the file that
is already there). Every timed shape is first checked: the
built roots against the root call, and every built proof through the verify
call."""
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

from tests.host import hostbuild  # noqa: E402

u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
i64p = ctypes.POINTER(ctypes.c_int64)


def p8(a):
    return a.ctypes.data_as(u8p)


def p32(a):
    return a.ctypes.data_as(u32p)


class Build:
    """n_trees trees of n items of item_len bytes, and the buffers of a building call."""

    def __init__(self, kind, n_trees, n, item_len, seed=1):
        from cometbft_amd import _native as N

        self.kind, self.n_trees, self.n, self.item_len = kind, n_trees, n, item_len
        t = n_trees * n
        self.items = np.random.default_rng(seed).integers(0, 256, t * item_len + 4, dtype=np.uint8)
        self.item_off = (item_len * np.arange(t + 1, dtype=np.uint64)).astype(np.uint32)
        self.tree_off = (n * np.arange(n_trees + 1, dtype=np.uint64)).astype(np.uint32)
        na = ctypes.c_uint64()
        N.check(N.lib().cmtv_merkle_proofs_len(n_trees, p32(self.tree_off), ctypes.byref(na)), "cmtv_merkle_proofs_len")
        self.n_aunts = na.value
        self.roots = np.zeros(32 * n_trees, np.uint8)
        self.roots2 = np.zeros(32 * n_trees, np.uint8)
        self.lh = np.zeros(32 * t, np.uint8)
        self.aunt_off = np.zeros(t + 1, np.uint32)
        self.aunts = np.zeros(32 * max(self.n_aunts, 1), np.uint8)
        self.fn = N.lib().cmtv_txs_proofs if kind == "txs" else N.lib().cmtv_merkle_proofs
        self.fn_roots = N.lib().cmtv_txs_hashes if kind == "txs" else N.lib().cmtv_merkle_roots

    def call(self, ctx):
        from cometbft_amd import _native as N

        N.check(self.fn(ctx.handle, self.n_trees, p32(self.tree_off), p8(self.items), p32(self.item_off),
                        p8(self.roots), p8(self.lh), p32(self.aunt_off), p8(self.aunts), self.n_aunts), "proofs")

    def call_roots(self, ctx):
        from cometbft_amd import _native as N

        N.check(self.fn_roots(ctx.handle, self.n_trees, p32(self.tree_off), p8(self.items), p32(self.item_off),
                              p8(self.roots2)), "roots")

    def verifier(self, limit=None):
        """The verify call over this shape's own proofs (the first `limit` of them)."""
        t = self.n_trees * self.n if limit is None else limit
        v = Verify(self.kind)
        v.n = t
        v.total = np.full(t, self.n, np.int64)
        v.index = (np.arange(t) % self.n).astype(np.int64)
        v.lh, v.aunt_off, v.aunts = self.lh, self.aunt_off, self.aunts
        v.roots, v.n_roots = self.roots, self.n_trees
        v.root_idx = (np.arange(t) // self.n).astype(np.uint32)
        v.leaves, v.leaf_off = self.items, self.item_off
        v.status = np.zeros(t, np.uint8)
        return v

    def check(self, ctx):
        self.call(ctx)
        self.call_roots(ctx)
        assert np.array_equal(self.roots, self.roots2), "roots"
        v = self.verifier()
        v.call(ctx)
        assert not v.status.any(), "a built proof does not verify"


class Verify:
    def __init__(self, kind):
        self.leaf_kind = 1 if kind == "txs" else 0

    def call(self, ctx):
        from cometbft_amd import _native as N

        N.check(N.lib().cmtv_merkle_proofs_verify(
            ctx.handle, self.n, self.total.ctypes.data_as(i64p), self.index.ctypes.data_as(i64p), p8(self.lh),
            p32(self.aunt_off), p8(self.aunts), self.n_roots, p8(self.roots), p32(self.root_idx), p8(self.leaves),
            p32(self.leaf_off), self.leaf_kind, p8(self.status), None, None), "verify")


class PartSet:
    def __init__(self, size, part_size=65536, seed=3):
        from cometbft_amd import _native as N

        self.size, self.part_size = size, part_size
        self.data = np.random.default_rng(seed).integers(0, 256, size + 4, dtype=np.uint8)
        n = (size + part_size - 1) // part_size
        self.n = n
        self.n_aunts = sum(N.lib().cmtv_merkle_proof_len(n, i) for i in range(n))
        self.total = ctypes.c_uint32()
        self.root = np.zeros(32, np.uint8)
        self.lh = np.zeros(32 * n, np.uint8)
        self.aunt_off = np.zeros(n + 1, np.uint32)
        self.aunts = np.zeros(32 * max(self.n_aunts, 1), np.uint8)
        self.item_off = np.minimum(part_size * np.arange(n + 1, dtype=np.uint64), size).astype(np.uint32)
        self.tree_off = np.array([0, n], np.uint32)
        self.roots2 = np.zeros(32, np.uint8)

    def call(self, ctx):
        from cometbft_amd import _native as N

        N.check(N.lib().cmtv_part_set_proofs(ctx.handle, p8(self.data), self.size, self.part_size,
                                             ctypes.byref(self.total), p8(self.root), p8(self.lh), p32(self.aunt_off),
                                             p8(self.aunts), self.n_aunts), "cmtv_part_set_proofs")

    def call_roots(self, ctx):
        from cometbft_amd import _native as N

        N.check(N.lib().cmtv_merkle_roots(ctx.handle, 1, p32(self.tree_off), p8(self.data), p32(self.item_off),
                                          p8(self.roots2)), "cmtv_merkle_roots")

    def verifier(self):
        """PartSet.AddPart of every part: the proofs on one root."""
        v = Verify("items")
        v.n = self.n
        v.total = np.full(self.n, self.n, np.int64)
        v.index = np.arange(self.n, dtype=np.int64)
        v.lh, v.aunt_off, v.aunts = self.lh, self.aunt_off, self.aunts
        v.roots, v.n_roots = self.root, 1
        v.root_idx = np.zeros(self.n, np.uint32)
        v.leaves, v.leaf_off = self.data, self.item_off
        v.status = np.zeros(self.n, np.uint8)
        return v

    def check(self, ctx):
        self.call(ctx)
        self.call_roots(ctx)
        assert self.total.value == self.n and np.array_equal(self.root, self.roots2), "part set root"
        v = self.verifier()
        v.call(ctx)
        assert not v.status.any(), "a part's proof does not verify"


def timed(ctx, call, reps, warmup):
    for _ in range(warmup):
        call(ctx)
    s0 = ctx.stats()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call(ctx)
        wall.append((time.perf_counter() - t0) * 1e3)
    s1 = ctx.stats()
    return {"wall_ms": statistics.median(wall), "wall_min_ms": min(wall), "reps": reps, "warmup": warmup,
            "kernel_ms": (s1["device_ms"] - s0["device_ms"]) / reps,
            "launches_per_call": (s1["kernel_launches"] - s0["kernel_launches"]) / reps}


def cpu_proxy(binary, what, kind, a, b, c, reps):
    r = subprocess.run([binary, "bench", what, "1" if kind == "txs" else "0", str(a), str(b), str(c), str(reps)],
                       capture_output=True, check=True, timeout=1200)
    return json.loads(r.stdout)["p50_ms"]


def build_row(ctx, binary, shape, reps, warmup, cpu_reps):
    shape.check(ctx)
    r = timed(ctx, shape.call, reps, warmup)
    r["roots_ms"] = timed(ctx, shape.call_roots, reps, warmup)["wall_ms"]
    r["proofs_over_roots"] = r["wall_ms"] / r["roots_ms"]
    if isinstance(shape, PartSet):
        r["cpu_ms"] = cpu_proxy(binary, "build", "items", 1, shape.n, shape.part_size, cpu_reps)
    else:
        r["cpu_ms"] = cpu_proxy(binary, "build", shape.kind, shape.n_trees, shape.n, shape.item_len, cpu_reps)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle_proof_bench.json"))
    ap.add_argument("--parts-only", action="store_true")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_merkle_proofs.py needs a GPU")
    os.environ["CMTV_TIMING"] = "1"
    from cometbft_amd import Context

    ctx = Context(device=0)
    binary = hostbuild.build(os.path.join(ROOT, "tests", "host", "merkleproofcheck.cpp"),
                             os.path.join(ROOT, "build", "merkleproofcheck_bench"), ["-std=c++17"])
    props = torch.cuda.get_device_properties(0)
    res = {"device": props.name, "arch": getattr(props, "gcnArchName", ""), "cus": props.multi_processor_count,
           "host": os.uname().nodename, "host_cpus_usable": len(os.sched_getaffinity(0)),
           "cpu_proxy": "tests/host/merkleproofcheck.cpp bench, g++ -O2, one thread; a proxy for the Go loop, "
                        "not the reference",
           "shapes": {}, "crossover": {}}

    def put(name, r):
        res["shapes"][name] = r
        print(name, r, flush=True)

    def part_sweep():
        sweep = []
        for parts in (1, 2, 4, 8, 16, 24, 32, 48, 64, 96, 128, 256):
            shape = PartSet(parts * 65536)
            shape.check(ctx)
            dev = timed(ctx, shape.call, 10, 2)
            cpu = cpu_proxy(binary, "build", "items", 1, parts, 65536, 3)
            sweep.append({"parts": parts, "wall_ms": dev["wall_ms"], "kernel_ms": dev["kernel_ms"], "cpu_ms": cpu})
        wins = [s["parts"] for s in sweep if s["wall_ms"] < s["cpu_ms"]]
        res["crossover"]["part_set"] = {"sweep": sweep, "smallest_parts_device_wins": wins[0] if wins else None}
        print("part_set crossover", res["crossover"]["part_set"], flush=True)

    if a.parts_only:
        with open(a.out) as f:
            res = json.load(f)
        part_sweep()
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        ctx.close()
        return

    for n in (150, 10_000, 65_537):
        shape = Build("items", 1, n, 32)
        put(f"merkle_proofs_1x{n}", build_row(ctx, binary, shape, a.reps, a.warmup, 5 if n > 1000 else 50))
        if n == 10_000:  # verifying: 10,000 proofs of depth 14
            v = shape.verifier()
            r = timed(ctx, v.call, a.reps, a.warmup)
            r["cpu_ms"] = cpu_proxy(binary, "verify", "items", n, n, 32, 5)
            put("verify_10000_depth14", r)
    shape = Build("txs", a.blocks, 10, 250)
    put(f"txs_proofs_{a.blocks}x10x250", build_row(ctx, binary, shape, 5, 1, 1))
    # verifying: 100,000 transaction proofs of depth 4 (TxProof.Validate), each block's on its own root
    v = shape.verifier(limit=100_000)
    r = timed(ctx, v.call, 10, 2)
    r["cpu_ms"] = cpu_proxy(binary, "verify", "txs", 100_000, 10, 250, 3)
    put("verify_100000_depth4_txs", r)
    del shape, v
    for size, label in ((65536, "64KiB"), (1 << 20, "1MiB"), (21 << 20, "21MiB")):
        shape = PartSet(size)
        put(f"part_set_{label}", build_row(ctx, binary, shape, 20, 3, 3))
        if label == "21MiB":  # PartSet.AddPart of 336 parts of 64 KiB on one root
            v = shape.verifier()
            r = timed(ctx, v.call, 20, 3)
            r["cpu_ms"] = cpu_proxy(binary, "verify", "items", shape.n, shape.n, 65536, 3)
            put("verify_336_parts_64KiB", r)
    for what in ("build", "verify"):
        sweep = []
        for n in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096):
            shape = Build("items", 1, n, 32)
            shape.check(ctx)
            call = shape.call if what == "build" else shape.verifier().call
            dev = timed(ctx, call, 100, 10)["wall_ms"]
            cpu = cpu_proxy(binary, what, "items", *((1, n, 32) if what == "build" else (n, n, 32)), 50)
            sweep.append({"n": n, "wall_ms": dev, "cpu_ms": cpu})
        wins = [s["n"] for s in sweep if s["wall_ms"] < s["cpu_ms"]]
        res["crossover"][what] = {"sweep": sweep, "smallest_n_device_wins": wins[0] if wins else None}
        print(what, "crossover", res["crossover"][what]["smallest_n_device_wins"], flush=True)
    part_sweep()
    res["device_loses_at"] = [k for k, v in res["shapes"].items() if v["wall_ms"] >= v["cpu_ms"]]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"written": a.out, "device_loses_at": res["device_loses_at"]}))
    ctx.close()


if __name__ == "__main__":
    main()
