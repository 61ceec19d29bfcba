#!/usr/bin/env python3
"""ValidatorSet.Hash() and Commit.Hash() on the device (cmtv_valset_hash,
cmtv_commit_hash, cmtv_commit_hashes) against the same trees on one CPU
thread. Needs a GPU; there is no CPU fallback. Writes
profiles/merkle_bench.json.

    python tools/bench_merkle.py [--reps 200] [--warmup 20] [--big 100000] [--out profiles/merkle_bench.json]

Per shape:
  wall_ms    p50 of a host clock around the blocking C call (arguments
             already packed, as a cgo shim holds them)
  kernel_ms  the passes' time between HIP events (CMTV_TIMING=1: every run is
             timed; cmtv_stats.device_ms), per call
  cpu_ms     the same trees hashed on one CPU thread by
             tests/host/merklecheck.cpp, the host build of merkle.h at -O2
             without sanitizers. A PROXY for the Go loop, not the reference:
             it encodes the leaves with the same register builders and hashes
             with the same portable SHA-256 (no SHA extensions).
Shapes: one set / one commit at n = 150 and 10,000; cmtv_commit_hashes at
7,000 x 150 and `--big` x 150. For the last, upload_ms is a pinned-memory
torch copy of as many bytes as the call stages, the share of the call that
is upload. crossover: the smallest n of a doubling sweep at which the device
call's p50 is below the proxy's. The roots of every timed shape are checked
against hashlib on a sample of trees first."""
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

import merkle_ref as R  # noqa: E402
from tests.host import hostbuild  # noqa: E402


def p8(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


class Commits:
    """H commits of n signatures (flag Commit, 64-byte signatures) in flat
    arrays, one cmtv_commit per height pointing into them."""

    def __init__(self, H, n, seed=1):
        from cometbft_amd import _native as N

        rng = np.random.default_rng(seed)
        t = H * n
        self.H, self.n = H, n
        self.flags = np.full(t + 1, 2, np.uint8)
        self.sec = (1_700_000_000 + np.arange(t + 1) // n).astype(np.int64)
        self.nanos = rng.integers(0, 10**9, t + 1, dtype=np.int32)
        self.sigs = rng.integers(0, 256, 64 * t + 4, dtype=np.uint8)
        self.addrs = rng.integers(0, 256, 20 * t + 4, dtype=np.uint8)
        self.off = (64 * np.arange(n + 1)).astype(np.uint32)
        self.arr = (N.cmtv_commit * H)()
        base = {k: getattr(self, k).ctypes.data for k in ("flags", "sec", "nanos", "sigs", "addrs")}
        u8, i64, i32 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
        off = self.off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        for h in range(H):
            c = self.arr[h]
            c.height, c.n_sigs, c.sig_off = h + 1, n, off
            c.flags = ctypes.cast(base["flags"] + h * n, u8)
            c.ts_seconds = ctypes.cast(base["sec"] + 8 * h * n, i64)
            c.ts_nanos = ctypes.cast(base["nanos"] + 4 * h * n, i32)
            c.sigs = ctypes.cast(base["sigs"] + 64 * h * n, u8)
            c.val_addrs = ctypes.cast(base["addrs"] + 20 * h * n, u8)
        self.out = (ctypes.c_uint8 * (32 * H))()
        self.staged_bytes = t * (4 + 8 + 4 + 1 + 20 + 64) + 8 * H

    def ref(self, h):
        n = self.n
        rows = [(2, self.addrs[20 * (h * n + i): 20 * (h * n + i) + 20].tobytes(), int(self.sec[h * n + i]),
                 int(self.nanos[h * n + i]), self.sigs[64 * (h * n + i): 64 * (h * n + i) + 64].tobytes())
                for i in range(n)]
        return R.commit_hash(rows)

    def call(self, ctx):
        from cometbft_amd import _native as N

        N.check(N.lib().cmtv_commit_hashes(ctx.handle, self.H, self.arr, self.out), "cmtv_commit_hashes")

    def check(self, ctx, sample):
        self.call(ctx)
        raw = bytes(self.out)
        for h in sample:
            assert raw[32 * h: 32 * h + 32] == self.ref(h), ("commit root", self.H, self.n, h)


class ValSets:
    """One set of n Ed25519 validators."""

    def __init__(self, n, seed=2):
        from cometbft_amd import _native as N

        rng = np.random.default_rng(seed)
        self.n = n
        self.pk = rng.integers(0, 256, 32 * n + 4, dtype=np.uint8)
        self.off = (32 * np.arange(n + 1)).astype(np.uint32)
        self.vp = rng.integers(1, 10**9, n + 1, dtype=np.int64)
        self.c = N.cmtv_valset(n_vals=n, pubkeys=p8(self.pk), pk_off=self.off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                               voting_power=self.vp.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
        self.out = (ctypes.c_uint8 * 32)()

    def call(self, ctx):
        from cometbft_amd import _native as N

        N.check(N.lib().cmtv_valset_hash(ctx.handle, ctypes.byref(self.c), None, self.out), "cmtv_valset_hash")

    def check(self, ctx, sample=None):
        self.call(ctx)
        want = R.valset_hash([(0, self.pk[32 * i: 32 * i + 32].tobytes(), int(self.vp[i])) for i in range(self.n)])
        assert bytes(self.out) == want, ("valset root", self.n)


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


def cpu_proxy(binary, kind, n_trees, n, reps):
    r = subprocess.run([binary, "bench", kind, str(n_trees), str(n), str(reps)], capture_output=True, check=True,
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
    ap.add_argument("--big", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle_bench.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_merkle.py needs a GPU")
    os.environ["CMTV_TIMING"] = "1"
    from cometbft_amd import Context

    ctx = Context(device=0)
    binary = hostbuild.build(os.path.join(ROOT, "tests", "host", "merklecheck.cpp"),
                             os.path.join(ROOT, "build", "merklecheck_bench"), ["-std=c++17"])
    props = torch.cuda.get_device_properties(0)
    clock_khz = getattr(props, "clock_rate", None)  # not every torch build reports it
    res = {"device": props.name, "arch": getattr(props, "gcnArchName", ""), "cus": props.multi_processor_count,
           "clock_mhz": clock_khz / 1e3 if clock_khz else None,
           "host": os.uname().nodename, "host_cpus_usable": len(os.sched_getaffinity(0)),
           "cpu_proxy": "tests/host/merklecheck.cpp bench, g++ -O2, one thread; a proxy for the Go loop, not the reference",
           "shapes": {}, "crossover": {}}
    for name, mk, kind in (("valset_hash", ValSets, "valset"), ("commit_hash", lambda n: Commits(1, n), "commit")):
        for n in (150, 10_000):
            shape = mk(n)
            shape.check(ctx, [0])
            r = timed(ctx, shape, a.reps, a.warmup)
            r["cpu_ms"] = cpu_proxy(binary, kind, 1, n, 50)
            res["shapes"][f"{name}_{n}"] = r
            print(name, n, r, flush=True)
        sweep = []
        for n in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024):
            shape = mk(n)
            dev = timed(ctx, shape, 100, 10)["wall_ms"]
            cpu = cpu_proxy(binary, kind, 1, n, 200)
            sweep.append({"n": n, "wall_ms": dev, "cpu_ms": cpu})
        wins = [s["n"] for s in sweep if s["wall_ms"] < s["cpu_ms"]]
        res["crossover"][name] = {"sweep": sweep, "smallest_n_device_wins": wins[0] if wins else None}
        print(name, "crossover", res["crossover"][name]["smallest_n_device_wins"], flush=True)
    for H, reps in ((7_000, 10), (a.big, 3)):
        shape = Commits(H, 150)
        shape.check(ctx, [0, H // 2, H - 1])
        r = timed(ctx, shape, reps, 1)
        r["cpu_ms"] = cpu_proxy(binary, "commit", H, 150, 3 if H <= 10_000 else 1)
        r["staged_bytes"] = shape.staged_bytes
        r["upload_ms"] = upload_ms(shape.staged_bytes)
        r["upload_share"] = r["upload_ms"] / r["wall_ms"]
        res["shapes"][f"commit_hashes_{H}x150"] = r
        print("commit_hashes", H, r, flush=True)
        del shape
    res["device_loses_at"] = [k for k, v in res["shapes"].items() if v["wall_ms"] >= v["cpu_ms"]]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"written": a.out, "device_loses_at": res["device_loses_at"]}))
    ctx.close()


if __name__ == "__main__":
    main()
