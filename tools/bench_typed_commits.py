#!/usr/bin/env python3
"""Replay of an all-secp256k1 chain (150 validators) through
cmtv_verify_commits_typed, against the per-height loop of
cmtv_verify_commit_typed that was the only way before it, and the batched
kernel (k_verify_secp256k1_keyed_batch<KB>: KB signatures per lane sharing
one inversion mod n) against the one-signature-per-lane kernel inside the
same call. Needs a GPU; there is no CPU fallback.

    python tools/bench_typed_commits.py [--heights 67,700,1400,7000,14000] [--reps 30,10,8,5,4] [--warmup 2]
                                        [--real-keys]

Per number of heights H, the sides alternate in one loop, each a host clock
around a call that returns after its verdicts are back; medians are reported:
  loop      cmtv_verify_commit_typed once per height (capped at 700 heights)
  lane      cmtv_verify_commits_typed with the batched form disabled
            (CMTV_KEYED_BATCH_MIN_WAVES at its maximum): the unchanged
            k_verify_secp256k1_keyed_tmpl. THIS is the baseline of kb4 / kb8.
  kb4, kb8  the same call on contexts whose knob makes keyed_batch_kb pick
            KB = 4 / KB = 8 for this size
  default   the same call on a context opened without the knob: what ships
            (default_batched says whether it took the batched kernel)
All contexts have cmtv_keyset_cache on (registered keys; the set is registered
by the warm-up) and CMTV_TIMING=1, so cmtv_stats.device_ms gives each side's
summed kernel time too: *_kernel_ms is its median per call. lane_spread is
the run-to-run spread of `lane` ((p75 - p25) / median): a kb / lane ratio
within it of 1 is no difference.

Verdicts are checked before and after the timed loops: every side must return
CMTV_OK for every height of the good chain and "wrong signature (#i)" at the
flipped index of three heights of a bad one. Keys are consecutive multiples of
G, every signature uses one nonce and all validators of a height sign at one
timestamp (valid ECDSA, cheap to make: the verifier's work depends on none of
it). --real-keys builds the chain with the device signer instead
(testutil.make_secp256k1_validator_set: distinct derived keys in address order,
RFC 6979 nonces, a timestamp per validator), to measure that claim; the default
stays the cheap construction so recorded numbers remain comparable.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

CHAIN = "cmtverify-bench"
H0 = 1000
N_VALS = 150
LOOP_CAP = 700
BATCH_CHUNK = 1 << 20  # runtime_state.h kKeyedBatchChunk


def kb_for(n, min_waves):
    """runtime_state.h keyed_batch_kb."""
    kb = 1
    while kb < 8 and n > (min_waves - 1) * 64 * (kb * 2):
        kb *= 2
    return kb if kb >= 4 else 1


def open_ctx(min_waves):
    from cometbft_amd import Context

    old = {k: os.environ.get(k) for k in ("CMTV_KEYED_BATCH_MIN_WAVES", "CMTV_TIMING")}
    os.environ.pop("CMTV_KEYED_BATCH_MIN_WAVES", None)
    if min_waves is not None:
        os.environ["CMTV_KEYED_BATCH_MIN_WAVES"] = str(min_waves)
    os.environ["CMTV_TIMING"] = "1"
    try:
        ctx = Context(device=0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    ctx.keyset_cache(2)
    return ctx


class Chain:
    """H heights of one validator set as a cgo shim would hand them over:
    flat arrays, one cmtv_commit / cmtv_valset / cmtv_block_id per height."""

    def __init__(self, n_heights, real_ctx=None):
        import secp256k1_ref as S
        from bench_typed_commit import make_set
        from cometbft_amd import _native as N
        from cometbft_amd import testutil as TU
        from cometbft_amd import types as T

        n, H = N_VALS, n_heights
        self.N, self.H = N, H
        self.flags = np.full(n + 1, T.BLOCK_ID_FLAG_COMMIT, np.uint8)
        self.sig_off = (64 * np.arange(n + 1)).astype(np.uint32)
        self.addrs = np.zeros(20 * n + 1, np.uint8)
        self.bad = None
        if real_ctx is not None:
            self._init_real(real_ctx, S, TU)
            return
        privs, pks = make_set(n)
        self.vals = T.ValidatorSet([T.Validator(pk, 10, 0, "secp256k1") for pk in pks])
        self.vs, self._keep_v = self.vals._pack()
        u8p = ctypes.POINTER(ctypes.c_uint8)
        self.kt = self._keep_v[5].ctypes.data_as(u8p)
        k = int.from_bytes(hashlib.sha256(b"bench-typed-commits/nonce").digest(), "big") % S.N
        r = S.to_affine(S.gmul(k))[0] % S.N
        ki = pow(k, S.N - 2, S.N)
        rb = r.to_bytes(32, "big")
        rd = [r * d % S.N for d in privs]
        self.secs = np.zeros((H, n), np.int64)
        self.nanos = np.zeros((H, n), np.int32)
        self.hashes = np.zeros((H, 2, 32), np.uint8)
        sigs = bytearray(64 * n * H)
        self.sample = []
        for h in range(H):
            bid = TU.block_id_for_height(H0 + h)
            sec, nanos = TU.timestamp(H0 + h, 0)
            self.secs[h, :], self.nanos[h, :] = sec, nanos
            self.hashes[h, 0] = np.frombuffer(bid.hash, np.uint8)
            self.hashes[h, 1] = np.frombuffer(bid.part_set_header.hash, np.uint8)
            msg = T.vote_sign_bytes(CHAIN, T.PRECOMMIT_TYPE, H0 + h, 0, bid, sec, nanos)
            e = S.msg_scalar(msg)
            at = 64 * n * h
            for i in range(n):
                s = ki * (e + rd[i]) % S.N
                if s > S.HALF_N:
                    s = S.N - s
                sigs[at + 64 * i: at + 64 * i + 32] = rb
                sigs[at + 64 * i + 32: at + 64 * i + 64] = s.to_bytes(32, "big")
            if h % max(1, H // 8) == 0:
                self.sample.append((pks[h % n], msg, bytes(sigs[at + 64 * (h % n): at + 64 * (h % n) + 64])))
        for pk, msg, sig in self.sample:  # a sample against the reference verifier
            assert S.verify(pk, msg, sig)
        self.msg_len = len(msg)
        self.good = np.frombuffer(bytes(sigs), np.uint8).reshape(H, 64 * n).copy()

    def _init_real(self, ctx, S, TU, sign_heights=2048):
        """The same arrays from the device signer: derived keys, RFC 6979
        nonces, validator i of height h signing at testutil.timestamp(h, i)."""
        n, H = N_VALS, self.H
        sv = TU.make_secp256k1_validator_set(ctx, n)
        self.vals = sv.valset
        self.vs, self._keep_v = self.vals._pack()
        self.kt = self._keep_v[5].ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        self.addrs[:20 * n] = np.frombuffer(b"".join(v.address for v in self.vals.validators), np.uint8)
        ts = [[TU.timestamp(H0 + h, i) for i in range(n)] for h in range(H)]
        self.secs = np.array([[t[0] for t in row] for row in ts], np.int64)
        self.nanos = np.array([[t[1] for t in row] for row in ts], np.int32)
        self.hashes = np.zeros((H, 2, 32), np.uint8)
        for h in range(H):
            bid = TU.block_id_for_height(H0 + h)
            self.hashes[h, 0] = np.frombuffer(bid.hash, np.uint8)
            self.hashes[h, 1] = np.frombuffer(bid.part_set_header.hash, np.uint8)
        self.good = np.zeros((H, 64 * n), np.uint8)
        self.sample = []
        for c0 in range(0, H, sign_heights):
            hc = min(sign_heights, H - c0)
            m, off = TU.replay_messages(H0 + c0, hc, n)
            kidx = np.tile(np.arange(n, dtype=np.uint32), hc)
            self.good[c0:c0 + hc] = ctx.sign_secp256k1(sv.secrets, m, off, kidx).reshape(hc, 64 * n)
            i = c0 % n
            self.sample.append((self.vals.validators[i].pub_key, m[off[i]:off[i + 1]].tobytes(),
                                self.good[c0, 64 * i: 64 * i + 64].tobytes()))
        self.msg_len = int(off[1] - off[0])
        for pk, msg, sig in self.sample:  # a sample against the reference verifier
            assert S.verify(pk, msg, sig)

    def args(self, n_heights, sigs):
        """The C arrays of the first n_heights heights over the signature block `sigs`."""
        N = self.N
        u8p = ctypes.POINTER(ctypes.c_uint8)
        p8 = lambda a: a.ctypes.data_as(u8p)  # noqa: E731
        H = n_heights
        vs_arr = (N.cmtv_valset * H)()
        cm_arr = (N.cmtv_commit * H)()
        bid_arr = (N.cmtv_block_id * H)()
        heights = (ctypes.c_int64 * H)()
        kt_arr = (u8p * H)()
        i64p, i32p, u32p = (ctypes.POINTER(t) for t in (ctypes.c_int64, ctypes.c_int32, ctypes.c_uint32))
        for h in range(H):
            bid = N.cmtv_block_id(hash=p8(self.hashes[h, 0]), hash_len=32, psh_total=1, psh_hash=p8(self.hashes[h, 1]),
                                  psh_hash_len=32)
            vs_arr[h], bid_arr[h], heights[h], kt_arr[h] = self.vs, bid, H0 + h, self.kt
            cm_arr[h] = N.cmtv_commit(height=H0 + h, round=0, block_id=bid, n_sigs=N_VALS, flags=p8(self.flags),
                                      ts_seconds=self.secs[h].ctypes.data_as(i64p),
                                      ts_nanos=self.nanos[h].ctypes.data_as(i32p), sigs=p8(sigs[h]),
                                      sig_off=self.sig_off.ctypes.data_as(u32p), val_addrs=p8(self.addrs))
        return dict(n=H, vs=vs_arr, cm=cm_arr, bid=bid_arr, heights=heights, kt=kt_arr,
                    res=(N.cmtv_commit_result * H)(), rcs=(ctypes.c_int * H)())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heights", default="67,700,1400,7000,14000")
    ap.add_argument("--reps", default="30,10,8,5,4")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--real-keys", action="store_true",
                    help="derived keys, RFC 6979 nonces and per-validator timestamps from the device signer")
    args = ap.parse_args()
    hs = [int(x) for x in args.heights.split(",")]
    reps = [int(x) for x in args.reps.split(",")]

    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_typed_commits: needs a GPU")
    torch.cuda.init()
    from cometbft_amd import _native as N

    lib = N.lib()
    cid = CHAIN.encode()
    ctx_lane, ctx_kb8, ctx_def = open_ctx(1 << 20), open_ctx(1), open_ctx(None)
    chain = Chain(max(hs), ctx_def if args.real_keys else None)

    def many(ctx, a):
        rc = lib.cmtv_verify_commits_typed(ctx.handle, N.VERIFY_COMMIT, 0, cid, len(cid), a["n"], a["vs"], a["kt"],
                                           a["bid"], a["heights"], a["cm"], 0, 0, a["res"], a["rcs"], None, 0)
        assert rc == N.CMTV_OK, rc

    def loop(ctx, a, count):
        res = N.cmtv_commit_result()
        for h in range(count):
            a["rcs"][h] = lib.cmtv_verify_commit_typed(ctx.handle, N.VERIFY_COMMIT, 0, cid, len(cid),
                                                       ctypes.byref(a["vs"][h]), a["kt"][h], ctypes.byref(a["bid"][h]),
                                                       a["heights"][h], ctypes.byref(a["cm"][h]), 0, 0,
                                                       ctypes.byref(res), None, 0)
            a["res"][h] = res

    for H, rep in zip(hs, reps):
        n = H * N_VALS
        # KB = 4: the smallest knob whose widest KB for this launch size is 4
        cn = min(n, BATCH_CHUNK)
        mw4 = (cn + 511) // 512 + 1
        assert kb_for(cn, mw4) == 4 and kb_for(cn, 1) == 8 and kb_for(cn, 1 << 20) == 1
        ctx_kb4 = open_ctx(mw4)
        good = chain.args(H, chain.good)
        bad_sigs = chain.good[:H].copy()
        bad_at = {0: 3, H // 2: N_VALS - 1, H - 1: 77}
        for h, i in bad_at.items():
            bad_sigs[h, 64 * i + 40] ^= 1
        bad = chain.args(H, bad_sigs)
        n_loop = min(H, LOOP_CAP)
        sides = {"lane": (ctx_lane, lambda: many(ctx_lane, good)), "kb4": (ctx_kb4, lambda: many(ctx_kb4, good)),
                 "kb8": (ctx_kb8, lambda: many(ctx_kb8, good)), "default": (ctx_def, lambda: many(ctx_def, good)),
                 "loop": (ctx_lane, lambda: loop(ctx_lane, good, n_loop))}

        default_batched = [False]

        def check():
            for name, ctx in (("lane", ctx_lane), ("kb4", ctx_kb4), ("kb8", ctx_kb8), ("default", ctx_def)):
                s0 = ctx.stats()["secp_batch_launches"]
                many(ctx, good)
                assert all(good["rcs"][h] == N.CMTV_OK for h in range(H)), name
                launches = ctx.stats()["secp_batch_launches"] - s0
                if name == "default":
                    default_batched[0] = launches > 0
                else:
                    assert (launches > 0) == (name != "lane"), (name, launches)
                many(ctx, bad)
                for h in range(H):
                    want = bad_at.get(h)
                    assert bad["rcs"][h] == (N.CMTV_OK if want is None else N.CMTV_ECOMMIT), (name, h)
                    assert want is None or bad["res"][h].sig_index == want, (name, h, bad["res"][h].sig_index)
            loop(ctx_lane, bad, n_loop)
            for h in range(n_loop):
                want = bad_at.get(h)
                assert bad["rcs"][h] == (N.CMTV_OK if want is None else N.CMTV_ECOMMIT), ("loop", h)
                assert want is None or bad["res"][h].sig_index == want

        check()  # also registers the set on every context and builds the fixed table
        for _ in range(args.warmup):
            for _, f in sides.values():
                f()
        times = {k: [] for k in sides}
        kernel = {k: [] for k in sides}
        for _ in range(rep):
            for k, (ctx, f) in sides.items():
                d0 = ctx.stats()["device_ms"]
                t = time.perf_counter()
                f()
                times[k].append(time.perf_counter() - t)
                kernel[k].append(ctx.stats()["device_ms"] - d0)
        check()
        ctx_kb4.close()
        med = {k: float(np.median(v)) * 1e3 for k, v in times.items()}
        kmed = {k: float(np.median(v)) for k, v in kernel.items()}
        q = np.percentile(times["lane"], [25, 75])
        kq = np.percentile(kernel["lane"], [25, 75])
        scale = H / n_loop  # the loop's time for all H heights, had it run them
        print(json.dumps({
            "tool": "bench_typed_commits", "real_keys": args.real_keys, "heights": H, "validators": N_VALS, "signatures": n, "reps": rep,
            "msg_len": chain.msg_len, "loop_heights": n_loop,
            **{k + "_ms": round(v, 4) for k, v in med.items()},
            **{k + "_kernel_ms": round(v, 4) for k, v in kmed.items()},
            "lane_msigs_per_s": round(n / med["lane"] / 1e3, 3),
            "loop_msigs_per_s": round(n_loop * N_VALS / med["loop"] / 1e3, 4),
            "lane_over_loop": round(med["lane"] / (med["loop"] * scale), 5),
            "default_batched": default_batched[0], "default_over_lane": round(med["default"] / med["lane"], 4),
            "default_over_lane_kernel": round(kmed["default"] / kmed["lane"], 4) if kmed["lane"] else None,
            "kb4_over_lane": round(med["kb4"] / med["lane"], 4), "kb8_over_lane": round(med["kb8"] / med["lane"], 4),
            "kb4_over_lane_kernel": round(kmed["kb4"] / kmed["lane"], 4) if kmed["lane"] else None,
            "kb8_over_lane_kernel": round(kmed["kb8"] / kmed["lane"], 4) if kmed["lane"] else None,
            "lane_spread": round(float(q[1] - q[0]) * 1e3 / med["lane"], 4),
            "lane_kernel_spread": round(float(kq[1] - kq[0]) / kmed["lane"], 4) if kmed["lane"] else None,
            "mac_ratio_kb4": 0.67, "mac_ratio_kb8": 0.62}), flush=True)
    ctx_lane.close()
    ctx_kb8.close()
    ctx_def.close()


if __name__ == "__main__":
    main()
