"""GPU parity of k_verify_quad_hs_fold with its window sums software-pipelined
over the two waves of the helper's SIMD (cometbft_amd/csrc/hs_helper.h
hs_helper_sums_pipe, quad.h h_sums_pipe): the hash helper and the comb wave
form every second window's S_w = [dA](-A) + [dR](-/+R) each, the front half
in one window and the back half and the store to the ring in the next, and
meet only at the window barriers -- no flag, no poll, no late path, so neither
counter of late waves may move because of it.

Contexts: CMTV_HS_SUM_PIPE=1 (the pipeline); CMTV_HS_SUM_PIPE=0 (the hash
helper sums alone); the pipeline with CMTV_FORCE_WIDE=1 (64 windows), with
CMTV_FORCE_PS_LATE=1 (the comb wave skips its share of [s]B and goes straight
to the sums; every quad wave counts in late_ps_waves), and with CMTV_HS_PRE at
0 and 16 (the comb wave reaches barrier 1 first or last).

Sizes: 1 and 16 (one signature; one full quad wave), 47 / 48 / 49 (the helper
lanes t >= 48 and their clamped slot; a second workgroup holding one
signature), 97 (three workgroups, the last nearly empty), 145 (holds the 35-
and 36-window vectors, each at another lane of another wave: odd and even
window counts, so either wave stores the last sum).

Inputs: about a third honest, the others with one flipped bit in the
signature, the key or the message, and s at 0, 1, L - 1, L, L + 1, 2^252.
Verdicts are compared with the C oracle bit for bit in both modes, the bitmap
with the byte verdicts. The CPU side is tests/test_sum_pipe_host.py."""
import json
import os

import numpy as np
import pytest

from oracle import coracle
from cometbft_amd import MODE_GO_STDLIB, MODE_ZIP215, pack_messages

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 2**252 + 27742317777372353535851937790883648493
SIZES = [1, 16, 47, 48, 49, 97, 145]
MODES = [(MODE_GO_STDLIB, "go"), (MODE_ZIP215, "zip215")]
S_EDGES = [0, 1, L - 1, L, L + 1, 2**252]
CONTEXTS = ["pipe", "alone", "pipe-wide", "pipe-ps-late", "pipe-pre0", "pipe-pre16"]


@pytest.fixture(scope="module")
def pool():
    """145 signatures, the oracle's verdicts computed once. Entry i is honest
    (i % 6 in 0, 3) or carries one flipped bit in s (1), R (2), A (4) or the
    message (5); the s edge values replace s at entries 5, 12, 19, ... (the
    first two inside the first wave); the wide vectors sit at lane
    (7 + 3 w) % 16 of wave w + 1."""
    rng = np.random.default_rng(41)
    n = 145
    seeds = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    msgs = [rng.integers(0, 256, 70 + i % 50, dtype=np.uint8).tobytes() for i in range(n)]
    m, off = coracle.pack_msgs(msgs)
    sig = coracle.sign_batch(seeds, m, off, nthreads=8).copy()
    pk = coracle.pubkeys_from_seeds(seeds).copy()
    for i in range(n):
        bit = 1 << int(rng.integers(0, 8))
        c = i % 6
        if c == 1:
            sig[i, 32 + int(rng.integers(0, 31))] ^= bit
        elif c == 2:
            sig[i, int(rng.integers(0, 32))] ^= bit
        elif c == 4:
            pk[i, int(rng.integers(0, 32))] ^= bit
        elif c == 5:
            b = bytearray(msgs[i])
            b[int(rng.integers(0, len(b)))] ^= bit
            msgs[i] = bytes(b)
    edge_at = [5 + 7 * j for j in range(len(S_EDGES))]
    for i, v in zip(edge_at, S_EDGES):
        sig[i, 32:] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)
    with open(os.path.join(ROOT, "tests", "golden", "wide_vectors.json")) as f:
        wide = json.load(f)["ed25519"][:8]
    assert {35, 36} <= {v["windows"] for v in wide}
    for w, v in enumerate(wide):
        i = 16 * (w + 1) + (7 + 3 * w) % 16
        assert i not in edge_at
        pk[i] = np.frombuffer(bytes.fromhex(v["pk"]), np.uint8)
        sig[i] = np.frombuffer(bytes.fromhex(v["sig"]), np.uint8)
        msgs[i] = bytes.fromhex(v["msg"])
    m, off = coracle.pack_msgs(msgs)
    exp = {key: coracle.verify_batch(pk, sig, m, off, mode, nthreads=8) for mode, key in MODES}
    assert 30 < exp["go"].sum() < 110  # honest and rejected ones both
    assert exp["zip215"].sum() > exp["go"].sum()  # the mixed-order wide vectors
    return {"pk": pk, "sig": sig, "msgs": msgs, "exp": exp}


@pytest.fixture(scope="module")
def ctxs():
    from conftest import _env_ctx

    return {"pipe": _env_ctx(CMTV_FORM="quad", CMTV_HS_SUM_PIPE=1),
            "alone": _env_ctx(CMTV_FORM="quad", CMTV_HS_SUM_PIPE=0),
            "pipe-wide": _env_ctx(CMTV_FORM="quad", CMTV_HS_SUM_PIPE=1, CMTV_FORCE_WIDE=1),
            "pipe-ps-late": _env_ctx(CMTV_FORM="quad", CMTV_HS_SUM_PIPE=1, CMTV_FORCE_PS_LATE=1),
            "pipe-pre0": _env_ctx(CMTV_FORM="quad", CMTV_HS_SUM_PIPE=1, CMTV_HS_PRE=0),
            "pipe-pre16": _env_ctx(CMTV_FORM="quad", CMTV_HS_SUM_PIPE=1, CMTV_HS_PRE=16)}


def _workgroups(n):
    # launch_verify's grid: a workgroup per three 16-bit slices of the bitmap words
    return (4 * ((n + 63) // 64) + 2) // 3


def _verify(ctx, pool, n, mode):
    m, off = pack_messages(pool["msgs"][:n])
    got, words = ctx.verify(pool["pk"][:n], pool["sig"][:n], m, off, mode, bitmap=True)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:n]
    assert np.array_equal(bits, got)
    return got


def _counted(ctx, which, n, run):
    """run() under the counters' rules: late_sum_waves never moves,
    late_ps_waves rises by three per workgroup exactly under
    CMTV_FORCE_PS_LATE."""
    before = ctx.stats()
    out = run()
    after = ctx.stats()
    late_sum = after["late_sum_waves"] - before["late_sum_waves"]
    late_ps = after["late_ps_waves"] - before["late_ps_waves"]
    assert late_sum == 0, (which, n, late_sum)
    assert late_ps == (3 * _workgroups(n) if "ps-late" in which else 0), (which, n, late_ps)
    return out


@pytest.mark.parametrize("which", CONTEXTS)
@pytest.mark.parametrize("mode,key", MODES)
@pytest.mark.parametrize("n", SIZES)
def test_sum_pipe_sizes_and_flips(ctxs, pool, n, mode, key, which):
    ctx = ctxs[which]
    got = _counted(ctx, which, n, lambda: _verify(ctx, pool, n, mode))
    exp = pool["exp"][key][:n]
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:20]


@pytest.mark.parametrize("which", CONTEXTS)
@pytest.mark.parametrize("mode,key", MODES)
def test_sum_pipe_small_and_mixed_order_corpus(ctxs, corpus, mode, key, which):
    assert {"small_order_A", "small_order_R", "mixed_order_A", "mixed_order_R"} <= set(corpus["cats"])
    ctx = ctxs[which]
    msg, off = pack_messages(corpus["msgs"])
    n = len(corpus["msgs"])
    got = _counted(ctx, which, n, lambda: ctx.verify(corpus["pk"], corpus["sig"], msg, off, mode))
    bad = np.nonzero(got != corpus[key])[0]
    assert bad.size == 0, [(int(i), corpus["cats"][int(i)]) for i in bad[:10]]
