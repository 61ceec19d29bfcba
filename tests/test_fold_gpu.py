"""GPU parity of k_verify_quad_hs_fold, the Ed25519 quad form with [s]B folded
into R: a comb wave computes P_s = [s]B from s alone and hands it to the quads
through an LDS flag; X = [k1](-A) + [k2](P_s - R) (cometbft_amd/csrc/quad.h
q_verify_hs_fold, kernels.hip). Verdicts are compared with the C oracle bit
for bit, in both modes:

 - sizes 1, 16, 17, 47, 48, 49, 97, 145: one quad, the wave (16) and
   workgroup (48) boundaries on both sides, a ragged last workgroup;
 - honest signatures and single-bit flips in s, R, A and the message;
 - s at the comb's edges: 0, 1, L - 1, L, L + 1, 2^252 and the radix-2^16
   digits 0x7FFF / 0x8000 / 0xFFFF (the signed recoding) in the low, a middle
   and the top position;
 - the small-order and mixed-order corpus;
 - the 35- and 36-window vectors, each at another lane of its wave;
 - the forced 64-window fallback (CMTV_FORCE_WIDE);
 - all of it once more with CMTV_FORCE_PS_LATE=1, where no quad wave waits for
   the comb wave and each adds the comb rows itself, and counts itself in
   cmtv_stats.late_ps_waves: the wait never decides a verdict.
The CPU side of the same code is tests/test_fold_host.py.
Reference semantics: crypto/ed25519/ed25519.go:148-155 (Go 1.19 Verify)."""
import json
import os

import numpy as np
import pytest

from oracle import coracle
from cometbft_amd import MODE_GO_STDLIB, MODE_ZIP215, pack_messages

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 2**252 + 27742317777372353535851937790883648493
SIZES = [1, 16, 17, 47, 48, 49, 97, 145]
MODES = [(MODE_GO_STDLIB, "go"), (MODE_ZIP215, "zip215")]


def _s_edges():
    vals = [0, 1, L - 1, L, L + 1, 2**252]
    for d in (0x7FFF, 0x8000, 0xFFFF):
        for pos in (0, 7, 15):
            vals.append(d << (16 * pos))
    return vals


@pytest.fixture(scope="module")
def pool():
    """145 signatures, the oracle's verdicts computed once. Entry i is honest
    (i % 6 in 0, 5) or carries one flipped bit in s (1), R (2), A (3) or the
    message (4); the s edge values replace s at entries 2, 11, 20, ... (the
    first two inside the first wave); the wide vectors sit at lane
    (3 + 5 w) % 16 of wave w + 1."""
    rng = np.random.default_rng(29)
    n = 145
    seeds = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    msgs = [rng.integers(0, 256, 90 + i % 40, dtype=np.uint8).tobytes() for i in range(n)]
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
        elif c == 3:
            pk[i, int(rng.integers(0, 32))] ^= bit
        elif c == 4:
            b = bytearray(msgs[i])
            b[int(rng.integers(0, len(b)))] ^= bit
            msgs[i] = bytes(b)
    edge_at = [2 + 9 * j for j in range(len(_s_edges()))]
    for i, v in zip(edge_at, _s_edges()):
        sig[i, 32:] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)
    with open(os.path.join(ROOT, "tests", "golden", "wide_vectors.json")) as f:
        wide = json.load(f)["ed25519"]
    wide = wide[:8]
    assert {35, 36} <= {v["windows"] for v in wide}
    for w, v in enumerate(wide):
        i = 16 * (w + 1) + (3 + 5 * w) % 16
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
def ctxs(form_ctx):
    from conftest import _env_ctx

    return {"fold": form_ctx("quad"),
            "late": _env_ctx(CMTV_FORM="quad", CMTV_FORCE_PS_LATE=1),
            "wide": _env_ctx(CMTV_FORM="quad", CMTV_FORCE_WIDE=1),
            "wide-late": _env_ctx(CMTV_FORM="quad", CMTV_FORCE_WIDE=1, CMTV_FORCE_PS_LATE=1)}


def _verify(ctx, pool, n, mode):
    m, off = pack_messages(pool["msgs"][:n])
    got, words = ctx.verify(pool["pk"][:n], pool["sig"][:n], m, off, mode, bitmap=True)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:n]
    assert np.array_equal(bits, got)
    return got


@pytest.mark.parametrize("which", ["fold", "late"])
@pytest.mark.parametrize("mode,key", MODES)
@pytest.mark.parametrize("n", SIZES)
def test_fold_sizes_flips_and_s_edges(ctxs, pool, n, mode, key, which):
    ctx = ctxs[which]
    late0 = ctx.stats()["late_ps_waves"]
    got = _verify(ctx, pool, n, mode)
    exp = pool["exp"][key][:n]
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:20]
    late = ctx.stats()["late_ps_waves"] - late0
    if which == "late":
        # every quad wave of every workgroup, idle ones of the last included
        assert late == 3 * ((4 * ((n + 63) // 64) + 2) // 3)
    else:
        assert late == 0


@pytest.mark.parametrize("which", ["wide", "wide-late"])
@pytest.mark.parametrize("mode,key", MODES)
def test_fold_forced_wide(ctxs, pool, corpus, mode, key, which):
    ctx = ctxs[which]
    got = _verify(ctx, pool, 145, mode)
    assert np.array_equal(got, pool["exp"][key]), np.nonzero(got != pool["exp"][key])[0][:20]
    msg, off = pack_messages(corpus["msgs"])
    got = ctx.verify(corpus["pk"], corpus["sig"], msg, off, mode)
    assert np.array_equal(got, corpus[key]), np.nonzero(got != corpus[key])[0][:10]


@pytest.mark.parametrize("which", ["fold", "late"])
@pytest.mark.parametrize("mode,key", MODES)
def test_fold_small_and_mixed_order_corpus(ctxs, corpus, mode, key, which):
    assert {"small_order_A", "small_order_R", "mixed_order_A", "mixed_order_R"} <= set(corpus["cats"])
    msg, off = pack_messages(corpus["msgs"])
    got = ctxs[which].verify(corpus["pk"], corpus["sig"], msg, off, mode)
    bad = np.nonzero(got != corpus[key])[0]
    assert bad.size == 0, [(int(i), corpus["cats"][int(i)]) for i in bad[:10]]


def test_fold_is_the_quad_form_and_the_old_kernel_agrees(pool):
    """CMTV_HS_FOLD=0 keeps k_verify_quad_hs: the same verdicts, and no quad
    wave of it ever counts as late."""
    from conftest import _env_ctx

    ctx = _env_ctx(CMTV_FORM="quad", CMTV_HS_FOLD=0, CMTV_FORCE_PS_LATE=1)
    for mode, key in MODES:
        assert np.array_equal(_verify(ctx, pool, 145, mode), pool["exp"][key])
    assert ctx.stats()["late_ps_waves"] == 0
