"""The serial carry chain of fe_mul / fe_sq (fe25519.h) on the device, end to
end: every Ed25519 form (CMTV_FORM) in both verdict modes and sr25519, against
liboracle, at n = 1, 47, 49 and 97 signatures -- one quad wave, one quad
workgroup (48 signatures) minus one, one plus one, two plus one.

30% of the signatures carry one flipped bit (in R, s or A), and the 35- and
36-window vectors of tests/golden/wide_vectors.json sit among them (two of
them inside the first 47, both window counts). One forced-wide run
(CMTV_FORCE_WIDE=1) and one CMTV_FORCE_PS_LATE=1 run at n = 49.

tests/test_fe_reduce.py checks the same functions' limbs against integers
on the host; tests/test_device_primitives_gpu.py their device lowering."""
import json
import os

import numpy as np
import pytest

from oracle import coracle
from cometbft_amd import MODE_GO_STDLIB, MODE_ZIP215, pack_messages

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 47, 49, 97]
MODES = [(MODE_GO_STDLIB, "go"), (MODE_ZIP215, "zip215")]
ED_FORMS = ["row4", "row", "oct2", "quad", "lane"]
WIDE_AT = [5, 30, 48, 52, 70, 96]


@pytest.fixture(scope="module")
def pool():
    """97 signatures and the oracle's verdicts, computed once"""
    rng = np.random.default_rng(808)
    n = 97
    seeds = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    msgs = [rng.integers(0, 256, 60 + i % 70, dtype=np.uint8).tobytes() for i in range(n)]
    m, off = coracle.pack_msgs(msgs)
    sig = coracle.sign_batch(seeds, m, off, nthreads=8).copy()
    pk = coracle.pubkeys_from_seeds(seeds).copy()
    flip = rng.random(n) < 0.3
    flip[0] = False  # n = 1 is an honest signature
    for i in np.nonzero(flip)[0]:
        bit = np.uint8(1 << int(rng.integers(0, 8)))
        where = int(rng.integers(0, 3))
        if where == 2:
            pk[i, int(rng.integers(0, 32))] ^= bit
        else:
            sig[i, 32 * where + int(rng.integers(0, 31))] ^= bit
    with open(os.path.join(ROOT, "tests", "golden", "wide_vectors.json")) as f:
        wide = json.load(f)["ed25519"]
    by_windows = {w: [v for v in wide if v["windows"] == w] for w in (35, 36)}
    assert by_windows[35] and by_windows[36]
    for k, i in enumerate(WIDE_AT):
        v = by_windows[35 + (k & 1)][(k // 2) % len(by_windows[35 + (k & 1)])]
        pk[i] = np.frombuffer(bytes.fromhex(v["pk"]), np.uint8)
        sig[i] = np.frombuffer(bytes.fromhex(v["sig"]), np.uint8)
        msgs[i] = bytes.fromhex(v["msg"])
        flip[i] = False
    m, off = coracle.pack_msgs(msgs)
    exp = {key: coracle.verify_batch(pk, sig, m, off, mode, nthreads=8) for mode, key in MODES}
    plain = np.ones(n, bool)
    plain[WIDE_AT] = False
    for key in exp:  # honest ones pass, and most flipped ones do not
        assert exp[key][plain & ~flip].all() and exp[key][flip].sum() < flip.sum() / 2
    assert 20 <= flip.sum() <= 40
    return {"pk": pk, "sig": sig, "msgs": msgs, "exp": exp}


def _check(ctx, pool, n, mode, key):
    m, off = pack_messages(pool["msgs"][:n])
    got = ctx.verify(pool["pk"][:n], pool["sig"][:n], m, off, mode)
    exp = pool["exp"][key][:n]
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:20]


@pytest.mark.parametrize("form", ED_FORMS)
@pytest.mark.parametrize("mode,key", MODES)
@pytest.mark.parametrize("n", SIZES)
def test_every_form_matches_the_oracle(form_ctx, pool, n, mode, key, form):
    _check(form_ctx(form), pool, n, mode, key)


@pytest.fixture(scope="module")
def knob_ctxs():
    """one context per test knob, closed when the module is done: an open
    context keeps its streams, and their hardware queues, for the rest of
    the session (tests/test_row_ring_gpu.py needs four queues of its own)"""
    from conftest import _env_ctx

    made = {knob: _env_ctx(CMTV_FORM="quad", **{knob: 1}) for knob in ("CMTV_FORCE_WIDE", "CMTV_FORCE_PS_LATE")}
    yield made
    for ctx in made.values():
        ctx.close()


@pytest.mark.parametrize("knob", ["CMTV_FORCE_WIDE", "CMTV_FORCE_PS_LATE"])
@pytest.mark.parametrize("mode,key", MODES)
def test_forced_wide_and_late_ps(knob_ctxs, pool, mode, key, knob):
    _check(knob_ctxs[knob], pool, 49, mode, key)


@pytest.mark.parametrize("form", ["quad", "lane"])
def test_sr25519_matches_the_oracle(form_ctx, form):
    n = 49
    rng = np.random.default_rng(809)
    minis = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    msgs = [rng.integers(0, 256, int(l), dtype=np.uint8).tobytes() for l in rng.integers(0, 200, n)]
    m, off = coracle.pack_msgs(msgs)
    sig = coracle.sr25519_sign_batch(minis, m, off).copy()
    pk = coracle.sr25519_pubkeys(minis).copy()
    flip = np.nonzero(rng.random(n) < 0.3)[0]
    sig[flip, rng.integers(0, 63, flip.size)] ^= (1 << rng.integers(0, 8, flip.size)).astype(np.uint8)
    exp = coracle.sr25519_verify_batch(pk, sig, m, off, nthreads=8)
    assert 0 < (exp == 0).sum() < n
    got = form_ctx(form).verify_sr25519(pk, sig, m, off)
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:20]
