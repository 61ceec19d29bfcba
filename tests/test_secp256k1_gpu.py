"""GPU parity for secp256k1 ECDSA: libcmtverify's k_verify_secp256k1 verdicts
vs the big-integer oracle tests/secp256k1_ref.py (the restatement of
crypto/secp256k1/secp256k1.go:192-217), bit-exact.

The Python oracle is slow, so one module-wide pool of (key, signature,
message) triples with their verdicts is computed once; every sized batch is
drawn from it.
"""
import ctypes
import json
import os
import random
import sys

import numpy as np
import pytest

from cometbft_amd import Context, Secp256k1BatchVerifier, Secp256k1PubKey, _native as N, pack_messages

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import secp256k1_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 300]
POOL = 320


@pytest.fixture(scope="module")
def corpus():
    with open(os.path.join(ROOT, "tests", "golden", "secp256k1_corpus.json")) as f:
        return json.load(f)["vectors"]


def build_pool():
    """POOL triples over 16 keys, message lengths from the SHA-256 padding
    boundaries, about 30% with one flipped bit (in r, s, the message or the
    key's x), and the oracle's verdict for each."""
    rng = random.Random(2561)
    privs = [rng.randbytes(32) for _ in range(16)]
    pks = [S.pubkey_from_priv(p) for p in privs]
    out = []
    for i in range(POOL):
        k = i % len(privs)
        m = rng.randbytes(LENGTHS[rng.randrange(len(LENGTHS))])
        pk, sig = pks[k], S.sign(privs[k], m, seed=b"%d" % i)
        if rng.random() < 0.3:
            where = rng.randrange(4 if m else 3)
            bit = 1 << rng.randrange(8)
            if where < 2:
                sig = bytearray(sig)
                sig[32 * where + rng.randrange(32)] ^= bit
            elif where == 2:
                pk = bytearray(pk)
                pk[1 + rng.randrange(32)] ^= bit
            else:
                m = bytearray(m)
                m[rng.randrange(len(m))] ^= bit
        out.append((bytes(pk), bytes(sig), bytes(m), int(S.verify(bytes(pk), bytes(m), bytes(sig)))))
    return out


@pytest.fixture(scope="module")
def pool():
    return build_pool()


def arrays(triples):
    pk = np.frombuffer(b"".join(t[0] for t in triples), np.uint8).reshape(-1, 33).copy()
    sig = np.frombuffer(b"".join(t[1] for t in triples), np.uint8).reshape(-1, 64).copy()
    m, off = pack_messages([t[2] for t in triples])
    return pk, sig, m, off, np.array([t[3] for t in triples], np.uint8)


def check_bitmap(words, exp):
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")
    assert np.array_equal(bits[: len(exp)], exp)
    assert not bits[len(exp):].any(), "bits at and beyond n must be 0"


def test_corpus_bit_exact(gpu_ctx, corpus):
    pk = np.array([np.frombuffer(bytes.fromhex(v["pk"]), np.uint8) for v in corpus])
    sig = np.array([np.frombuffer(bytes.fromhex(v["sig"]), np.uint8) for v in corpus])
    m, off = pack_messages([bytes.fromhex(v["msg"]) for v in corpus])
    exp = np.array([v["valid"] for v in corpus], np.uint8)
    valid, words = gpu_ctx.verify_secp256k1(pk, sig, m, off, bitmap=True)
    bad = np.nonzero(valid != exp)[0]
    assert bad.size == 0, [(corpus[i]["cat"], int(valid[i]), int(exp[i])) for i in bad[:20]]
    assert len(exp) % 64 != 0
    check_bitmap(words, exp)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 300])
def test_ragged_sizes_honest_and_flipped(gpu_ctx, pool, n):
    """A batch of one cannot hold both verdicts: n = 1 runs one valid and one
    invalid single-signature batch."""
    starts = [next(i for i, t in enumerate(pool) if t[3] == v) for v in (1, 0)] if n == 1 else [7]
    seen = set()
    for a in starts:
        pk, sig, m, off, exp = arrays(pool[a: a + n])
        assert len(exp) == n
        seen |= set(exp.tolist())
        valid, words = gpu_ctx.verify_secp256k1(pk, sig, m, off, bitmap=True)
        assert np.array_equal(valid, exp), np.nonzero(valid != exp)[0][:10]
        check_bitmap(words, exp)
    assert seen == {0, 1}


@pytest.fixture(scope="module")
def chunk_ctx():
    """A context whose lane launches take at most 128 signatures."""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    old = os.environ.get("CMTV_LANE_CHUNK")
    os.environ["CMTV_LANE_CHUNK"] = "128"
    try:
        return Context(device=0)
    finally:
        if old is None:
            del os.environ["CMTV_LANE_CHUNK"]
        else:
            os.environ["CMTV_LANE_CHUNK"] = old


@pytest.mark.parametrize("n", [129, 1000])
def test_launch_chunking(chunk_ctx, pool, n):
    rng = random.Random(n)
    idx = [rng.randrange(len(pool)) for _ in range(n)]
    pk, sig, m, off, exp = arrays([pool[i] for i in idx])
    assert set(exp.tolist()) == {0, 1}
    before = chunk_ctx.stats()
    valid, words = chunk_ctx.verify_secp256k1(pk, sig, m, off, bitmap=True)
    after = chunk_ctx.stats()
    assert np.array_equal(valid, exp), np.nonzero(valid != exp)[0][:10]
    check_bitmap(words, exp)
    assert after["kernel_launches"] - before["kernel_launches"] == (n + 127) // 128
    assert after["signatures"] - before["signatures"] == n
    assert after["invalid"] - before["invalid"] == int((exp == 0).sum())


def test_device_buffers_match_host_path(gpu_ctx, pool):
    import torch

    n = 300
    pk, sig, m, off, exp = arrays(pool[:n])
    host = gpu_ctx.verify_secp256k1(pk, sig, m, off)
    assert np.array_equal(host, exp) and set(exp.tolist()) == {0, 1}
    dev = torch.device("cuda:0")
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         {"pk": pk.reshape(-1), "sig": sig.reshape(-1), "m": m, "off": off.view(np.int32)}.items()}
    stream = torch.cuda.Stream(device=dev)
    assert stream.cuda_stream != 0
    d_valid = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    d_words = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    args = (n, d["pk"].data_ptr(), d["sig"].data_ptr(), d["m"].data_ptr(), d["off"].data_ptr())
    gpu_ctx.verify_secp256k1_device(*args, 0, d_words.data_ptr(), stream.cuda_stream)  # only d_bitmap
    gpu_ctx.verify_secp256k1_device(*args, d_valid.data_ptr(), 0, stream.cuda_stream)  # only d_valid
    stream.synchronize()
    assert np.array_equal(d_valid.cpu().numpy(), host)
    check_bitmap(d_words.cpu().numpy().view(np.uint64), host)


def test_pubkey_and_batch_mirror(gpu_ctx, pool):
    with open(os.path.join(ROOT, "tests", "golden", "secp256k1_kat.json")) as f:
        kat = json.load(f)["key"]
    assert Secp256k1PubKey(bytes.fromhex(kat["pub"])).address().hex() == kat["address"]
    good = next(t for t in pool if t[3] == 1)
    bad = next(t for t in pool if t[3] == 0)
    k = Secp256k1PubKey(good[0])
    assert k.verify_signature(good[2], good[1], ctx=gpu_ctx)
    assert not k.verify_signature(good[2] + b"x", good[1], ctx=gpu_ctx)
    assert not k.verify_signature(good[2], good[1][:63], ctx=gpu_ctx)
    assert not k.verify_signature(good[2], good[1] + b"\0", ctx=gpu_ctx)
    for wrong in (good[0][:32], good[0] + b"\0"):
        with pytest.raises(ValueError):
            Secp256k1PubKey(wrong).verify_signature(good[2], good[1], ctx=gpu_ctx)
        with pytest.raises(ValueError):
            Secp256k1PubKey(wrong).address()
    bv = Secp256k1BatchVerifier(gpu_ctx)
    assert bv.verify() == (True, [])
    bv.add(good[0], good[2], good[1])
    bv.add(bad[0], bad[2], bad[1])
    bv.add(good[0], good[2], good[1][:10])
    bv.add(good[0], good[2], good[1])
    assert len(bv) == 4
    ok, res = bv.verify()
    assert not ok and res == [True, False, False, True]
    with pytest.raises(ValueError):
        bv.add(good[0][:32], good[2], good[1])
    bv.reset()
    bv.add(good[0], good[2], good[1])
    assert bv.verify() == (True, [True])


def test_stats_advance(gpu_ctx, pool):
    pk, sig, m, off, exp = arrays(pool[:70])
    before = gpu_ctx.stats()
    gpu_ctx.verify_secp256k1(pk, sig, m, off)
    after = gpu_ctx.stats()
    assert after["signatures"] - before["signatures"] == 70
    assert after["kernel_launches"] - before["kernel_launches"] == 1
    assert after["calls"] - before["calls"] == 1
    assert after["invalid"] - before["invalid"] == int((exp == 0).sum())


def test_argument_errors(gpu_ctx, pool):
    pk, sig, m, off, _ = arrays(pool[:4])
    L = N.lib()
    u8p, u32p, u64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    valid = np.zeros(4, np.uint8)
    good = dict(pk=pk.ctypes.data_as(u8p), sig=sig.ctypes.data_as(u8p), msg=m.ctypes.data_as(u8p),
                off=off.ctypes.data_as(u32p), valid=valid.ctypes.data_as(u8p), words=None)
    before = gpu_ctx.stats()

    def host(**kw):
        a = {**good, **kw}
        return L.cmtv_verify_secp256k1(gpu_ctx.handle, 4, a["pk"], a["sig"], a["msg"], a["off"], a["valid"],
                                       a["words"])

    assert host(pk=None) == N.CMTV_EINVAL
    assert host(sig=None) == N.CMTV_EINVAL
    assert host(off=None) == N.CMTV_EINVAL
    assert host(msg=None) == N.CMTV_EINVAL  # msg_off[n] != 0
    assert host(valid=None) == N.CMTV_EINVAL  # neither output
    dec = off.copy()
    dec[1] = max(int(dec[1]), 1)
    dec[2] = dec[1] - 1
    assert host(off=dec.ctypes.data_as(u32p)) == N.CMTV_EINVAL
    assert L.cmtv_verify_secp256k1(None, 4, good["pk"], good["sig"], good["msg"], good["off"], good["valid"],
                                   None) == N.CMTV_EINVAL
    assert L.cmtv_verify_secp256k1(gpu_ctx.handle, 0, None, None, None, None, None, None) == N.CMTV_OK
    dev = [L.cmtv_verify_secp256k1_device(gpu_ctx.handle, 4, *[None if j == i else 16 for j in range(4)], 16, None,
                                          None) for i in range(4)]
    assert dev == [N.CMTV_EINVAL] * 4
    assert L.cmtv_verify_secp256k1_device(gpu_ctx.handle, 4, 16, 16, 16, 16, None, None, None) == N.CMTV_EINVAL
    after = gpu_ctx.stats()
    assert after["kernel_launches"] == before["kernel_launches"] and after["calls"] == before["calls"]
