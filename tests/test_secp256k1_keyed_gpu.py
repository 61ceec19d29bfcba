"""GPU parity for registered-key secp256k1 ECDSA: k_secp_qcomb_build and
k_verify_secp256k1_keyed (cmtv_register_keys_secp256k1,
cmtv_verify_secp256k1_indexed[_device]) against the big-integer oracle
tests/secp256k1_ref.py and against cmtv_verify_secp256k1 on the same bytes,
bit-exact.

The Python oracle is slow, so one module-wide pool of (key index, signature,
message) triples with their verdicts is computed once; every sized batch is
drawn from it.
"""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

from cometbft_amd import Context, Secp256k1KeySet, _native as N, pack_messages

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import secp256k1_keyed_vectors as V  # noqa: E402
import secp256k1_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 300]
POOL = 96
NKEYS = 16


class Pool:
    """POOL triples over NKEYS keys (triple i by key i % NKEYS), message
    lengths from the SHA-256 padding boundaries, about 30% with one flipped
    bit (in r, s or the message), and the oracle's verdict for each."""

    def __init__(self):
        rng = random.Random(2562)
        self.privs = [rng.randbytes(32) for _ in range(NKEYS)]
        self.pks = [S.pubkey_from_priv(p) for p in self.privs]
        self.t = []
        for i in range(POOL):
            k = i % NKEYS
            m = rng.randbytes(LENGTHS[i % len(LENGTHS)])
            sig = S.sign(self.privs[k], m, seed=b"%d" % i)
            if rng.random() < 0.3:
                where = rng.randrange(3 if m else 2)
                bit = 1 << rng.randrange(8)
                if where < 2:
                    sig = bytearray(sig)
                    sig[32 * where + rng.randrange(32)] ^= bit
                else:
                    m = bytearray(m)
                    m[rng.randrange(len(m))] ^= bit
            self.t.append((k, bytes(sig), bytes(m), int(S.verify(self.pks[k], bytes(m), bytes(sig)))))
        self.by_half = [[t for t in self.t if t[0] < 8], [t for t in self.t if t[0] >= 8]]


@pytest.fixture(scope="module")
def pool():
    p = Pool()
    assert {t[3] for t in p.t} == {0, 1}
    return p


@pytest.fixture(scope="module")
def keys(gpu_ctx, pool):
    ks = gpu_ctx.register_secp256k1_keys(key_array(pool.pks))
    yield ks
    ks.free()


def key_array(pks):
    return np.frombuffer(b"".join(pks), np.uint8).reshape(-1, 33).copy()


def arrays(triples):
    idx = np.array([t[0] for t in triples], np.uint32)
    sig = np.frombuffer(b"".join(t[1] for t in triples), np.uint8).reshape(-1, 64).copy()
    m, off = pack_messages([t[2] for t in triples])
    return idx, sig, m, off, np.array([t[3] for t in triples], np.uint8)


def check_bitmap(words, exp):
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")
    assert np.array_equal(bits[: len(exp)], exp)
    assert not bits[len(exp):].any(), "bits at and beyond n must be 0"


def test_corpus_bit_exact(gpu_ctx):
    pks, idx, vecs = V.corpus_indexed()
    assert len(vecs) == 776 and len(pks) == 95
    ks = gpu_ctx.register_secp256k1_keys(key_array(pks))
    try:
        assert len(ks) == 95
        sig = np.array([np.frombuffer(bytes.fromhex(v["sig"]), np.uint8) for v in vecs])
        m, off = pack_messages([bytes.fromhex(v["msg"]) for v in vecs])
        exp = np.array([v["valid"] for v in vecs], np.uint8)
        valid, words = gpu_ctx.verify_secp256k1_indexed(ks, np.array(idx, np.uint32), sig, m, off, bitmap=True)
        bad = np.nonzero(valid != exp)[0]
        assert bad.size == 0, [(vecs[i]["cat"], int(valid[i]), int(exp[i])) for i in bad[:20]]
        assert len(exp) % 64 != 0
        check_bitmap(words, exp)
        generic = gpu_ctx.verify_secp256k1(key_array([pks[i] for i in idx]), sig, m, off)
        assert np.array_equal(valid, generic)
    finally:
        ks.free()


def test_directed_u2(gpu_ctx):
    """u2 = r / s at the comb's digit edges and on both sides of its carry
    row (tests/secp256k1_keyed_vectors.py), each with its flipped twin."""
    vecs = V.directed_vectors()
    assert len(vecs) == 12
    ks = gpu_ctx.register_secp256k1_keys(key_array([v[0] for v in vecs[::2]]))
    try:
        idx, sig, m, off, exp = arrays([(i // 2, v[1], v[2], v[3]) for i, v in enumerate(vecs)])
        assert exp.tolist() == [1, 0] * 6
        valid = gpu_ctx.verify_secp256k1_indexed(ks, idx, sig, m, off)
        assert np.array_equal(valid, exp)
    finally:
        ks.free()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 300])
def test_ragged_sizes_shuffled_keys(gpu_ctx, pool, keys, n):
    """Shuffled, repeated key indices. A batch of one cannot hold both
    verdicts: n = 1 runs one valid and one invalid single-signature batch."""
    rng = random.Random(n)
    if n == 1:
        batches = [[next(t for t in pool.t if t[3] == v)] for v in (1, 0)]
    else:
        batches = [[pool.t[rng.randrange(POOL)] for _ in range(n)]]
    seen = set()
    for b in batches:
        idx, sig, m, off, exp = arrays(b)
        seen |= set(exp.tolist())
        valid, words = gpu_ctx.verify_secp256k1_indexed(keys, idx, sig, m, off, bitmap=True)
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
    """Entries [0, 128) use keys 0-7 only, later ones keys 8-15 only: a key
    index pointer that is not advanced per chunk gives wrong verdicts."""
    rng = random.Random(n)
    picked = [rng.choice(pool.by_half[0 if i < 128 else 1]) for i in range(n)]
    idx, sig, m, off, exp = arrays(picked)
    assert idx[:128].max() < 8 and idx[128:].min() >= 8 and set(exp.tolist()) == {0, 1}
    ks = chunk_ctx.register_secp256k1_keys(key_array(pool.pks))
    try:
        before = chunk_ctx.stats()
        valid, words = chunk_ctx.verify_secp256k1_indexed(ks, idx, sig, m, off, bitmap=True)
        after = chunk_ctx.stats()
    finally:
        ks.free()
    assert np.array_equal(valid, exp), np.nonzero(valid != exp)[0][:10]
    check_bitmap(words, exp)
    assert after["kernel_launches"] - before["kernel_launches"] == (n + 127) // 128
    assert after["keyed_launches"] - before["keyed_launches"] == (n + 127) // 128
    assert after["signatures"] - before["signatures"] == n
    assert after["invalid"] - before["invalid"] == int((exp == 0).sum())


def test_rejected_keys_in_a_set(gpu_ctx, pool):
    """Rejected keys first, in the middle and last of a 9-key set: the set
    registers, their signatures are 0, the neighbours' verdicts unchanged."""
    off_curve = next(x for x in range(1, 100) if S.lift_x(x, 0) is None)
    bad = [bytes([5]) + pool.pks[0][1:], bytes([2]) + S.P.to_bytes(32, "big"),
           bytes([3]) + off_curve.to_bytes(32, "big")]
    pks = [bad[0]] + pool.pks[1:4] + [bad[1]] + pool.pks[5:8] + [bad[2]]
    assert len(pks) == 9
    ks = gpu_ctx.register_secp256k1_keys(key_array(pks))
    try:
        assert len(ks) == 9
        triples = [t for t in pool.t if t[0] < 9]
        idx, sig, m, off, exp = arrays(triples)
        rejected = np.isin(idx, [0, 4, 8])
        assert rejected.any() and exp[rejected].any() and exp[~rejected].any()
        exp = np.where(rejected, 0, exp).astype(np.uint8)
        valid = gpu_ctx.verify_secp256k1_indexed(ks, idx, sig, m, off)
        assert np.array_equal(valid, exp)
        generic = gpu_ctx.verify_secp256k1(key_array([pks[i] for i in idx]), sig, m, off)
        assert np.array_equal(valid, generic)
    finally:
        ks.free()


def test_same_x_both_parities(gpu_ctx, pool):
    """Keys 02 || x and 03 || x: a signature valid under one is invalid under
    the other."""
    k, sig, msg, _ = next(t for t in pool.t if t[3] == 1)
    pk = pool.pks[k]
    twin = bytes([pk[0] ^ 1]) + pk[1:]
    ks = gpu_ctx.register_secp256k1_keys(key_array([pk, twin]))
    try:
        idx, sigs, m, off, _ = arrays([(0, sig, msg, 1), (1, sig, msg, 0)])
        assert gpu_ctx.verify_secp256k1_indexed(ks, idx, sigs, m, off).tolist() == [1, 0]
        assert not S.verify(twin, msg, sig)
    finally:
        ks.free()


def test_device_entry_point(gpu_ctx, pool, keys):
    """A non-null stream; only d_bitmap, then only d_valid; key indices equal
    to n_keys and to 0xFFFFFFFF give verdict 0 and change no other entry."""
    import torch

    n = 300
    rng = random.Random(300)
    idx, sig, m, off, exp = arrays([pool.t[rng.randrange(POOL)] for _ in range(n)])
    host = gpu_ctx.verify_secp256k1_indexed(keys, idx, sig, m, off)
    assert np.array_equal(host, exp) and set(exp.tolist()) == {0, 1}
    out_of_range = {int(np.nonzero(exp == 1)[0][0]): NKEYS, int(np.nonzero(exp == 1)[0][-1]): 0xFFFFFFFF}
    bad_idx = idx.copy()
    for i, k in out_of_range.items():
        bad_idx[i] = k
    bad_exp = exp.copy()
    bad_exp[list(out_of_range)] = 0
    dev = torch.device("cuda:0")
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         {"idx": idx.view(np.int32), "bad": bad_idx.view(np.int32), "sig": sig.reshape(-1), "m": m,
          "off": off.view(np.int32)}.items()}
    stream = torch.cuda.Stream(device=dev)
    assert stream.cuda_stream != 0
    stream.wait_stream(torch.cuda.current_stream())
    for which, want in (("idx", exp), ("bad", bad_exp)):
        d_valid = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        d_words = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device=dev)
        stream.wait_stream(torch.cuda.current_stream())
        args = (keys, n, d[which].data_ptr(), d["sig"].data_ptr(), d["m"].data_ptr(), d["off"].data_ptr())
        gpu_ctx.verify_secp256k1_indexed_device(*args, 0, d_words.data_ptr(), stream.cuda_stream)  # only d_bitmap
        gpu_ctx.verify_secp256k1_indexed_device(*args, d_valid.data_ptr(), 0, stream.cuda_stream)  # only d_valid
        stream.synchronize()
        assert np.array_equal(d_valid.cpu().numpy(), want), which
        check_bitmap(d_words.cpu().numpy().view(np.uint64), want)
    # the host entry point refuses the same indices before anything is launched
    before = gpu_ctx.stats()
    with pytest.raises(N.CmtvError) as ei:
        gpu_ctx.verify_secp256k1_indexed(keys, bad_idx, sig, m, off)
    assert ei.value.code == N.CMTV_EINVAL
    after = gpu_ctx.stats()
    assert after["kernel_launches"] == before["kernel_launches"] and after["calls"] == before["calls"]


def test_two_key_sets(gpu_ctx, pool):
    """Two sets alive at once (the second with the keys in reverse order);
    the first freed, the second still gives the right verdicts."""
    a = gpu_ctx.register_secp256k1_keys(key_array(pool.pks))
    b = gpu_ctx.register_secp256k1_keys(key_array(pool.pks[::-1]))
    try:
        idx, sig, m, off, exp = arrays(pool.t[:70])
        assert np.array_equal(gpu_ctx.verify_secp256k1_indexed(a, idx, sig, m, off), exp)
        assert np.array_equal(gpu_ctx.verify_secp256k1_indexed(b, NKEYS - 1 - idx, sig, m, off), exp)
        a.free()
        assert np.array_equal(gpu_ctx.verify_secp256k1_indexed(b, NKEYS - 1 - idx, sig, m, off), exp)
    finally:
        a.free()
        b.free()


def test_argument_errors(gpu_ctx, pool, keys):
    idx, sig, m, off, _ = arrays(pool.t[:4])
    L = N.lib()
    u8p, u32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32)
    valid = np.zeros(4, np.uint8)
    good = dict(ctx=gpu_ctx.handle, ks=keys.handle, idx=idx.ctypes.data_as(u32p), sig=sig.ctypes.data_as(u8p),
                msg=m.ctypes.data_as(u8p), off=off.ctypes.data_as(u32p), valid=valid.ctypes.data_as(u8p), words=None)
    before = gpu_ctx.stats()

    def host(n=4, **kw):
        a = {**good, **kw}
        return L.cmtv_verify_secp256k1_indexed(a["ctx"], a["ks"], n, a["idx"], a["sig"], a["msg"], a["off"],
                                               a["valid"], a["words"])

    def device(n=4, **kw):
        a = {"ctx": gpu_ctx.handle, "ks": keys.handle, "idx": 16, "sig": 16, "msg": 16, "off": 16, "valid": 16,
             "words": None, **kw}
        return L.cmtv_verify_secp256k1_indexed_device(a["ctx"], a["ks"], n, a["idx"], a["sig"], a["msg"], a["off"],
                                                      a["valid"], a["words"], None)

    other = Context(device=0)
    try:
        for call in (host, device):
            assert call(ks=None) == N.CMTV_EINVAL
            assert call(ctx=other.handle) == N.CMTV_EINVAL  # the set belongs to gpu_ctx
            assert call(ctx=None) == N.CMTV_EINVAL
            assert call(valid=None) == N.CMTV_EINVAL  # neither output
            for name in ("idx", "sig", "off"):
                assert call(**{name: None}) == N.CMTV_EINVAL, name
            assert call(n=0, idx=None, sig=None, msg=None, off=None, valid=None) == N.CMTV_OK
    finally:
        other.close()
    assert host(msg=None) == N.CMTV_EINVAL  # msg_off[n] != 0
    assert device(msg=None) == N.CMTV_EINVAL
    dec = off.copy()
    dec[1] = max(int(dec[1]), 1)
    dec[2] = dec[1] - 1
    assert host(off=dec.ctypes.data_as(u32p)) == N.CMTV_EINVAL
    # registration
    pk = key_array(pool.pks[:2])
    h = ctypes.c_void_p()
    reg = L.cmtv_register_keys_secp256k1
    assert reg(gpu_ctx.handle, 0, pk.ctypes.data_as(u8p), ctypes.byref(h)) == N.CMTV_EINVAL and not h
    assert reg(gpu_ctx.handle, 65537, pk.ctypes.data_as(u8p), ctypes.byref(h)) == N.CMTV_EINVAL and not h
    assert reg(gpu_ctx.handle, 2, None, ctypes.byref(h)) == N.CMTV_EINVAL and not h
    assert reg(gpu_ctx.handle, 2, pk.ctypes.data_as(u8p), None) == N.CMTV_EINVAL
    assert reg(None, 2, pk.ctypes.data_as(u8p), ctypes.byref(h)) == N.CMTV_EINVAL and not h
    L.cmtv_secp_keyset_free(None)
    assert L.cmtv_secp_keyset_len(None) == 0
    after = gpu_ctx.stats()
    assert after["kernel_launches"] == before["kernel_launches"] and after["calls"] == before["calls"]


def test_python_classes_round_trip(gpu_ctx, pool):
    ks = gpu_ctx.register_secp256k1_keys(key_array(pool.pks[:3]))
    assert isinstance(ks, Secp256k1KeySet) and len(ks) == 3 and ks.handle
    assert ks.pk.shape == (3, 33) and ks.pk.tobytes() == b"".join(pool.pks[:3])
    idx, sig, m, off, exp = arrays([t for t in pool.t if t[0] < 3])
    valid, words = gpu_ctx.verify_secp256k1_indexed(ks, idx, sig, m, off, bitmap=True)
    assert np.array_equal(valid, exp)
    check_bitmap(words, exp)
    with pytest.raises(ValueError):
        gpu_ctx.verify_secp256k1_indexed(ks, idx[:-1], sig, m, off)
    ks.free()
    assert ks.handle is None
    ks.free()  # twice is fine
    with pytest.raises(N.CmtvError):
        gpu_ctx.register_secp256k1_keys(np.zeros((0, 33), np.uint8))
