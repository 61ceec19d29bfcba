"""CPU tests of the header additions to the C ABI: the host leaf encoder
cmtv_header_leaf_bytes against tests/header_ref.py and the reference's
known-answer leaves, its cap rule with a canary, the rule that a header has no
hash (as far as it shows without a device), that the new symbols are bound, and
that the addition left the ABI version and cmtv_stats alone. (The calls that
take a context are in tests/test_header_gpu.py: they need an open one.)"""
import ctypes
import itertools
import json
import os
import random
import sys

from cometbft_amd import _native as N
from cometbft_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import header_ref as H  # noqa: E402
import merkle_ref as R  # noqa: E402
from header_util import U64, CHeader, as_int64, gen_header  # noqa: E402

CANARY = 0xA5
VARINTS = [0, 1, 127, 128, 2**63 - 1, -1, 2**64 - 1]


def leaf_bytes(ch, leaf, cap=2048):
    out = (ctypes.c_uint8 * max(cap, 1))(*([CANARY] * max(cap, 1)))
    n = N.lib().cmtv_header_leaf_bytes(ctypes.byref(ch.c), leaf, out, cap)
    return n, bytes(out)


def all_leaves(h, align=0):
    ch = CHeader(h, align)
    got = []
    for leaf in range(14):
        n, out = leaf_bytes(ch, leaf)
        assert n >= 0 and set(out[n:]) <= {CANARY}, (leaf, n)
        got.append(out[:n])
    return got


def test_new_symbols_are_bound():
    lib = N.lib()
    for name in ("cmtv_header_hash", "cmtv_header_hashes", "cmtv_header_leaf_bytes", "cmtv_txs_hash", "cmtv_txs_hashes"):
        assert name in N.EXPORTS and getattr(lib, name).argtypes is not None, name
    assert N.HDR_N_BYTES_FIELDS == 9 == len(H.BYTES_FIELDS)
    with open(os.path.join(ROOT, "include", "cmtverify.h")) as f:
        src = f.read()
    for name in ("cmtv_header_hash", "cmtv_header_hashes", "cmtv_header_leaf_bytes", "cmtv_txs_hash", "cmtv_txs_hashes",
                 "CMTV_HDR_PROPOSER_ADDRESS"):
        assert name in src, name


def test_leaf_bytes_reproduce_the_known_answer_leaves():
    with open(os.path.join(ROOT, "tests", "golden", "merkle_kat.json")) as f:
        kat = json.load(f)["header_hash"]
    got = all_leaves(H.kat_header())
    assert [g.hex() for g in got] == kat["leaves"]
    assert R.root(got) == bytes.fromhex(kat["root"])


def test_leaf_bytes_match_the_restatement():
    rng = random.Random(71)
    hs = [gen_header(rng) for _ in range(20)]
    for n in (0, 1, 20, 32, 52, 53, 64, 65, 200, 1000):
        hs.append(gen_header(rng, chain_id=rng.randbytes(n), app_hash=rng.randbytes(n), data_hash=rng.randbytes(n),
                             proposer_address=rng.randbytes(n)))
    for a, b in itertools.product(VARINTS, VARINTS):
        hs.append(gen_header(rng, version_block=a & U64, version_app=b & U64, height=as_int64(a)))
    for s in (0, R.GO_ZERO_TIME_SECONDS, 2**31, R.LAST_VALID_SECOND):
        for ns in (0, 1, 999_999_999):
            hs.append(gen_header(rng, seconds=s, nanos=ns))
    for hl, total, pl in itertools.product((0, 1, 31, 32, 33, 100), (0, 1, 2**32 - 1), (0, 1, 31, 32, 33)):
        hs.append(gen_header(rng, id_hash=rng.randbytes(hl), id_total=total, id_part_hash=rng.randbytes(pl)))
    hs.append(H.Hdr())  # every item empty but the block id's part-set header
    for i, h in enumerate(hs):
        assert all_leaves(h, align=i % 4) == H.leaves(h), h
    assert all_leaves(H.Hdr())[4] == b"\x12\x00"


def test_python_header_packs_the_same_struct():
    h = H.kat_header()
    t = T.Header(h.version_block, h.version_app, h.chain_id.decode(), h.height, (h.seconds, h.nanos),
                 T.BlockID(h.id_hash, T.PartSetHeader(h.id_total, h.id_part_hash)),
                 *[getattr(h, f) for f in H.BYTES_FIELDS])
    c, keep = t._c()
    got = []
    for leaf in range(14):
        out = (ctypes.c_uint8 * 128)()
        n = N.lib().cmtv_header_leaf_bytes(ctypes.byref(c), leaf, out, 128)
        got.append(bytes(out)[:n])
    assert got == H.leaves(h)


def test_leaf_bytes_report_the_length_when_the_buffer_is_short():
    ch = CHeader(H.kat_header())
    for leaf, want in enumerate(H.leaves(ch.h)):
        n, out = leaf_bytes(ch, leaf, cap=len(want) - 1)
        assert n == len(want) and set(out) == {CANARY}, leaf
        n, out = leaf_bytes(ch, leaf, cap=len(want))
        assert n == len(want) and out == want, leaf
        assert N.lib().cmtv_header_leaf_bytes(ctypes.byref(ch.c), leaf, None, 0) == len(want)
    # an empty item: length 0, nothing written
    n, out = leaf_bytes(CHeader(H.Hdr()), 1, cap=8)
    assert n == 0 and set(out) == {CANARY}


def test_leaf_bytes_einval_rules_leave_out_untouched():
    ch = CHeader(H.kat_header())
    lib = N.lib()
    out = (ctypes.c_uint8 * 64)(*([CANARY] * 64))
    assert lib.cmtv_header_leaf_bytes(None, 0, out, 64) == N.CMTV_EINVAL
    assert lib.cmtv_header_leaf_bytes(ctypes.byref(ch.c), 14, out, 64) == N.CMTV_EINVAL
    assert lib.cmtv_header_leaf_bytes(ctypes.byref(ch.c), 2**32 - 1, out, 64) == N.CMTV_EINVAL
    assert lib.cmtv_header_leaf_bytes(ctypes.byref(ch.c), 0, None, 64) == N.CMTV_EINVAL
    # a NULL pointer with a length, whichever leaf is asked for
    for i in range(N.HDR_N_BYTES_FIELDS):
        bad = CHeader(H.kat_header())
        bad.c.field[i] = None
        assert lib.cmtv_header_leaf_bytes(ctypes.byref(bad.c), 0, out, 64) == N.CMTV_EINVAL, i
    for name in ("hash", "psh_hash"):
        bad = CHeader(H.kat_header())
        setattr(bad.c.last_block_id, name, None)
        assert lib.cmtv_header_leaf_bytes(ctypes.byref(bad.c), 4, out, 64) == N.CMTV_EINVAL, name
    bad = CHeader(H.kat_header())
    bad.c.chain_id = None
    assert lib.cmtv_header_leaf_bytes(ctypes.byref(bad.c), 1, out, 64) == N.CMTV_EINVAL
    # ... and a NULL pointer with no length is an empty field
    ok = CHeader(H.kat_header().with_(app_hash=b""))
    ok.c.field[N.HDR_APP_HASH] = None
    assert lib.cmtv_header_leaf_bytes(ctypes.byref(ok.c), 10, out, 64) == 0
    assert set(bytes(out)) == {CANARY}


def test_the_time_leaf_follows_std_time_marshal():
    """A header has no hash where StdTimeMarshal fails; leaf 3 of such a header
    is CMTV_EINVAL, every other leaf is still encoded."""
    for sec, nanos in [(R.GO_ZERO_TIME_SECONDS - 1, 0), (R.LAST_VALID_SECOND + 1, 0), (-2**63, 0), (2**63 - 1, 0),
                       (0, -1), (0, 10**9), (0, 2**31 - 1), (0, -2**31)]:
        h = H.kat_header().with_(seconds=sec, nanos=nanos)
        assert H.header_hash(h) is None
        ch = CHeader(h)
        n, out = leaf_bytes(ch, 3)
        assert n == N.CMTV_EINVAL and set(out) == {CANARY}, (sec, nanos)
        assert leaf_bytes(ch, 2)[0] == 2
    for sec, nanos in [(R.GO_ZERO_TIME_SECONDS, 0), (R.LAST_VALID_SECOND, 999_999_999)]:
        h = H.kat_header().with_(seconds=sec, nanos=nanos)
        assert H.header_hash(h) is not None
        assert leaf_bytes(CHeader(h), 3)[0] == len(R.timestamp_bytes(sec, nanos))
    assert H.header_hash(H.kat_header().with_(validators_hash=b"")) is None


def test_null_context_is_einval_and_writes_nothing():
    lib = N.lib()
    out = (ctypes.c_uint8 * 64)(*([CANARY] * 64))
    has = (ctypes.c_uint8 * 2)(CANARY, CANARY)
    ch = CHeader(H.kat_header())
    assert lib.cmtv_header_hash(None, ctypes.byref(ch.c), out, has) == N.CMTV_EINVAL
    assert lib.cmtv_header_hashes(None, 1, ctypes.byref(ch.c), out, has) == N.CMTV_EINVAL
    assert lib.cmtv_header_hashes(None, 0, None, None, None) == N.CMTV_EINVAL
    off = (ctypes.c_uint32 * 2)(0, 1)
    tx = (ctypes.c_uint8 * 4)(1, 2, 3, 4)
    assert lib.cmtv_txs_hash(None, 1, tx, off, out) == N.CMTV_EINVAL
    assert lib.cmtv_txs_hash(None, 0, None, None, out) == N.CMTV_EINVAL
    assert lib.cmtv_txs_hashes(None, 1, off, tx, off, out) == N.CMTV_EINVAL
    assert set(bytes(out)) == {CANARY} and set(bytes(has)) == {CANARY}


def test_abi_version_and_stats_layout_unchanged():
    assert N.lib().cmtv_abi_version() == 11
    assert ctypes.sizeof(N.cmtv_stats) == 200
    with open(os.path.join(ROOT, "include", "cmtverify.h")) as f:
        assert "#define CMTV_ABI_VERSION 11" in f.read()
    assert ctypes.sizeof(N.cmtv_header) == 200 and N.cmtv_header.field.offset == 88
