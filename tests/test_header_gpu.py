"""Header.Hash() and Txs.Hash() on the device (cmtv_header_hash[es],
cmtv_txs_hash[es]; cometbft_amd/csrc/header.hip, merkle.hip) against
tests/header_ref.py: the reference's known-answer header, every header count
around the group, wave and workgroup boundaries, the edge values of every
field, headers without a hash, one differing byte per field, the host-encoded
route of a long field, a call cut into runs, transaction lists around the
block size B, the Python wrappers, the argument rules that need an open
context and CMTV_FAULT_AT."""
import ctypes
import itertools
import json
import os
import random
import re
import sys

import numpy as np
import pytest

from cometbft_amd import _native as N
from cometbft_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import header_ref as H  # noqa: E402
import merkle_ref as R  # noqa: E402
from header_util import U64, CHeader, as_int64, gen_header  # noqa: E402

pytestmark = pytest.mark.gpu

CSRC = os.path.join(ROOT, "cometbft_amd", "csrc")


def _define(name, file):
    with open(os.path.join(CSRC, file)) as f:
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, f.read()).group(1))


B = _define("CMTV_MERKLE_BLOCK_LEAVES", "merkle.h")
WG = _define("CMTV_HEADERS_PER_WG", "header.h")  # headers per workgroup; 4 per wave, one per 16 lanes
CANARY = 0xA5
_p8, _p32 = T._p8, T._p32
VARINTS = [0, 1, 127, 128, 2**63 - 1, -1, 2**64 - 1]
SECONDS = [0, R.GO_ZERO_TIME_SECONDS, 2**31, R.LAST_VALID_SECOND]
NANOS = [0, 1, 999_999_999]
FIELD_LENS = [0, 1, 20, 32, 52, 53, 64]


def _canary(n):
    return (ctypes.c_uint8 * max(n, 1))(*([CANARY] * max(n, 1)))


def _split(out, n):
    raw = bytes(out)
    return [raw[32 * i: 32 * i + 32] for i in range(n)]


def c_header_hashes(ctx, chs):
    """The roots, None where has_hash says there is none (the 32 bytes are then zero)."""
    n = len(chs)
    arr = (N.cmtv_header * n)(*[c.c for c in chs])
    out, has = _canary(32 * n), _canary(n)
    rc = N.lib().cmtv_header_hashes(ctx.handle, n, arr, out, has)
    assert rc == N.CMTV_OK, rc
    roots = _split(out, n)
    assert set(bytes(has)[:n]) <= {0, 1}
    assert all(r == bytes(32) for r, ok in zip(roots, has) if not ok)
    return [r if ok else None for r, ok in zip(roots, has)]


def c_header_hash(ctx, ch):
    out, has = _canary(32), _canary(1)
    rc = N.lib().cmtv_header_hash(ctx.handle, ctypes.byref(ch.c), out, has)
    assert rc == N.CMTV_OK, rc
    return bytes(out) if has[0] else None


def check(ctx, hs, align=None):
    chs = [CHeader(h, i % 4 if align is None else align) for i, h in enumerate(hs)]
    got = c_header_hashes(ctx, chs)
    for i, (h, g) in enumerate(zip(hs, got)):
        assert g == H.header_hash(h), (i, h)
    return got


def _offsets(lens):
    off = np.zeros(len(lens) + 1, np.uint32)
    if len(lens):
        off[1:] = np.cumsum(lens)
    return off


def _blob(parts):
    return np.frombuffer(b"".join(parts) + b"\0\0\0\0", np.uint8).copy()


def c_txs_hashes(ctx, blocks):
    txs = [tx for b in blocks for tx in b]
    out = _canary(32 * len(blocks))
    rc = N.lib().cmtv_txs_hashes(ctx.handle, len(blocks), _p32(_offsets([len(b) for b in blocks])), _p8(_blob(txs)),
                                 _p32(_offsets([len(tx) for tx in txs])), out)
    assert rc == N.CMTV_OK, rc
    return _split(out, len(blocks))


def c_txs_hash(ctx, txs):
    out = _canary(32)
    rc = N.lib().cmtv_txs_hash(ctx.handle, len(txs), _p8(_blob(txs)), _p32(_offsets([len(tx) for tx in txs])), out)
    assert rc == N.CMTV_OK, rc
    return bytes(out)


# ------------------------------------------------------------------ headers
def test_kat_header(gpu_ctx):
    with open(os.path.join(ROOT, "tests", "golden", "merkle_kat.json")) as f:
        want = bytes.fromhex(json.load(f)["header_hash"]["root"])
    h = H.kat_header()
    assert H.header_hash(h) == want
    for align in range(4):
        assert c_header_hash(gpu_ctx, CHeader(h, align)) == want
    # types/block_test.go:327 "nil ValidatorsHash yields nil"
    assert c_header_hash(gpu_ctx, CHeader(h.with_(validators_hash=b""))) is None
    assert c_header_hashes(gpu_ctx, [CHeader(h), CHeader(h.with_(validators_hash=b"")), CHeader(h)]) == [want, None, want]


@pytest.mark.parametrize("n", sorted({1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257, WG - 1, WG, WG + 1, 2 * WG + 1}))
def test_header_counts(gpu_ctx, n):
    """One group of 16 lanes a header, four a wave, WG a workgroup."""
    rng = random.Random(100 + n)
    check(gpu_ctx, [gen_header(rng) for _ in range(n)])


def test_edge_fields(gpu_ctx):
    rng = random.Random(81)
    hs = []
    for n in FIELD_LENS:
        hs.append(gen_header(rng, chain_id=rng.randbytes(n), validators_hash=rng.randbytes(max(n, 1)),
                             **{f: rng.randbytes(n) for f in H.BYTES_FIELDS if f != "validators_hash"}))
        for f in ("chain_id",) + H.BYTES_FIELDS:  # one field at the length, its neighbours as usual
            if n or f != "validators_hash":
                hs.append(gen_header(rng, **{f: rng.randbytes(n)}))
    for a, b in itertools.product(VARINTS, VARINTS):
        hs.append(gen_header(rng, version_block=a & U64, version_app=b & U64, height=as_int64(b)))
    for s, ns in itertools.product(SECONDS, NANOS):
        hs.append(gen_header(rng, seconds=s, nanos=ns))
    for hl, total, pl in itertools.product([0, 1, 31, 32], [0, 1, 2**32 - 1], [0, 1, 31, 32]):
        hs.append(gen_header(rng, id_hash=rng.randbytes(hl), id_total=total, id_part_hash=rng.randbytes(pl)))
    hs.append(H.Hdr(validators_hash=b"\x01"))
    got = check(gpu_ctx, hs)
    assert None not in got
    for align in range(4):  # every field at every pointer alignment
        check(gpu_ctx, hs[:2 * len(FIELD_LENS)], align)


def test_out_of_range_times_have_no_hash_and_leave_the_neighbours_alone(gpu_ctx):
    rng = random.Random(82)
    hs = [gen_header(rng) for _ in range(40)]
    bad = [(R.GO_ZERO_TIME_SECONDS - 1, 0), (R.LAST_VALID_SECOND + 1, 0), (-2**63, 0), (2**63 - 1, 0), (0, -1),
           (0, 10**9), (0, 2**31 - 1), (0, -2**31)]
    at = [0, 3, 4, 15, 16, 17, 31, 39]
    for i, (s, ns) in zip(at, bad):
        hs[i] = hs[i].with_(seconds=s, nanos=ns)
    hs[20] = hs[20].with_(validators_hash=b"")
    got = check(gpu_ctx, hs)
    assert [i for i, g in enumerate(got) if g is None] == sorted(at + [20])
    # a call of hashless headers only: no device work, every flag 0
    assert check(gpu_ctx, [hs[i] for i in at]) == [None] * len(at)


def test_one_differing_byte_per_field_changes_the_root(gpu_ctx):
    """A lane reading its neighbour's field would leave one of these roots unchanged."""
    rng = random.Random(83)
    base = gen_header(rng)

    def flip(b):
        return bytes([b[0] ^ 1]) + b[1:]

    variants = [base.with_(version_block=base.version_block ^ 1), base.with_(version_app=base.version_app ^ 1),
                base.with_(chain_id=flip(base.chain_id)), base.with_(height=base.height ^ 1),
                base.with_(seconds=base.seconds ^ 1), base.with_(nanos=base.nanos ^ 1),
                base.with_(id_hash=flip(base.id_hash)), base.with_(id_total=base.id_total ^ 1),
                base.with_(id_part_hash=flip(base.id_part_hash))]
    variants += [base.with_(**{f: flip(getattr(base, f))}) for f in H.BYTES_FIELDS]
    assert len(variants) == 18  # the 14 leaves, the version's, the time's and the block id's parts apart
    hs = []
    for v in variants:  # each pair side by side in a wave
        hs += [base, v]
    got = check(gpu_ctx, hs)
    assert all(g == got[0] for g in got[0::2])
    assert len(set(got[1::2]) | {got[0]}) == len(variants) + 1


def test_long_fields_take_the_host_encoded_route(gpu_ctx):
    rng = random.Random(84)
    wide = [gen_header(rng, app_hash=rng.randbytes(65)), gen_header(rng, app_hash=rng.randbytes(200)),
            gen_header(rng, chain_id=rng.randbytes(65)), gen_header(rng, id_hash=rng.randbytes(33)),
            gen_header(rng, id_part_hash=rng.randbytes(33)), gen_header(rng, proposer_address=rng.randbytes(1000))]
    for h in wide:
        assert c_header_hash(gpu_ctx, CHeader(h)) == H.header_hash(h)
    # mixed with device-form and hashless headers in one call, order kept
    dev = [gen_header(rng) for _ in range(20)]
    mix = dev[:3] + [wide[0]] + dev[3:4] + [wide[1], wide[2], dev[4].with_(validators_hash=b"")] + dev[5:] + wide[3:]
    got = check(gpu_ctx, mix)
    assert got.count(None) == 1 and got[7] is None
    check(gpu_ctx, wide)


def _run_rule():
    """Headers of gen_header's sizes that one run holds, by merkle.cpp's own rule:
    16 + the staged arrays' bytes + the byte fields' per header, kRunBytes a run."""
    with open(os.path.join(CSRC, "merkle.cpp")) as f:
        m = re.search(r"kRunBytes\s*=\s*(\d+)ull\s*<<\s*(\d+)", f.read())
    run_bytes = int(m.group(1)) << int(m.group(2))
    with open(os.path.join(CSRC, "header.h")) as f:
        src = f.read()
    k = {name: int(re.search(r"%s\s*=\s*(\d+)" % name, src).group(1))
         for name in ("kHeaderU64Fields", "kHeaderVarFields", "kHeaderU32Fields")}
    fixed = 8 * k["kHeaderU64Fields"] + 4 * k["kHeaderVarFields"] + 4 * k["kHeaderU32Fields"]
    var = 16 + 32 + 32 + 8 * 32 + 20
    return run_bytes // (16 + fixed + var)


def test_a_call_cut_into_runs(gpu_ctx):
    """One header more than a run holds (about 73,000 of them): two runs. The
    structs repeat five headers' arrays."""
    rng = random.Random(85)
    base = [CHeader(gen_header(rng)) for _ in range(5)]
    assert all(len(c.h.chain_id) == 16 for c in base)
    refs = [H.header_hash(c.h) for c in base]
    n = _run_rule() + 1
    assert 10_000 < n < 200_000
    pick = np.array([rng.randrange(5) for _ in range(n)])
    arr = (N.cmtv_header * n)()
    size = ctypes.sizeof(N.cmtv_header)
    rows = np.stack([np.frombuffer(bytes(c.c), np.uint8) for c in base])
    np.frombuffer(arr, np.uint8).reshape(n, size)[:] = rows[pick]
    out = (ctypes.c_uint8 * (32 * n))()
    assert N.lib().cmtv_header_hashes(gpu_ctx.handle, n, arr, out, None) == N.CMTV_OK
    got = np.frombuffer(out, np.uint8).reshape(n, 32)
    want = np.stack([np.frombuffer(r, np.uint8) for r in refs])[pick]
    assert np.array_equal(got, want), np.nonzero((got != want).any(axis=1))[0][:10]


# ------------------------------------------------------------------ transactions
@pytest.mark.parametrize("n", [0, 1, 2, 3, B - 1, B, B + 1, 2 * B + 1])
def test_txs_hash(gpu_ctx, n):
    rng = random.Random(200 + n)
    txs = [rng.randbytes(rng.randrange(131)) for _ in range(n)]
    assert c_txs_hash(gpu_ctx, txs) == H.txs_hash(txs)
    if n == 0:
        assert H.txs_hash(txs) == R.EMPTY_ROOT


def test_txs_every_length(gpu_ctx):
    rng = random.Random(86)
    txs = [rng.randbytes(n) for n in range(131)]
    assert c_txs_hash(gpu_ctx, txs) == H.txs_hash(txs)
    # a transaction's leaf is not the item's: the same bytes through cmtv_merkle_root differ
    out = _canary(32)
    assert N.lib().cmtv_merkle_root(gpu_ctx.handle, len(txs), _p8(_blob(txs)), _p32(_offsets([len(t) for t in txs])),
                                    out) == N.CMTV_OK
    assert bytes(out) == R.root(txs) != H.txs_hash(txs)


def test_one_long_transaction(gpu_ctx):
    rng = random.Random(87)
    txs = [rng.randbytes(10), rng.randbytes(100_000), b""]
    assert c_txs_hash(gpu_ctx, txs) == H.txs_hash(txs)
    assert c_txs_hash(gpu_ctx, txs[1:2]) == H.tx_leaf(txs[1])


def test_txs_hashes_many_blocks(gpu_ctx):
    rng = random.Random(88)
    blocks = [[rng.randbytes(rng.randrange(300)) for _ in range(rng.choice([0, 0, 1, 2, 10, 40]))] for _ in range(400)]
    blocks[0], blocks[399], blocks[200] = [], [], [rng.randbytes(250) for _ in range(B + 3)]
    got = c_txs_hashes(gpu_ctx, blocks)
    assert got == [H.txs_hash(b) for b in blocks]
    assert got[0] == R.EMPTY_ROOT
    for i in (0, 1, 200, 399):
        assert c_txs_hash(gpu_ctx, blocks[i]) == got[i]


# ------------------------------------------------------------------ wrappers
def _t_header(h):
    return T.Header(h.version_block, h.version_app, h.chain_id.decode(), h.height, (h.seconds, h.nanos),
                    T.BlockID(h.id_hash, T.PartSetHeader(h.id_total, h.id_part_hash)),
                    *[getattr(h, f) for f in H.BYTES_FIELDS])


def test_python_wrappers_agree_with_the_c_calls(gpu_ctx):
    import cometbft_amd

    rng = random.Random(89)
    hs = [gen_header(rng) for _ in range(9)]
    hs[2] = hs[2].with_(validators_hash=b"")
    hs[4] = hs[4].with_(app_hash=rng.randbytes(70))
    hs[6] = hs[6].with_(nanos=10**9)
    want = [H.header_hash(h) for h in hs]
    assert want[2] is None and want[6] is None
    ths = [_t_header(h) for h in hs]
    assert T.header_hashes(ths, gpu_ctx) == want == c_header_hashes(gpu_ctx, [CHeader(h) for h in hs])
    assert [t.hash(gpu_ctx) for t in ths] == want
    assert T.header_hashes([], gpu_ctx) == []
    assert _t_header(H.kat_header()).hash(gpu_ctx) == H.header_hash(H.kat_header())
    blocks = [[rng.randbytes(rng.randrange(200)) for _ in range(n)] for n in (0, 1, 7, B + 2)]
    assert T.txs_hashes(blocks, gpu_ctx) == c_txs_hashes(gpu_ctx, blocks) == [H.txs_hash(b) for b in blocks]
    assert T.txs_hash(blocks[2], gpu_ctx) == H.txs_hash(blocks[2])
    assert T.txs_hash([], gpu_ctx) == R.EMPTY_ROOT and T.txs_hashes([], gpu_ctx) == []
    assert cometbft_amd.header_hashes is T.header_hashes and cometbft_amd.Header is T.Header
    assert cometbft_amd.txs_hash is T.txs_hash and cometbft_amd.txs_hashes is T.txs_hashes


# ------------------------------------------------------------------ argument rules
def test_argument_errors_write_nothing(gpu_ctx):
    lib, h = N.lib(), gpu_ctx.handle
    rng = random.Random(90)
    out, has = _canary(4 * 32), _canary(4)

    def untouched():
        return set(bytes(out)) == {CANARY} and set(bytes(has)) == {CANARY}

    good = CHeader(gen_header(rng))
    assert lib.cmtv_header_hash(h, None, out, has) == N.CMTV_EINVAL
    assert lib.cmtv_header_hash(h, ctypes.byref(good.c), None, has) == N.CMTV_EINVAL
    assert lib.cmtv_header_hashes(h, 2, None, out, has) == N.CMTV_EINVAL
    # a NULL pointer with a length: every pointer of the struct, alone and inside a plural call
    bads = []
    for i in range(N.HDR_N_BYTES_FIELDS):
        bad = CHeader(gen_header(rng))
        bad.c.field[i] = None
        bads.append(bad)
    for name in ("hash", "psh_hash"):
        bad = CHeader(gen_header(rng))
        setattr(bad.c.last_block_id, name, None)
        bads.append(bad)
    bad = CHeader(gen_header(rng))
    bad.c.chain_id = None
    bads.append(bad)
    for bad in bads:
        assert lib.cmtv_header_hash(h, ctypes.byref(bad.c), out, has) == N.CMTV_EINVAL
        arr = (N.cmtv_header * 3)(good.c, good.c, bad.c)
        assert lib.cmtv_header_hashes(h, 3, arr, out, has) == N.CMTV_EINVAL
    assert untouched()
    # has_hash NULL with a header that has no hash
    for nohash in (good.h.with_(validators_hash=b""), good.h.with_(seconds=R.LAST_VALID_SECOND + 1),
                   good.h.with_(nanos=-1)):
        nh = CHeader(nohash)
        assert lib.cmtv_header_hash(h, ctypes.byref(nh.c), out, None) == N.CMTV_EINVAL
        arr = (N.cmtv_header * 3)(good.c, nh.c, good.c)
        assert lib.cmtv_header_hashes(h, 3, arr, out, None) == N.CMTV_EINVAL
    assert untouched()
    # ... and has_hash NULL is fine when every header has one
    arr = (N.cmtv_header * 2)(good.c, good.c)
    out2 = _canary(64)
    assert lib.cmtv_header_hashes(h, 2, arr, out2, None) == N.CMTV_OK
    assert _split(out2, 2) == [H.header_hash(good.h)] * 2

    tx, off = _blob([b"abc", b"de"]), _offsets([3, 2])
    block_off = _offsets([2])
    assert lib.cmtv_txs_hashes(h, 1, None, _p8(tx), _p32(off), out) == N.CMTV_EINVAL
    assert lib.cmtv_txs_hashes(h, 1, _p32(block_off), _p8(tx), None, out) == N.CMTV_EINVAL
    assert lib.cmtv_txs_hashes(h, 1, _p32(block_off), None, _p32(off), out) == N.CMTV_EINVAL
    assert lib.cmtv_txs_hashes(h, 1, _p32(block_off), _p8(tx), _p32(off), None) == N.CMTV_EINVAL
    assert lib.cmtv_txs_hash(h, 2, _p8(tx), None, out) == N.CMTV_EINVAL
    assert lib.cmtv_txs_hash(h, 2, _p8(tx), _p32(np.array([0, 3, 2], np.uint32)), out) == N.CMTV_EINVAL
    assert lib.cmtv_txs_hashes(h, 2, _p32(np.array([0, 2, 1], np.uint32)), _p8(tx), _p32(off), out) == N.CMTV_EINVAL
    assert untouched()
    # n = 0 is not an error and writes nothing
    assert lib.cmtv_header_hashes(h, 0, None, None, None) == N.CMTV_OK
    assert lib.cmtv_txs_hashes(h, 0, None, None, None, None) == N.CMTV_OK


def test_fault_at_fails_the_call_and_the_next_one_succeeds():
    """CMTV_FAULT_AT fails a launch on the host without running it: the header
    launch goes through the same counter as every other."""
    from conftest import _env_ctx

    ctx = _env_ctx(CMTV_FAULT_AT=1)
    try:
        ch = CHeader(gen_header(random.Random(91)))
        out, has = _canary(32), _canary(1)
        assert N.lib().cmtv_header_hash(ctx.handle, ctypes.byref(ch.c), out, has) == N.CMTV_EHIP
        assert set(bytes(out)) == {CANARY} and set(bytes(has)) == {CANARY}
        assert c_header_hash(ctx, ch) == H.header_hash(ch.h)
        assert ctx.stats()["faults_injected"] == 1
    finally:
        ctx.close()
    ctx = _env_ctx(CMTV_FAULT_AT=1)
    try:
        txs = [b"a", b"bc"]
        out = _canary(32)
        assert N.lib().cmtv_txs_hash(ctx.handle, 2, _p8(_blob(txs)), _p32(_offsets([1, 2])), out) == N.CMTV_EHIP
        assert set(bytes(out)) == {CANARY}
        assert c_txs_hash(ctx, txs) == H.txs_hash(txs)
    finally:
        ctx.close()
