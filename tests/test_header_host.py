"""The header device code on the CPU: tests/host/headercheck.cpp compiles
cometbft_amd/csrc/header.h (merkle.h, sha256.h) with CMTV_HD = inline under
AddressSanitizer and UBSan (a plain host program), and every digest is compared
with tests/header_ref.py (hashlib).

  * the three register leaf builders of Header.Hash(), then SHA-256
  * the 16-lane group reduction, emulated lane by lane with the host form of
    the row move, for one header and for several headers per wave
  * the transaction leaf of Txs.Hash() at every length 0..130 and alignment
  * the reference's known-answer header (tests/golden/merkle_kat.json)
"""
import itertools
import json
import os
import random
import struct
import subprocess
import sys

import pytest

from tests.host import hostbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import header_ref as H  # noqa: E402
import merkle_ref as R  # noqa: E402
from header_util import U64, as_int64, gen_header  # noqa: E402

SRC = os.path.join(ROOT, "tests", "host", "headercheck.cpp")
BIN = os.path.join(ROOT, "build", "headercheck_san")

FIELD_LENS = [0, 1, 20, 32, 52, 53, 64]  # 52 | 53: one block | two blocks
VARINTS = [0, 1, 127, 128, 2**63 - 1, -1, 2**64 - 1]
SECONDS = [0, R.GO_ZERO_TIME_SECONDS, 2**31, R.LAST_VALID_SECOND]
NANOS = [0, 1, 999_999_999]
ID_HASH_LENS = [0, 1, 31, 32]
ID_TOTALS = [0, 1, 2**32 - 1]


@pytest.fixture(scope="module")
def headercheck():
    return hostbuild.build(SRC, BIN, ["-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def run(binary, records, n_out=None):
    inp = struct.pack("<I", len(records)) + b"".join(records)
    r = subprocess.run([binary], input=inp, capture_output=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    n_out = len(records) if n_out is None else n_out
    assert len(r.stdout) == 32 * n_out
    return [r.stdout[32 * i: 32 * i + 32] for i in range(n_out)]


def rec_bytes(align, b):
    return struct.pack("<III", 1, align, len(b)) + b


def rec_varints(a, b):
    return struct.pack("<IQQ", 2, a & U64, b & U64)


def rec_block_id(al, h, total, al2, p):
    return struct.pack("<III", 3, al, len(h)) + h + struct.pack("<III", total, al2, len(p)) + p


def _lp(b):
    return struct.pack("<I", len(b)) + b


def rec_headers(hs):
    out = [struct.pack("<II", 4, len(hs))]
    for h in hs:
        out.append(struct.pack("<QQ", h.version_block & U64, h.version_app & U64) + _lp(h.chain_id)
                   + struct.pack("<qqi", h.height, h.seconds, h.nanos) + _lp(h.id_hash)
                   + struct.pack("<I", h.id_total) + _lp(h.id_part_hash)
                   + b"".join(_lp(getattr(h, f)) for f in H.BYTES_FIELDS))
    return b"".join(out)


def rec_tx(align, tx):
    return struct.pack("<III", 5, align, len(tx)) + tx


def test_bytes_leaf_builder(headercheck):
    rng = random.Random(1)
    cases = [(al, rng.randbytes(n)) for n in FIELD_LENS for al in range(4)]
    cases += [(al, b"\xff" * n) for n in FIELD_LENS for al in range(4)]
    cases += [(rng.randrange(4), rng.randbytes(n)) for n in range(65)]
    got = run(headercheck, [rec_bytes(*c) for c in cases])
    for c, g in zip(cases, got):
        assert g == R.leaf_hash(H.tagged_bytes(0x0A, c[1])), (c[0], len(c[1]))


def test_varints_leaf_builder(headercheck):
    cases = list(itertools.product(VARINTS, VARINTS))                       # versions; a height beside b = 0
    cases += [(s, n) for s in SECONDS for n in NANOS]                       # times
    rng = random.Random(2)
    cases += [(rng.randrange(2**64) >> rng.randrange(64), rng.randrange(2**64) >> rng.randrange(64)) for _ in range(300)]
    got = run(headercheck, [rec_varints(*c) for c in cases])
    for (a, b), g in zip(cases, got):
        assert g == R.leaf_hash(H.tagged_varint(0x08, a & U64) + H.tagged_varint(0x10, b & U64)), (a, b)
    # what the three leaves are, in the restatement's own terms
    assert run(headercheck, [rec_varints(-1, 0), rec_varints(R.GO_ZERO_TIME_SECONDS, 999_999_999)]) == [
        R.leaf_hash(H.leaves(H.Hdr(height=-1))[2]),
        R.leaf_hash(R.timestamp_bytes(R.GO_ZERO_TIME_SECONDS, 999_999_999))]


def test_block_id_leaf_builder(headercheck):
    rng = random.Random(3)
    cases = [(rng.randrange(4), rng.randbytes(hl), total, rng.randrange(4), rng.randbytes(pl))
             for hl, total, pl in itertools.product(ID_HASH_LENS, ID_TOTALS, ID_HASH_LENS)]
    cases += [(a1, b"\xff" * 32, 2**32 - 1, a2, b"\xff" * 32) for a1 in range(4) for a2 in range(4)]
    cases += [(rng.randrange(4), rng.randbytes(rng.randrange(33)), rng.randrange(2**32) >> rng.randrange(32),
               rng.randrange(4), rng.randbytes(rng.randrange(33))) for _ in range(300)]
    got = run(headercheck, [rec_block_id(*c) for c in cases])
    for c, g in zip(cases, got):
        assert g == R.leaf_hash(H.block_id_bytes(c[1], c[2], c[4])), (len(c[1]), c[2], len(c[4]))


def test_group_reduction(headercheck):
    """One header, and every count around a wave's four: the staged
    struct-of-arrays fields, a leaf per lane, four levels of row moves."""
    rng = random.Random(4)
    recs, want = [], []
    for n in (1, 2, 3, 4, 5, 7, 8, 9, 17):
        hs = [gen_header(rng) for _ in range(n)]
        recs.append(rec_headers(hs))
        want += [H.header_hash(h) for h in hs]
    assert run(headercheck, recs, len(want)) == want


def test_group_reduction_edge_fields(headercheck):
    """Headers whose neighbours in the wave differ in every field's length."""
    rng = random.Random(5)
    hs = []
    for n in FIELD_LENS:
        hs.append(gen_header(rng, chain_id=rng.randbytes(n), app_hash=rng.randbytes(n), proposer_address=rng.randbytes(n),
                             validators_hash=rng.randbytes(max(n, 1))))
    for v in VARINTS:
        hs.append(gen_header(rng, version_block=v & U64, version_app=(v >> 1) & U64, height=as_int64(v)))
    for s, ns in itertools.product(SECONDS, NANOS):
        hs.append(gen_header(rng, seconds=s, nanos=ns))
    for hl, total, pl in itertools.product(ID_HASH_LENS, ID_TOTALS, ID_HASH_LENS):
        hs.append(gen_header(rng, id_hash=rng.randbytes(hl), id_total=total, id_part_hash=rng.randbytes(pl)))
    hs.append(H.Hdr(validators_hash=b"\x01"))  # every other item empty
    got = run(headercheck, [rec_headers(hs)], len(hs))
    for h, g in zip(hs, got):
        assert g == H.header_hash(h), h


def test_transaction_leaf_every_length_and_alignment(headercheck):
    rng = random.Random(6)
    cases = [(al, rng.randbytes(n)) for n in range(131) for al in range(4)]
    cases += [(al, b"\xff" * n) for n in (55, 56, 63, 64, 119, 120) for al in range(4)]
    got = run(headercheck, [rec_tx(*c) for c in cases])
    for c, g in zip(cases, got):
        assert g == H.tx_leaf(c[1]), (c[0], len(c[1]))


def test_kat_header(headercheck):
    with open(os.path.join(ROOT, "tests", "golden", "merkle_kat.json")) as f:
        kat = json.load(f)["header_hash"]
    h = H.kat_header()
    assert [x.hex() for x in H.leaves(h)] == kat["leaves"]  # the restatement itself
    assert H.header_hash(h) == bytes.fromhex(kat["root"])
    assert run(headercheck, [rec_headers([h])]) == [bytes.fromhex(kat["root"])]
