"""The merkle device code on the CPU: tests/host/merklecheck.cpp compiles
cometbft_amd/csrc/merkle.h (sha256.h) with CMTV_HD = inline under
AddressSanitizer and UBSan (a plain host program), and every digest is compared
with tests/merkle_ref.py (hashlib and the recursive HashFromByteSlices).

  * the register leaf builders of Validator.Bytes() and CommitSig, then SHA-256
  * the generic leaf hash at every length 0..130 and pointer alignment
  * the inner-node hash
  * the kernels' pass structure, emulated lane by lane, for 0..2B+2 leaves
  * the reference's own test vectors (tests/golden/merkle_kat.json)
"""
import itertools
import json
import os
import random
import re
import struct
import subprocess
import sys

import pytest

from tests.host import hostbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import merkle_ref as R  # noqa: E402

SRC = os.path.join(ROOT, "tests", "host", "merklecheck.cpp")
BIN = os.path.join(ROOT, "build", "merklecheck_san")
with open(os.path.join(ROOT, "cometbft_amd", "csrc", "merkle.h")) as _f:
    B = int(re.search(r"#define\s+CMTV_MERKLE_BLOCK_LEAVES\s+(\d+)", _f.read()).group(1))

POWERS = [0, 1, 127, 128, 2**63 - 1, -1]
FLAGS = [0, 1, 2, 3, 127, 128, 255]
SIG_LENS = [0, 1, 63, 64]
SECONDS = [0, R.GO_ZERO_TIME_SECONDS, 2**31, R.LAST_VALID_SECOND]
NANOS = [0, 1, 999_999_999]


@pytest.fixture(scope="module")
def merklecheck():
    return hostbuild.build(SRC, BIN, ["-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def run(binary, records, n_out=None):
    inp = struct.pack("<I", len(records)) + b"".join(records)
    r = subprocess.run([binary], input=inp, capture_output=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    n_out = len(records) if n_out is None else n_out
    assert len(r.stdout) == 32 * n_out
    return [r.stdout[32 * i: 32 * i + 32] for i in range(n_out)]


def rec_validator(key_type, align, key, power):
    return struct.pack("<IIII", 1, key_type, align, len(key)) + key + struct.pack("<q", power)


def rec_commit_sig(flag, addr, sec, nanos, align, sig):
    return struct.pack("<II", 2, flag) + addr + struct.pack("<qiII", sec, nanos, align, len(sig)) + sig


def rec_leaf(align, item):
    return struct.pack("<III", 3, align, len(item)) + item


def rec_inner(left, right):
    return struct.pack("<I", 4) + left + right


def rec_trees(trees):
    out = [struct.pack("<II", 5, len(trees))]
    for t in trees:
        out.append(struct.pack("<I", len(t)))
        for it in t:
            out.append(struct.pack("<I", len(it)) + it)
    return b"".join(out)


def test_validator_leaf_builder(merklecheck):
    rng = random.Random(1)
    cases = []
    for kt in (R.KEY_ED25519, R.KEY_SECP256K1):
        for klen in range(1, 65):
            for power in POWERS:
                cases.append((kt, rng.randrange(4), rng.randbytes(klen), power))
    got = run(merklecheck, [rec_validator(*c) for c in cases])
    for c, g in zip(cases, got):
        assert g == R.leaf_hash(R.validator_bytes(c[0], c[2], c[3])), (c[0], len(c[2]), c[3])


def test_commit_sig_leaf_builder(merklecheck):
    rng = random.Random(2)
    cases = []
    for flag, slen, sec, nanos in itertools.product(FLAGS, SIG_LENS, SECONDS, NANOS):
        cases.append((flag, rng.randbytes(20), sec, nanos, rng.randrange(4), rng.randbytes(slen)))
    for _ in range(300):  # every signature length, random fields
        cases.append((rng.choice(FLAGS), rng.randbytes(20), rng.choice(SECONDS + [rng.randrange(2**34)]),
                      rng.choice([0, rng.randrange(10**9)]), rng.randrange(4), rng.randbytes(rng.randrange(65))))
    got = run(merklecheck, [rec_commit_sig(*c) for c in cases])
    for c, g in zip(cases, got):
        assert g == R.leaf_hash(R.commit_sig_leaf(c[0], c[1], c[2], c[3], c[5])), (c[0], c[2], c[3], len(c[5]))


def test_generic_leaf_hash_every_length_and_alignment(merklecheck):
    rng = random.Random(3)
    cases = [(al, rng.randbytes(n)) for n in range(131) for al in range(4)]
    cases += [(al, bytes([0xFF]) * n) for n in (55, 56, 63, 64, 119, 120) for al in range(4)]
    got = run(merklecheck, [rec_leaf(*c) for c in cases])
    for c, g in zip(cases, got):
        assert g == R.leaf_hash(c[1]), (c[0], len(c[1]))


def test_inner_hash(merklecheck):
    rng = random.Random(4)
    cases = [(rng.randbytes(32), rng.randbytes(32)) for _ in range(200)]
    cases += [(bytes(32), bytes(32)), (b"\xff" * 32, b"\xff" * 32), (bytes(32), b"\xff" * 32), (b"\xff" * 32, bytes(32))]
    got = run(merklecheck, [rec_inner(*c) for c in cases])
    for c, g in zip(cases, got):
        assert g == R.inner_hash(*c)


def test_block_reduction_every_leaf_count(merklecheck):
    """One call holding a tree of every size 0..2B+2, ragged items: the
    kernels' prefix arrays, block mapping and level reduction."""
    rng = random.Random(5)
    trees = [[rng.randbytes(rng.randrange(131)) for _ in range(n)] for n in range(2 * B + 3)]
    got = run(merklecheck, [rec_trees(trees)], len(trees))
    for n, (t, g) in enumerate(zip(trees, got)):
        assert g == R.root(t), n


def test_three_passes(merklecheck):
    """B^2 + 1 leaves: the smallest tree whose block nodes need a third pass."""
    items = [bytes([i & 0xFF]) for i in range(B * B + 1)]
    got = run(merklecheck, [rec_trees([items, [], items[:1]])], 3)
    assert got == [R.root(items), R.EMPTY_ROOT, R.leaf_hash(items[0])]


def test_kat_file(merklecheck):
    with open(os.path.join(ROOT, "tests", "golden", "merkle_kat.json")) as f:
        kat = json.load(f)
    assert len(kat["trees"]) == 6 and len(kat["rfc6962"]) == 4 and len(kat["header_hash"]["leaves"]) == 14
    trees = [[bytes.fromhex(i) for i in t["items"]] for t in kat["trees"]]
    want = [bytes.fromhex(t["root"]) for t in kat["trees"]]
    header = [bytes.fromhex(x) for x in kat["header_hash"]["leaves"]]
    trees.append(header)
    want.append(bytes.fromhex(kat["header_hash"]["root"]))
    assert [R.root(t) for t in trees] == want  # the reference restatement itself
    assert run(merklecheck, [rec_trees(trees)], len(trees)) == want
    recs, want = [], []
    for c in kat["rfc6962"]:
        if c["kind"] == "tree":
            recs.append(rec_trees([[bytes.fromhex(i) for i in c["items"]]]))
            assert R.root([bytes.fromhex(i) for i in c["items"]]).hex() == c["want"]
        elif c["kind"] == "leaf":
            recs.append(rec_leaf(1, bytes.fromhex(c["item"])))
            assert R.leaf_hash(bytes.fromhex(c["item"])).hex() == c["want"]
        else:
            # innerHash of two short byte strings: not two digests, so only the restatement takes it
            assert R.inner_hash(bytes.fromhex(c["left"]), bytes.fromhex(c["right"])).hex() == c["want"]
            continue
        want.append(bytes.fromhex(c["want"]))
    assert run(merklecheck, recs) == want
