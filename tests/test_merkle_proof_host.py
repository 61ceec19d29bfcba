"""The merkle proof device code on the CPU: tests/host/merkleproofcheck.cpp
compiles cometbft_amd/csrc/merkle_proof.h (merkle.h, sha256.h) with CMTV_HD =
inline under AddressSanitizer and UBSan (a plain host program), and every
byte is compared with tests/merkle_proof_ref.py (the recursive
trailsFromByteSlices / FlattenAunts and computeHashFromAunts).

  * the proof passes, emulated lane by lane, for 0..2B+2 leaves and for
    B^2 + 1 (three passes, the spreading step over two upper levels)
  * the verify lane on every one of those proofs, all 65,795 of the B^2 + 1 call included
  * the verify lane on the mutations that give each status, on int64 edge
    totals with 63 synthetic aunts, and without a leaf or a root
"""
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
import merkle_proof_ref as P  # noqa: E402
import merkle_ref as R  # noqa: E402

SRC = os.path.join(ROOT, "tests", "host", "merkleproofcheck.cpp")
BIN = os.path.join(ROOT, "build", "merkleproofcheck_san")
with open(os.path.join(ROOT, "cometbft_amd", "csrc", "merkle.h")) as _f:
    B = int(re.search(r"#define\s+CMTV_MERKLE_BLOCK_LEAVES\s+(\d+)", _f.read()).group(1))


@pytest.fixture(scope="module")
def check():
    return hostbuild.build(SRC, BIN, ["-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def run(binary, record):
    r = subprocess.run([binary], input=struct.pack("<I", 1) + record, capture_output=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout


def build(binary, trees, kind=0):
    """[(root, [(total, index, leaf_hash, aunts)])] per tree, from the emulated passes."""
    rec = [struct.pack("<III", 1, kind, len(trees))]
    for t in trees:
        rec.append(struct.pack("<I", len(t)))
        rec += [struct.pack("<I", len(it)) + it for it in t]
    raw = run(binary, b"".join(rec))
    out, at = [], 0
    for t in trees:
        root, at = raw[at: at + 32], at + 32
        proofs = []
        for i in range(len(t)):
            lh, (k,) = raw[at: at + 32], struct.unpack_from("<I", raw, at + 32)
            at += 36
            proofs.append((len(t), i, lh, [raw[at + 32 * j: at + 32 * j + 32] for j in range(k)]))
            at += 32 * k
        out.append((root, proofs))
    assert at == len(raw)
    return out


def verify(binary, cases, has_leaves=True, leaf_kind=0, has_roots=True):
    """cases: (total, index, leaf_hash, aunts, root, leaf) -> [(status, out_hash)]."""
    rec = [struct.pack("<IIIII", 2, len(cases), has_leaves, leaf_kind, has_roots)]
    for total, index, lh, aunts, root, leaf in cases:
        rec.append(struct.pack("<qq", total, index) + lh + struct.pack("<I", len(aunts)) + b"".join(aunts))
        if has_roots:
            rec.append(root)
        if has_leaves:
            rec.append(struct.pack("<I", len(leaf)) + leaf)
    raw = run(binary, b"".join(rec))
    assert len(raw) == 33 * len(cases)
    return [(raw[33 * i], raw[33 * i + 1: 33 * i + 33]) for i in range(len(cases))]


def expect(cases, has_leaves=True, tx=False, has_roots=True):
    out = []
    for total, index, lh, aunts, root, leaf in cases:
        st, _, h = P.verify(total, index, lh, aunts, root if has_roots else None, leaf if has_leaves else None, tx=tx)
        out.append((st, h))
    return out


def mutations(proof, root, leaf, rng):
    """The smallest change of a good proof that gives each status, and a few more."""
    total, index, lh, aunts = proof
    flip = lambda b, i=0: b[:i] + bytes([b[i] ^ 1]) + b[i + 1:]  # noqa: E731
    extra = rng.randbytes(32)
    out = [
        (total, index, lh, aunts, root, leaf),
        (-1, index, lh, aunts, root, leaf),
        (total, -1, lh, aunts, root, leaf),
        (-1, -1, lh, aunts, root, leaf),
        (total, index, lh, aunts, root, flip(leaf) if leaf else b"x"),
        (total, index, flip(lh, 31), aunts, root, leaf),
        (total, total, lh, aunts, root, leaf),
        (0, index, lh, aunts, root, leaf),
        (0, 0, lh, aunts, root, leaf),
        (total, index, lh, aunts + [extra], root, leaf),
        (total, index, lh, aunts[:-1], root, leaf),
        (total, index, lh, [], root, leaf),
        (total, index, lh, (aunts * 64)[:64], root, leaf),
        (total, index, lh, (aunts * 101)[:101], root, leaf),
        (total, index, lh, [flip(aunts[0], 7)] + aunts[1:], root, leaf),
        (total, index, lh, aunts[:-1] + [flip(aunts[-1], 31)], root, leaf),
        (total, index, lh, aunts, flip(root, 16), leaf),
        (total, index ^ 1, lh, aunts, root, leaf),       # the sibling's index
        (total + 1, index, lh, aunts, root, leaf),
        (1, 0, lh, [], lh, leaf),                        # a one-leaf tree of this leaf
    ]
    return out


def test_proofs_of_every_leaf_count(check):
    """One call holding a tree of every size 0..2B+2, ragged items: every root,
    leaf hash, aunt count and aunt, then Verify of every proof."""
    rng = random.Random(5)
    trees = [[rng.randbytes(rng.randrange(131)) for _ in range(n)] for n in range(2 * B + 3)]
    got = build(check, trees)
    cases = []
    for n, (t, (root, proofs)) in enumerate(zip(trees, got)):
        want_root, want = P.proofs_from_byte_slices(t)
        assert root == want_root == R.root(t), n
        assert proofs == want, n
        cases += [(p[0], p[1], p[2], p[3], root, t[p[1]]) for p in proofs]
    res = verify(check, cases)
    assert res == expect(cases)
    assert all(st == P.OK for st, _ in res)


def test_three_passes_and_spreading(check):
    """B^2 + 1 leaves: three passes, the aunts of two upper levels spread to every leaf."""
    items = [bytes([i & 0xFF, i >> 8 & 0xFF]) for i in range(B * B + 1)]
    trees = [items, [], items[:1], items[:B + 1]]
    got = build(check, trees)
    for t, (root, proofs) in zip(trees, got):
        want_root, want = P.proofs_from_byte_slices(t)
        assert root == want_root
        assert proofs == want
    # the verify lane on every proof of every tree: each verifies, and computes its tree's root
    cases = [(p[0], p[1], p[2], p[3], root, t[p[1]]) for t, (root, proofs) in zip(trees, got) for p in proofs]
    res = verify(check, cases)
    assert res == [(P.OK, c[4]) for c in cases]
    # and a sample element-wise against the recursive computeHashFromAunts
    pick = [0, 1, B - 1, B, B * B - 1, B * B] + random.Random(6).sample(range(len(cases)), 300)
    assert [res[i] for i in pick] == expect([cases[i] for i in pick])


def test_transaction_leaves(check):
    rng = random.Random(7)
    trees = [[rng.randbytes(rng.choice([0, 1, 55, 56, 64, 250])) for _ in range(n)] for n in (0, 1, 2, 7, B + 3)]
    got = build(check, trees, kind=1)
    cases = []
    for t, (root, proofs) in zip(trees, got):
        want_root, want = P.txs_proofs(t)
        assert (root, proofs) == (want_root, want)
        cases += [(p[0], p[1], p[2], p[3], root, t[p[1]]) for p in proofs]
    cases.append(cases[-1][:5] + (b"another tx",))
    res = verify(check, cases, leaf_kind=1)
    assert res == expect(cases, tx=True)
    assert [st for st, _ in res] == [P.OK] * (len(cases) - 1) + [P.ELEAF]


@pytest.mark.parametrize("n", [5, B + 1])
def test_every_status_from_the_smallest_change(check, n):
    rng = random.Random(8 + n)
    items = [rng.randbytes(rng.randrange(1, 90)) for _ in range(n)]
    root, proofs = P.proofs_from_byte_slices(items)
    cases = []
    for i in sorted({0, 1, 2, n // 2, n - 2, n - 1}):
        cases += mutations(proofs[i], root, items[i], rng)
    res = verify(check, cases)
    want = expect(cases)
    assert res == want
    assert {st for st, _ in res} == set(range(8))
    # the first mutations give the statuses in order
    assert [st for st, _ in res[:5]] == [P.OK, P.ENEGTOTAL, P.ENEGINDEX, P.ENEGTOTAL, P.ELEAF]
    # without the leaf bytes (ComputeRootHash) and without a root
    assert verify(check, cases, has_leaves=False) == expect(cases, has_leaves=False)
    assert verify(check, cases, has_roots=False) == expect(cases, has_roots=False)
    assert verify(check, cases, has_leaves=False, has_roots=False) == expect(cases, has_leaves=False, has_roots=False)


def test_int64_edge_totals_with_synthetic_aunts(check):
    rng = random.Random(9)
    totals = [2**63 - 1, 2**62, 2**62 + 1, 2**32, 2**32 + 1, 3, 2] + [rng.randrange(1, 2**63) for _ in range(200)]
    cases = []
    for total in totals:
        for index in {0, total - 1, rng.randrange(total)}:
            k = P.proof_len(total, index)
            lh = rng.randbytes(32)
            for kk in {k, k + 1, max(k - 1, 0), 63, 64}:
                aunts = [rng.randbytes(32) for _ in range(kk)]
                try:
                    root = P.hash_from_aunts(index, total, lh, aunts)
                except P.ProofError:
                    root = bytes(32)
                cases.append((total, index, lh, aunts, root, b""))
    assert max(P.proof_len(2**63 - 1, 0), P.proof_len(2**63 - 1, 2**62)) == 63
    res = verify(check, cases, has_leaves=False)
    assert res == expect(cases, has_leaves=False)
    assert {st for st, _ in res} == {P.OK, P.EEXTRA, P.EMISSING}
