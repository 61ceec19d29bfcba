"""Merkle inclusion proofs on the device (cmtv_merkle_proofs, cmtv_txs_proofs,
cmtv_part_set_proofs, cmtv_merkle_proofs_verify; cometbft_amd/csrc/
merkle_proof.hip) against tests/merkle_proof_ref.py, the recursive
trailsFromByteSlices / FlattenAunts and computeHashFromAunts: building over
every tree size around the block size B and the pass thresholds, item lengths
around the SHA-256 block at every alignment, transactions, part sets and a
call cut into runs; verifying every built proof, every status from its
smallest cause, int64 edge totals, shared roots, no leaf, no root and a mixed
batch of 10,000; the Python wrappers, pinned argument memory, CMTV_FAULT_AT
and the argument rules with an open context."""
import ctypes
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
import merkle_proof_ref as P  # noqa: E402
import merkle_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(ROOT, "cometbft_amd", "csrc", "merkle.h")) as _f:
    B = int(re.search(r"#define\s+CMTV_MERKLE_BLOCK_LEAVES\s+(\d+)", _f.read()).group(1))
CANARY = 0xA5
_p8, _p32 = T._p8, T._p32
_p64 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))  # noqa: E731
SIZES = [0, 1, 2, 3, 4, 5, 7, 8, 9, B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1, 3 * B + 1]


def _offsets(lens):
    off = np.zeros(len(lens) + 1, np.uint32)
    if len(lens):
        off[1:] = np.cumsum(lens)
    return off


def _blob(parts, lead=0):
    return np.frombuffer(bytes(lead) + b"".join(parts) + b"\0\0\0\0", np.uint8).copy()


def _hashes(raw, n):
    raw = bytes(raw)
    return [raw[32 * i: 32 * i + 32] for i in range(n)]


def ref_flat(trees, tx=False):
    """(roots, leaf hashes, aunt offsets, aunts) of the trees, flat as the C call returns them."""
    roots, lhs, off, aunts = [], [], [0], []
    for t in trees:
        root, proofs = P.txs_proofs(t) if tx else P.proofs_from_byte_slices(t)
        roots.append(root)
        for i, (total, index, lh, a) in enumerate(proofs):
            assert (total, index) == (len(t), i)
            lhs.append(lh)
            aunts += a
            off.append(len(aunts))
    return roots, lhs, off, aunts


def c_proofs(ctx, trees, tx=False, lead=0, put=lambda a: a, slack=0):
    """The building call on trees of byte strings: (rc, roots, leaf hashes, aunt offsets, aunts)."""
    items = [it for t in trees for it in t]
    tree_off = put(_offsets([len(t) for t in trees]))
    item_off = put(_offsets([len(i) for i in items]) + np.uint32(lead))
    blob = put(_blob(items, lead))
    n_aunts = ctypes.c_uint64()
    assert N.lib().cmtv_merkle_proofs_len(len(trees), _p32(tree_off), ctypes.byref(n_aunts)) == N.CMTV_OK
    na = n_aunts.value
    roots = put(np.full(32 * max(len(trees), 1), CANARY, np.uint8))
    lh = put(np.full(32 * max(len(items), 1), CANARY, np.uint8))
    aunt_off = put(np.full(len(items) + 1, 0xA5A5A5A5, np.uint32))
    aunts = put(np.full(32 * (na + slack) + 32, CANARY, np.uint8))
    fn = N.lib().cmtv_txs_proofs if tx else N.lib().cmtv_merkle_proofs
    rc = fn(ctx.handle, len(trees), _p32(tree_off), _p8(blob), _p32(item_off), _p8(roots), _p8(lh), _p32(aunt_off),
            _p8(aunts), na + slack)
    if rc != N.CMTV_OK:
        return rc, roots, lh, aunt_off, aunts
    assert set(aunts[32 * na:].tolist()) == {CANARY}  # nothing past the last aunt
    return rc, _hashes(roots, len(trees)), _hashes(lh, len(items)), aunt_off.tolist(), _hashes(aunts, na)


def c_roots(ctx, trees, tx=False):
    items = [it for t in trees for it in t]
    out = (ctypes.c_uint8 * (32 * len(trees)))()
    fn = N.lib().cmtv_txs_hashes if tx else N.lib().cmtv_merkle_roots
    assert fn(ctx.handle, len(trees), _p32(_offsets([len(t) for t in trees])), _p8(_blob(items)),
              _p32(_offsets([len(i) for i in items])), out) == N.CMTV_OK
    return _hashes(out, len(trees))


def check_build(ctx, trees, tx=False, **kw):
    rc, roots, lhs, off, aunts = c_proofs(ctx, trees, tx, **kw)
    assert rc == N.CMTV_OK, rc
    want = ref_flat(trees, tx)
    assert roots == want[0]
    assert lhs == want[1]
    assert off == want[2]
    assert aunts == want[3]
    assert roots == c_roots(ctx, trees, tx)
    return roots, lhs, off, aunts


def cases_of(trees, built):
    """(total, index, leaf_hash, aunts, root, leaf) of every proof of a built call."""
    roots, lhs, off, aunts = built
    out, g = [], 0
    for t, root in zip(trees, roots):
        for i, leaf in enumerate(t):
            out.append((len(t), i, lhs[g], aunts[off[g]: off[g + 1]], root, leaf))
            g += 1
    return out


def c_verify(ctx, cases, leaves=True, roots=True, kind=N.PROOF_LEAF_ITEM, shared=None, want_out=True,
             put=lambda a: a):
    """cmtv_merkle_proofs_verify of (total, index, leaf_hash, aunts, root, leaf) cases:
    (rc, statuses, out hashes, all_ok). shared: (roots, root_idx) in the place of one root a proof."""
    n = len(cases)
    total = put(np.array([c[0] for c in cases] + [0], np.int64))
    index = put(np.array([c[1] for c in cases] + [0], np.int64))
    lh = put(_blob([c[2] for c in cases]))
    aunt_off = put(_offsets([len(c[3]) for c in cases]))
    aunts = put(_blob([a for c in cases for a in c[3]]))
    if shared:
        rblob, ridx, n_roots = put(_blob(shared[0])), put(np.array(list(shared[1]) + [0], np.uint32)), len(shared[0])
    else:
        rblob, ridx, n_roots = put(_blob([c[4] for c in cases])), None, n
    lblob, loff = put(_blob([c[5] for c in cases])), put(_offsets([len(c[5]) for c in cases]))
    status = put(np.full(max(n, 1), CANARY, np.uint8))
    out = put(np.full(32 * max(n, 1), CANARY, np.uint8))
    ok = ctypes.c_int(-7)
    rc = N.lib().cmtv_merkle_proofs_verify(
        ctx.handle, n, _p64(total), _p64(index), _p8(lh), _p32(aunt_off), _p8(aunts), n_roots if roots else 0,
        _p8(rblob) if roots else None, _p32(ridx) if (roots and ridx is not None) else None,
        _p8(lblob) if leaves else None, _p32(loff) if leaves else None, kind, _p8(status),
        _p8(out) if want_out else None, ctypes.byref(ok))
    return rc, status[:n].tolist(), _hashes(out, n), ok.value


def expect(cases, leaves=True, roots=True, tx=False):
    res = [P.verify(c[0], c[1], c[2], c[3], c[4] if roots else None, c[5] if leaves else None, tx=tx) for c in cases]
    return [r[0] for r in res], [r[2] for r in res]


def check_verify(ctx, cases, **kw):
    tx = kw.get("kind", N.PROOF_LEAF_ITEM) == N.PROOF_LEAF_TX
    rc, st, out, ok = c_verify(ctx, cases, **kw)
    assert rc == N.CMTV_OK, rc
    want_st, want_out = expect(cases, kw.get("leaves", True), kw.get("roots", True), tx)
    assert st == want_st
    assert out == want_out
    assert ok == int(all(s == P.OK for s in want_st))
    return st


def verify_built(ctx, trees, built, kind=N.PROOF_LEAF_ITEM):
    """Every proof of a built call through the verify call, each tree's proofs on
    its root (root_idx), from the call's flat results: every status is OK and
    every computed root is the tree's."""
    roots, lhs, off, aunts = built
    sizes = [len(t) for t in trees]
    n = sum(sizes)
    if n == 0:
        return
    items = [it for t in trees for it in t]
    total = np.repeat(np.array(sizes, np.int64), sizes)
    index = np.concatenate([np.arange(k, dtype=np.int64) for k in sizes])
    ridx = np.repeat(np.arange(len(trees), dtype=np.uint32), sizes)
    status, out = np.full(n, CANARY, np.uint8), np.full(32 * n, CANARY, np.uint8)
    ok = ctypes.c_int(-7)
    rc = N.lib().cmtv_merkle_proofs_verify(
        ctx.handle, n, _p64(total), _p64(index), _p8(_blob(lhs)), _p32(np.array(off, np.uint32)), _p8(_blob(aunts)),
        len(roots), _p8(_blob(roots)), _p32(ridx), _p8(_blob(items)), _p32(_offsets([len(i) for i in items])), kind,
        _p8(status), _p8(out), ctypes.byref(ok))
    assert rc == N.CMTV_OK and ok.value == 1
    assert not status.any()
    assert bytes(out) == b"".join(roots[k] for k in ridx.tolist())


# ------------------------------------------------------------------ building
@pytest.fixture(scope="module")
def mixed(gpu_ctx):
    """One call of trees of every size around B, empty ones among them: the trees and what the call gave."""
    rng = random.Random(81)
    trees = []
    for n in SIZES:
        trees.append([rng.randbytes(rng.randrange(131)) for _ in range(n)])
        if n % 3 == 0:
            trees.append([])
    return trees, check_build(gpu_ctx, trees)


def test_mixed_tree_sizes_in_one_call(gpu_ctx, mixed):
    trees, built = mixed
    assert [len(t) for t in trees if t] == SIZES[1:]
    assert built[0][1] == R.EMPTY_ROOT
    assert all(s == P.OK for s in check_verify(gpu_ctx, cases_of(trees, built)))
    verify_built(gpu_ctx, trees, built)


@pytest.fixture(scope="module")
def big(gpu_ctx):
    """B^2 + 1 two-byte items: three passes, the spreading kernel over two upper levels."""
    items = [bytes([i & 0xFF, i >> 8 & 0xFF]) for i in range(B * B + 1)]
    return items, check_build(gpu_ctx, [items])


def test_three_passes_and_spreading(gpu_ctx, big):
    items, built = big
    n = len(items)
    assert built[2][1] == 2 * 8 + 1 and built[2][n] - built[2][n - 1] == 1  # leaf 0: 17 aunts, the last leaf: one
    verify_built(gpu_ctx, [items], built)  # every one of the 65,537 proofs
    # and a sample element-wise against the recursive computeHashFromAunts
    cases = cases_of([items], built)
    pick = [0, 1, B - 1, B, n - 2, n - 1] + random.Random(82).sample(range(n), 2000)
    assert all(s == P.OK for s in check_verify(gpu_ctx, [cases[i] for i in pick]))


def test_item_lengths_at_every_alignment(gpu_ctx):
    rng = random.Random(83)
    lens = [0, 1, 54, 55, 56, 63, 64, 65, 130]
    for lead in range(4):
        # each length at each alignment: the items follow each other, so a one-byte item shifts the next
        items = []
        for shift in range(4):
            items += [rng.randbytes(n) for n in lens] + [rng.randbytes(1)]
        trees = [items, items[:11], []]
        built = check_build(gpu_ctx, trees, lead=lead)
        assert all(s == P.OK for s in check_verify(gpu_ctx, cases_of(trees, built)))


def test_transaction_leaves(gpu_ctx):
    rng = random.Random(84)
    blocks = [[rng.randbytes(rng.choice([0, 1, 55, 56, 64, 250, 1000])) for _ in range(n)] for n in (0, 1, 2, 10, B + 3)]
    built = check_build(gpu_ctx, blocks, tx=True)
    cases = cases_of(blocks, built)
    assert all(s == P.OK for s in check_verify(gpu_ctx, cases, kind=N.PROOF_LEAF_TX))
    # the same proofs against the item leaf kind: the leaf is SHA-256(tx), so every leaf check fails
    assert set(check_verify(gpu_ctx, cases, kind=N.PROOF_LEAF_ITEM)) == {P.ELEAF}


def c_part_set(ctx, data, part_size, cap=None):
    n = (len(data) + part_size - 1) // part_size if part_size else 0
    na = sum(P.proof_len(n, i) for i in range(n))
    blob = _blob([data])
    total = ctypes.c_uint32(0xA5A5A5A5)
    root, lh = np.full(32, CANARY, np.uint8), np.full(32 * max(n, 1), CANARY, np.uint8)
    aunt_off, aunts = np.full(n + 1, 0xA5A5A5A5, np.uint32), np.full(32 * max(na, 1), CANARY, np.uint8)
    rc = N.lib().cmtv_part_set_proofs(ctx.handle, _p8(blob), len(data), part_size, ctypes.byref(total), _p8(root),
                                      _p8(lh), _p32(aunt_off), _p8(aunts), na if cap is None else cap)
    return rc, total.value, bytes(root), _hashes(lh, n), aunt_off.tolist(), _hashes(aunts, na)


@pytest.mark.parametrize("size,part_size", [(3 * 65536 + 1, 65536), (100, 7), (0, 65536), (65536, 65536)])
def test_part_sets(gpu_ctx, size, part_size):
    data = random.Random(85).randbytes(size)
    parts = P.parts(data, part_size)
    rc, total, root, lhs, off, aunts = c_part_set(gpu_ctx, data, part_size)
    assert rc == N.CMTV_OK
    want = ref_flat([parts])
    assert (total, [root], lhs, off, aunts) == (len(parts), *want)
    header, proofs = T.part_set_from_data(data, part_size, gpu_ctx)
    assert (header.total, header.hash) == (len(parts), want[0][0])
    assert [(p.total, p.index, p.leaf_hash, p.aunts) for p in proofs] == P.proofs_from_byte_slices(parts)[1]
    # PartSet.AddPart: every part against the header's hash
    assert T.verify_proofs(proofs, [header.hash], parts, root_idx=[0] * len(parts), ctx=gpu_ctx) == [None] * len(parts)


def test_a_call_cut_into_runs(gpu_ctx):
    """1,000 trees of 150 two-byte items: 150,000 leaf hashes and more than a
    million aunts, about 40 MB of results against 32 MB a run (merkle_proof.cpp
    kRunBytes), so two runs through the two staging slots and the call's own
    result buffers. The trees repeat five, so the reference is computed five times."""
    rng = random.Random(86)
    base = [[rng.randbytes(2) for _ in range(150)] for _ in range(5)]
    refs = [ref_flat([t]) for t in base]
    per = len(refs[0][3])  # the aunts of a tree depend on its size alone
    assert 32 * 1000 * (1 + 150 + per) > 32 << 20
    pick = [rng.randrange(5) for _ in range(1000)]
    launches = gpu_ctx.stats()["kernel_launches"]
    rc, roots, lhs, off, aunts = c_proofs(gpu_ctx, [base[k] for k in pick])
    assert rc == N.CMTV_OK
    # a tree of 150 leaves is one pass, so one launch a run: two runs
    assert gpu_ctx.stats()["kernel_launches"] - launches == 2
    assert roots == [refs[k][0][0] for k in pick]
    assert lhs == [h for k in pick for h in refs[k][1]]
    assert off == [t * per + o for t in range(len(pick)) for o in refs[0][2][:-1]] + [len(pick) * per]
    assert aunts == [a for k in pick for a in refs[k][3]]
    verify_built(gpu_ctx, [base[k] for k in pick], (roots, lhs, off, aunts))  # all 150,000 proofs


def test_a_verify_call_cut_into_runs(gpu_ctx):
    """36,000 proofs of two trees of 900-byte items stage about 47 MB against
    32 MiB a run (merkle_proof.cpp kRunBytes): two runs through the two slots
    and the call's own result buffers. Failures of every kind lie in both runs;
    once with a root a proof and once with root_idx, element-wise against the
    reference, statuses and out_hash."""
    rng = random.Random(94)
    good, roots = [], []
    for k, n in enumerate((1000, 37)):
        items = [rng.randbytes(900) for _ in range(n)]
        root, proofs = P.proofs_from_byte_slices(items)
        roots.append(root)
        good += [p + (root, it, k) for p, it in zip(proofs, items)]
    cases = [good[rng.randrange(len(good))] for _ in range(36_000)]
    assert sum(72 + 32 + 32 * len(c[3]) + len(c[5]) for c in cases) > (32 << 20) * 5 // 4
    flip = lambda b, i=0: b[:i] + bytes([b[i] ^ 0x40]) + b[i + 1:]  # noqa: E731
    kinds = [
        lambda c: (-c[0],) + c[1:],
        lambda c: (c[0], -1 - c[1]) + c[2:],
        lambda c: c[:5] + (flip(c[5], 899),) + c[6:],
        lambda c: (c[1], c[0]) + c[2:],
        lambda c: c[:3] + (c[3] + [c[2]],) + c[4:],
        lambda c: c[:3] + (c[3][1:],) + c[4:],
        lambda c: c[:3] + ([flip(c[3][0], 31)] + c[3][1:],) + c[4:],
        lambda c: c[:6] + (1 - c[6],),  # the other tree's root
    ]
    # the first and last proofs, and a spread over both runs
    for j, i in enumerate([0, 1, 35_998, 35_999] + rng.sample(range(2, 35_998), 396)):
        cases[i] = kinds[j % len(kinds)](cases[i])
    per_proof = [c[:4] + (roots[c[6]], c[5]) for c in cases]
    want_st, want_out = expect(per_proof)
    assert set(want_st[:18_000]) == set(want_st[18_000:]) == set(range(8))
    launches = gpu_ctx.stats()["kernel_launches"]
    rc, st, out, ok = c_verify(gpu_ctx, per_proof)
    assert gpu_ctx.stats()["kernel_launches"] - launches == 2  # one launch a run
    assert rc == N.CMTV_OK and ok == 0
    assert st == want_st
    assert out == want_out
    rc, st, out, ok = c_verify(gpu_ctx, per_proof, shared=(roots, [c[6] for c in cases]))
    assert rc == N.CMTV_OK and ok == 0 and st == want_st and out == want_out
    # a root table with entries no proof names, and the roots in the other order
    table = [bytes(32)] * 3 + roots[::-1] + [bytes(32)]
    rc, st, out, ok = c_verify(gpu_ctx, per_proof, shared=(table, [4 - c[6] for c in cases]))
    assert rc == N.CMTV_OK and st == want_st and out == want_out


# ------------------------------------------------------------------ verifying
def mutations(case, rng):
    """The smallest change of a good proof that gives each status, and a few more."""
    total, index, lh, aunts, root, leaf = case
    flip = lambda b, i=0: b[:i] + bytes([b[i] ^ 1]) + b[i + 1:]  # noqa: E731
    return [
        case,
        (-1, index, lh, aunts, root, leaf),
        (total, -1, lh, aunts, root, leaf),
        (-1, -1, lh, aunts, root, leaf),
        (total, index, lh, aunts, root, flip(leaf)),
        (total, total, lh, aunts, root, leaf),
        (0, index, lh, aunts, root, leaf),
        (total, index, lh, aunts + [rng.randbytes(32)], root, leaf),
        (total, index, lh, aunts[:-1], root, leaf),
        (total, index, lh, (aunts * 64)[:64], root, leaf),
        (total, index, lh, (aunts * 101)[:101], root, leaf),
        (total, index, lh, [flip(aunts[0], 7)] + aunts[1:], root, leaf),
        (total, index, lh, aunts, flip(root, 16), leaf),
        (total, index ^ 1, lh, aunts, root, leaf),  # the sibling's index: what it gives is the reference's to say
    ]


@pytest.fixture(scope="module")
def mutated():
    rng = random.Random(87)
    cases = []
    for n in (5, B + 1):
        items = [rng.randbytes(rng.randrange(1, 90)) for _ in range(n)]
        root, proofs = P.proofs_from_byte_slices(items)
        for i in sorted({0, 1, 2, n // 2, n - 2, n - 1}):
            cases += mutations(proofs[i] + (root, items[i]), rng)
    return cases


def test_every_status_from_its_smallest_cause(gpu_ctx, mutated):
    st = check_verify(gpu_ctx, mutated)
    assert st[:13] == [P.OK, P.ENEGTOTAL, P.ENEGINDEX, P.ENEGTOTAL, P.ELEAF, P.EINDEX, P.EINDEX, P.EEXTRA, P.EMISSING,
                       P.EEXTRA, P.EEXTRA, P.EROOT, P.EROOT]
    assert set(st) == set(range(8))


def test_out_hash_for_every_status(gpu_ctx, mutated):
    rc, st, out, ok = c_verify(gpu_ctx, mutated)
    assert rc == N.CMTV_OK and ok == 0
    for c, s, h in zip(mutated, st, out):
        if s == P.ELEAF:
            assert h == R.leaf_hash(c[5])
        elif s == P.OK:
            assert h == c[4]
        elif s == P.EROOT:
            assert h == P.hash_from_aunts(c[1], c[0], c[2], c[3]) != c[4]
        else:
            assert h == bytes(32)
    # status alone
    rc, st2, out2, _ = c_verify(gpu_ctx, mutated, want_out=False)
    assert rc == N.CMTV_OK and st2 == st and set(b"".join(out2)) == {CANARY}


def test_without_leaves_and_without_roots(gpu_ctx, mutated):
    check_verify(gpu_ctx, mutated, leaves=False)               # ComputeRootHash: no leaf check
    check_verify(gpu_ctx, mutated, roots=False)                # the computed root in out_hash, no comparison
    check_verify(gpu_ctx, mutated, leaves=False, roots=False)


def test_int64_edge_totals_with_synthetic_aunts(gpu_ctx):
    rng = random.Random(88)
    cases = []
    for total in [2**63 - 1, 2**62, 2**62 + 1, 2**32 + 1] + [rng.randrange(1, 2**63) for _ in range(100)]:
        for index in {0, total - 1, rng.randrange(total)}:
            k = P.proof_len(total, index)
            lh = rng.randbytes(32)
            for kk in {k, k + 1, max(k - 1, 0), 63}:
                aunts = [rng.randbytes(32) for _ in range(kk)]
                try:
                    root = P.hash_from_aunts(index, total, lh, aunts)
                except P.ProofError:
                    root = bytes(32)
                cases.append((total, index, lh, aunts, root, b""))
    assert P.proof_len(2**63 - 1, 0) == 63
    assert set(check_verify(gpu_ctx, cases, leaves=False)) == {P.OK, P.EEXTRA, P.EMISSING}


def test_many_proofs_on_one_root(gpu_ctx, mixed):
    trees, built = mixed
    cases = cases_of(trees, built)
    roots = built[0]
    ridx = []
    for k, tr in enumerate(trees):
        ridx += [k] * len(tr)
    rc, st, out, ok = c_verify(gpu_ctx, cases, shared=(roots, ridx))
    assert rc == N.CMTV_OK and set(st) == {P.OK} and ok == 1
    # every proof against the first non-empty tree's root: only that tree's verify
    first = next(k for k, tr in enumerate(trees) if tr)
    rc, st, out, ok = c_verify(gpu_ctx, cases, shared=(roots, [first] * len(cases)))
    assert rc == N.CMTV_OK and ok == 0
    assert st == [P.OK if k == first else P.EROOT for k in ridx]
    assert out == [c[4] for c in cases]


def test_mixed_batch_of_ten_thousand(gpu_ctx):
    """10,000 proofs of a 1,000-leaf tree and a 5-leaf tree, 1% of each failure."""
    rng = random.Random(89)
    good = []
    for n in (1000, 5):
        items = [rng.randbytes(rng.randrange(1, 60)) for _ in range(n)]
        root, proofs = P.proofs_from_byte_slices(items)
        good += [p + (root, it) for p, it in zip(proofs, items)]
    cases = [good[rng.randrange(len(good))] for _ in range(10_000)]
    flip = lambda b, i=0: b[:i] + bytes([b[i] ^ 0x40]) + b[i + 1:]  # noqa: E731
    kinds = [
        lambda c: (-c[0],) + c[1:],
        lambda c: (c[0], -1 - c[1]) + c[2:],
        lambda c: c[:5] + (c[5] + b"!",),
        lambda c: (c[1], c[0]) + c[2:],
        lambda c: c[:3] + (c[3] + [c[2]],) + c[4:],
        lambda c: c[:3] + (c[3][1:],) + c[4:],
        lambda c: c[:4] + (flip(c[4], 9),) + c[5:],
    ]
    at = rng.sample(range(10_000), 100 * len(kinds))
    for j, i in enumerate(at):
        cases[i] = kinds[j % len(kinds)](cases[i])
    st = check_verify(gpu_ctx, cases)
    for s in range(1, 8):
        assert st.count(s) >= 90, s
    assert st.count(P.OK) == 10_000 - 700


# ------------------------------------------------------------------ wrappers and plumbing
def test_python_wrappers_and_their_error_strings(gpu_ctx):
    import cometbft_amd

    for name in ("Proof", "TxProof", "proofs_from_byte_slices", "proofs_from_trees", "txs_proofs",
                 "part_set_from_data", "verify_proofs"):
        assert getattr(cometbft_amd, name) is getattr(T, name)
    rng = random.Random(90)
    items = [rng.randbytes(rng.randrange(1, 50)) for _ in range(7)]
    want_root, want = P.proofs_from_byte_slices(items)
    root, proofs = T.proofs_from_byte_slices(items, gpu_ctx)
    assert root == want_root and [(p.total, p.index, p.leaf_hash, p.aunts) for p in proofs] == want
    trees = [items, [], items[:1], items[:3]]
    got = T.proofs_from_trees(trees, gpu_ctx)
    assert [r for r, _ in got] == [R.root(t) for t in trees] and got[1] == (R.EMPTY_ROOT, [])
    assert T.proofs_from_trees([], gpu_ctx) == []
    for p, it in zip(proofs, items):
        p.validate_basic()
        p.verify(root, it, gpu_ctx)
        assert p.compute_root_hash(gpu_ctx) == root
    p = proofs[3]

    def error_of(proof, root, leaf):
        want = P.verify(proof.total, proof.index, proof.leaf_hash, proof.aunts, root, leaf)[1]
        with pytest.raises(ValueError) as e:
            proof.verify(root, leaf, gpu_ctx)
        assert str(e.value) == want, (str(e.value), want)
        return want

    with pytest.raises(ValueError, match="^invalid root hash: cannot be nil$"):
        p.verify(None, items[3], gpu_ctx)
    assert error_of(T.Proof(-1, p.index, p.leaf_hash, p.aunts), root, items[3]) == "proof total must be positive"
    assert error_of(T.Proof(p.total, -1, p.leaf_hash, p.aunts), root, items[3]) == "proof index cannot be negative"
    assert error_of(p, root, b"other").startswith("invalid leaf hash: wanted " + R.leaf_hash(b"other").hex().upper())
    assert error_of(T.Proof(7, 7, p.leaf_hash, p.aunts), root, items[3]) == \
        "compute root hash: invalid index 7 and/or total 7"
    assert error_of(T.Proof(0, 0, p.leaf_hash, p.aunts), root, items[3]) == \
        "compute root hash: invalid index 0 and/or total 0"
    assert error_of(T.Proof(7, 3, p.leaf_hash, p.aunts + [bytes(32)]), root, items[3]) == \
        "compute root hash: unexpected inner hashes"
    assert error_of(T.Proof(7, 3, p.leaf_hash, p.aunts[:-1]), root, items[3]) == \
        "compute root hash: expected at least one inner hash"
    bad_root = bytes(32)
    assert error_of(p, bad_root, items[3]) == f"invalid root hash: wanted {bad_root.hex().upper()} got {root.hex().upper()}"
    assert error_of(p, b"short", items[3]) == f"invalid root hash: wanted {b'short'.hex().upper()} got {root.hex().upper()}"
    # shapes that ValidateBasic refuses get Verify's own strings: a short leaf hash, more than 100 aunts
    assert error_of(T.Proof(7, 3, p.leaf_hash[:10], p.aunts), root, items[3]) == \
        f"invalid leaf hash: wanted {R.leaf_hash(items[3]).hex().upper()} got {p.leaf_hash[:10].hex().upper()}"
    assert error_of(T.Proof(-1, 3, p.leaf_hash[:10], p.aunts), root, items[3]) == "proof total must be positive"
    assert error_of(T.Proof(7, 3, p.leaf_hash, (p.aunts * 40)[:101]), root, items[3]) == \
        "compute root hash: unexpected inner hashes"
    with pytest.raises(ValueError, match="^expected Aunts#1 size to be 32, got 5$"):
        T.Proof(7, 3, p.leaf_hash, [p.aunts[0], b"short"]).verify(root, items[3], gpu_ctx)
    with pytest.raises(T.ReferencePanic, match="ComputeRootHash errored expected at least one inner hash"):
        T.Proof(7, 3, p.leaf_hash, p.aunts[:-1]).compute_root_hash(gpu_ctx)
    errs = T.verify_proofs([p, proofs[0], p], [root, bad_root, root], [items[3], items[0], b"x"], ctx=gpu_ctx)
    assert errs[0] is None and errs[1].startswith("invalid root hash") and errs[2].startswith("invalid leaf hash")

    # transactions: Txs.Proof and TxProof.Validate
    txs = [rng.randbytes(rng.randrange(1, 300)) for _ in range(9)]
    data_hash, tps = T.txs_proofs(txs, gpu_ctx)
    assert data_hash == T.txs_hash(txs, gpu_ctx) == P.txs_proofs(txs)[0]
    for tx, tp in zip(txs, tps):
        assert tp.data == tx and tp.leaf() == R.sha256(tx) and tp.root_hash == data_hash
        tp.validate(data_hash, gpu_ctx)
    tp = tps[4]
    ref = lambda q, dh: P.tx_proof_validate(q.root_hash, q.data, (q.proof.total, q.proof.index, q.proof.leaf_hash,  # noqa: E731
                                                                   q.proof.aunts), dh)
    variants = [
        (tp, bytes(32), "proof matches different data hash"),
        (T.TxProof(data_hash, tp.data, T.Proof(9, -1, tp.proof.leaf_hash, tp.proof.aunts)), data_hash,
         "proof index cannot be negative"),
        (T.TxProof(data_hash, tp.data, T.Proof(0, 0, tp.proof.leaf_hash, tp.proof.aunts)), data_hash,
         "proof total must be positive"),
        (T.TxProof(data_hash, b"forged", tp.proof), data_hash, "proof is not internally consistent"),
        (T.TxProof(data_hash, tp.data, T.Proof(9, 5, tp.proof.leaf_hash, tp.proof.aunts)), data_hash,
         "proof is not internally consistent"),
    ]
    for q, dh, want in variants:
        assert ref(q, dh) == want
        with pytest.raises(ValueError) as e:
            q.validate(dh, gpu_ctx)
        assert str(e.value) == want


def test_arguments_in_pinned_memory(gpu_ctx):
    rng = random.Random(91)
    block = gpu_ctx.alloc_pinned(4 << 20)
    try:
        arena = T._Arena(block)
        trees = [[rng.randbytes(rng.randrange(100)) for _ in range(n)] for n in (150, 0, B + 1)]
        built = check_build(gpu_ctx, trees, put=arena.put)
        cases = cases_of(trees, built)
        rc, st, out, ok = c_verify(gpu_ctx, cases, put=arena.put)
        assert rc == N.CMTV_OK and set(st) == {P.OK} and ok == 1
    finally:
        block.free()


def test_fault_at_fails_the_call_and_the_next_one_succeeds():
    """CMTV_FAULT_AT fails a launch on the host without running it: every output keeps its canaries."""
    from conftest import _env_ctx

    rng = random.Random(92)
    trees = [[rng.randbytes(20) for _ in range(n)] for n in (150, B + 5)]
    for at in (1, 2, 3):  # the first pass, the second pass, the spreading launch
        ctx = _env_ctx(CMTV_FAULT_AT=at)
        try:
            rc, roots, lh, aunt_off, aunts = c_proofs(ctx, trees)
            assert rc == N.CMTV_EHIP
            assert all(set(a.tolist()) == {CANARY} for a in (roots, lh, aunts))
            assert set(aunt_off.tolist()) == {0xA5A5A5A5}
            built = check_build(ctx, trees)
            assert ctx.stats()["faults_injected"] == 1
        finally:
            ctx.close()
    ctx = _env_ctx(CMTV_FAULT_AT=1)
    try:
        cases = cases_of(trees, built)
        rc, st, out, ok = c_verify(ctx, cases)
        assert rc == N.CMTV_EHIP and set(st) == {CANARY} and set(b"".join(out)) == {CANARY} and ok == -7
        assert all(s == P.OK for s in check_verify(ctx, cases))
    finally:
        ctx.close()


def test_argument_errors_with_an_open_context(gpu_ctx):
    rng = random.Random(93)
    trees = [[rng.randbytes(5) for _ in range(6)]]
    built = check_build(gpu_ctx, trees)
    rc, roots, lh, aunt_off, aunts = c_proofs(gpu_ctx, trees, slack=-1)  # cap_aunts one too few
    assert rc == N.CMTV_EINVAL
    assert all(set(a.tolist()) == {CANARY} for a in (roots, lh, aunts)) and set(aunt_off.tolist()) == {0xA5A5A5A5}
    assert c_proofs(gpu_ctx, trees, slack=5)[0] == N.CMTV_OK
    assert c_part_set(gpu_ctx, bytes(100), 0)[0] == N.CMTV_EINVAL
    assert c_part_set(gpu_ctx, bytes(100), 2**32 - 99)[0] == N.CMTV_EINVAL
    rc, total, root, *_ = c_part_set(gpu_ctx, bytes(100), 7, cap=3)
    assert rc == N.CMTV_EINVAL and total == 0xA5A5A5A5 and set(root) == {CANARY}
    cases = cases_of(trees, built)
    assert c_verify(gpu_ctx, cases, kind=2)[0] == N.CMTV_EINVAL
    assert c_verify(gpu_ctx, cases, roots=False, want_out=False)[0] == N.CMTV_EINVAL
    rc, st, out, ok = c_verify(gpu_ctx, cases, shared=([cases[0][4]], [0, 0, 0, 1, 0, 0]))
    assert rc == N.CMTV_EINVAL and set(st) == {CANARY} and set(b"".join(out)) == {CANARY} and ok == -7
    # no proofs and no trees: not an error
    assert N.lib().cmtv_merkle_proofs_verify(gpu_ctx.handle, 0, None, None, None, None, None, 0, None, None, None,
                                             None, 0, None, None, None) == N.CMTV_OK
    assert N.lib().cmtv_merkle_proofs(gpu_ctx.handle, 0, None, None, None, None, None, None, None, 0) == N.CMTV_OK


def test_every_building_argument_rule(gpu_ctx):
    """Each rule of the building calls on its own, the context open and every
    other argument good, so the rule itself is what refuses; every output keeps
    its canaries, and the good call then succeeds."""
    lib, h = N.lib(), gpu_ctx.handle
    items = np.frombuffer(b"abcde\0\0\0", np.uint8).copy()
    item_off, tree_off = np.array([0, 3, 5], np.uint32), np.array([0, 2], np.uint32)
    roots, lh, aunts = (np.full(64, CANARY, np.uint8) for _ in range(3))
    aunt_off = np.full(3, 0xA5A5A5A5, np.uint32)
    total = ctypes.c_uint32(0xA5A5A5A5)

    def untouched():
        return all(set(a.tolist()) == {CANARY} for a in (roots, lh, aunts)) and \
            set(aunt_off.tolist()) == {0xA5A5A5A5} and total.value == 0xA5A5A5A5

    names = ["tree_off", "items", "item_off", "roots", "leaf_hashes", "aunt_off", "aunts"]
    good = [_p32(tree_off), _p8(items), _p32(item_off), _p8(roots), _p8(lh), _p32(aunt_off), _p8(aunts), 2]
    for fn in (lib.cmtv_merkle_proofs, lib.cmtv_txs_proofs):
        for k, name in enumerate(names):  # each pointer NULL with a non-zero length behind it
            bad = list(good)
            bad[k] = None
            assert fn(h, 1, *bad) == N.CMTV_EINVAL, name
        assert fn(h, 1, *good[:7], 1) == N.CMTV_EINVAL  # cap_aunts: two leaves, one aunt each
        assert fn(h, 1, _p32(np.array([2, 0], np.uint32)), *good[1:]) == N.CMTV_EINVAL
        assert fn(h, 1, good[0], good[1], _p32(np.array([0, 3, 2], np.uint32)), *good[3:]) == N.CMTV_EINVAL
        assert fn(h, 2**31 + 1, *good) == N.CMTV_EINVAL
        assert untouched()
    data = np.frombuffer(bytes(100) + b"\0\0\0\0", np.uint8).copy()
    n_aunts = sum(P.proof_len(15, i) for i in range(15))
    ps_lh, ps_off, ps_aunts = np.full(32 * 15, CANARY, np.uint8), np.full(16, 0xA5A5A5A5, np.uint32), \
        np.full(32 * n_aunts, CANARY, np.uint8)
    ps = [_p8(roots), _p8(ps_lh), _p32(ps_off), _p8(ps_aunts), n_aunts]

    def part_set(data_p=_p8(data), size=100, part_size=7, total_p=ctypes.byref(total), out=ps):
        return lib.cmtv_part_set_proofs(h, data_p, size, part_size, total_p, *out)

    assert part_set(part_size=0) == N.CMTV_EINVAL
    assert part_set(part_size=2**32 - 99) == N.CMTV_EINVAL  # len + part_size = 2^32 + 1
    assert part_set(data_p=None) == N.CMTV_EINVAL
    assert part_set(total_p=None) == N.CMTV_EINVAL
    for k in range(4):
        bad = list(ps)
        bad[k] = None
        assert part_set(out=bad) == N.CMTV_EINVAL, k
    assert part_set(out=ps[:4] + [n_aunts - 1]) == N.CMTV_EINVAL
    assert untouched() and set(ps_lh.tolist()) == set(ps_aunts.tolist()) == {CANARY} and \
        set(ps_off.tolist()) == {0xA5A5A5A5}
    # the same arguments, nothing wrong: the calls succeed (len + part_size = 2^32 is the last sum allowed)
    assert part_set(part_size=2**32 - 100) == N.CMTV_OK and total.value == 1 and ps_off.tolist()[:2] == [0, 0]
    assert part_set() == N.CMTV_OK and total.value == 15 and ps_off.tolist() == ref_flat([P.parts(bytes(100), 7)])[2]
    assert part_set(size=0, part_size=2**32 - 1, data_p=None, out=[_p8(roots), None, None, None, 0]) == N.CMTV_OK
    assert total.value == 0 and bytes(roots[:32]) == R.EMPTY_ROOT
    assert lib.cmtv_merkle_proofs(h, 1, *good) == N.CMTV_OK
    assert aunt_off.tolist() == [0, 1, 2] and bytes(roots[:32]) == R.root([b"abc", b"de"])


def test_every_verify_argument_rule(gpu_ctx):
    """Each rule of cmtv_merkle_proofs_verify on its own, the context open and
    every other argument good; status, out_hash and all_ok stay untouched, and
    the good call then succeeds."""
    lib, h = N.lib(), gpu_ctx.handle
    items = [b"ab", b"cd"]
    root, proofs = P.proofs_from_byte_slices(items)
    n = 2
    total, index = np.array([2, 2], np.int64), np.array([0, 1], np.int64)
    lh, aunts = _blob([p[2] for p in proofs]), _blob([p[3][0] for p in proofs])
    roots, aunt_off = _blob([root, root]), np.array([0, 1, 2], np.uint32)
    leaves, leaf_off = _blob(items), np.array([0, 2, 4], np.uint32)
    status, out = np.full(n, CANARY, np.uint8), np.full(32 * n, CANARY, np.uint8)
    ok = ctypes.c_int(77)

    def call(**kw):
        a = dict(total=_p64(total), index=_p64(index), lh=_p8(lh), aunt_off=_p32(aunt_off), aunts=_p8(aunts), n_roots=n,
                 roots=_p8(roots), root_idx=None, leaves=_p8(leaves), leaf_off=_p32(leaf_off), kind=N.PROOF_LEAF_ITEM,
                 status=_p8(status), out=_p8(out), n=n)
        a.update(kw)
        return lib.cmtv_merkle_proofs_verify(h, a["n"], a["total"], a["index"], a["lh"], a["aunt_off"], a["aunts"],
                                             a["n_roots"], a["roots"], a["root_idx"], a["leaves"], a["leaf_off"],
                                             a["kind"], a["status"], a["out"], ctypes.byref(ok))

    for name in ("total", "index", "lh", "aunt_off", "aunts", "status"):
        assert call(**{name: None}) == N.CMTV_EINVAL, name
    assert call(leaf_off=None) == N.CMTV_EINVAL         # leaf bytes without their offsets
    assert call(leaves=None) == N.CMTV_EINVAL           # leaf bytes promised by leaf_off
    assert call(roots=None, out=None) == N.CMTV_EINVAL  # neither a root to compare nor a place for the result
    assert call(n_roots=3) == N.CMTV_EINVAL             # root_idx NULL: one root a proof
    assert call(n_roots=1) == N.CMTV_EINVAL
    assert call(root_idx=_p32(np.array([0, 2], np.uint32))) == N.CMTV_EINVAL
    assert call(n_roots=1, root_idx=_p32(np.array([0, 1], np.uint32))) == N.CMTV_EINVAL
    assert call(aunt_off=_p32(np.array([0, 2, 1], np.uint32))) == N.CMTV_EINVAL
    assert call(leaf_off=_p32(np.array([0, 3, 2], np.uint32))) == N.CMTV_EINVAL
    assert call(kind=2) == N.CMTV_EINVAL
    assert call(n=2**31 + 1) == N.CMTV_EINVAL
    assert set(status.tolist()) == {CANARY} and set(out.tolist()) == {CANARY} and ok.value == 77
    # what is allowed: no leaves at all, no roots with out_hash, one shared root, no aunts when none is read
    assert call(leaves=None, leaf_off=None) == N.CMTV_OK and status.tolist() == [0, 0] and ok.value == 1
    assert call(roots=None, n_roots=0) == N.CMTV_OK and bytes(out) == root + root
    assert call(n_roots=1, root_idx=_p32(np.array([0, 0], np.uint32))) == N.CMTV_OK and status.tolist() == [0, 0]
    assert call(aunts=None, aunt_off=_p32(np.array([0, 64, 128], np.uint32))) == N.CMTV_OK
    assert status.tolist() == [P.EEXTRA, P.EEXTRA] and ok.value == 0
    assert call() == N.CMTV_OK and status.tolist() == [0, 0] and bytes(out) == root + root and ok.value == 1
