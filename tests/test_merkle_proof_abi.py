"""CPU tests of the merkle proof additions to the C ABI: the two host-only
length calls against tests/merkle_proof_ref.py, every argument rule that is
decided before the context is looked at (a NULL context is CMTV_EINVAL like
any other bad argument, so each rule is tried with outputs full of canaries,
which must stay), that the addition left the ABI version and cmtv_stats
alone, and Proof.validate_basic on the reference's own cases. (The same
rules with an open context, where a good call succeeds, are in
tests/test_merkle_proof_gpu.py.)"""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

from cometbft_amd import _native as N
from cometbft_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import merkle_proof_ref as P  # noqa: E402

CANARY = 0xA5
_p8, _p32 = T._p8, T._p32


def _canary(n):
    return np.full(max(n, 1), CANARY, np.uint8)


def test_proof_len_matches_the_recursive_count():
    lib = N.lib()
    for n in range(1, 601):
        assert [lib.cmtv_merkle_proof_len(n, i) for i in range(n)] == [P.proof_len(n, i) for i in range(n)], n
    rng = random.Random(71)
    for total in (2**62, 2**62 + 1, 2**63 - 1):
        for index in [0, 1, total - 1, total // 2, 2**61, 2**62 - 1] + [rng.randrange(total) for _ in range(50)]:
            if index < total:
                assert lib.cmtv_merkle_proof_len(total, index) == P.proof_len(total, index), (total, index)
    assert max(lib.cmtv_merkle_proof_len(2**63 - 1, i) for i in (0, 2**62 - 1, 2**62)) == 63
    for total, index in [(0, 0), (1, 1), (5, 5), (5, 6), (2**63 - 1, 2**63 - 1), (7, 2**64 - 1)]:
        assert lib.cmtv_merkle_proof_len(total, index) == -1


def test_proofs_len_sums_every_leaf_of_every_tree():
    lib = N.lib()
    sizes = [0, 1, 2, 3, 0, 5, 255, 256, 257, 1000, 0]
    off = np.zeros(len(sizes) + 1, np.uint32)
    off[1:] = np.cumsum(sizes)
    off += 7  # the first tree need not start at item 0
    got = ctypes.c_uint64(123)
    assert lib.cmtv_merkle_proofs_len(len(sizes), _p32(off), ctypes.byref(got)) == N.CMTV_OK
    assert got.value == sum(P.proof_len(n, i) for n in sizes for i in range(n))
    assert lib.cmtv_merkle_proofs_len(0, None, ctypes.byref(got)) == N.CMTV_OK and got.value == 0
    got = ctypes.c_uint64(123)
    assert lib.cmtv_merkle_proofs_len(2, None, ctypes.byref(got)) == N.CMTV_EINVAL
    assert lib.cmtv_merkle_proofs_len(2, _p32(off), None) == N.CMTV_EINVAL
    assert lib.cmtv_merkle_proofs_len(2, _p32(np.array([0, 3, 2], np.uint32)), ctypes.byref(got)) == N.CMTV_EINVAL
    assert got.value == 123


def test_building_calls_refuse_bad_arguments_and_write_nothing():
    lib = N.lib()
    items = np.frombuffer(b"abcde\0\0\0", np.uint8).copy()
    item_off = np.array([0, 3, 5], np.uint32)
    tree_off = np.array([0, 2], np.uint32)
    roots, lh, aunts = _canary(64), _canary(64), _canary(64)
    aunt_off = np.full(3, 0xA5A5A5A5, np.uint32)
    total = ctypes.c_uint32(0xA5A5A5A5)

    def untouched():
        return all(set(a.tolist()) == {CANARY} for a in (roots, lh, aunts)) and \
            set(aunt_off.tolist()) == {0xA5A5A5A5} and total.value == 0xA5A5A5A5

    good = [_p32(tree_off), _p8(items), _p32(item_off), _p8(roots), _p8(lh), _p32(aunt_off), _p8(aunts), 2]
    for fn in (lib.cmtv_merkle_proofs, lib.cmtv_txs_proofs):
        assert fn(None, 1, *good) == N.CMTV_EINVAL  # no context
        for k in range(7):  # each pointer NULL with a non-zero length
            bad = list(good)
            bad[k] = None
            assert fn(None, 1, *bad) == N.CMTV_EINVAL, k
        assert fn(None, 1, *good[:7], 1) == N.CMTV_EINVAL  # cap_aunts too small: two leaves, one aunt each
        assert fn(None, 1, _p32(np.array([2, 0], np.uint32)), *good[1:]) == N.CMTV_EINVAL
        assert fn(None, 1, good[0], good[1], _p32(np.array([0, 3, 2], np.uint32)), *good[3:]) == N.CMTV_EINVAL
        assert fn(None, 2**31 + 1, *good) == N.CMTV_EINVAL
    data = np.frombuffer(bytes(100) + b"\0\0\0\0", np.uint8).copy()
    ps = [_p8(roots), _p8(lh), _p32(aunt_off), _p8(aunts), 64]
    assert lib.cmtv_part_set_proofs(None, _p8(data), 100, 7, ctypes.byref(total), *ps) == N.CMTV_EINVAL
    assert lib.cmtv_part_set_proofs(None, _p8(data), 100, 0, ctypes.byref(total), *ps) == N.CMTV_EINVAL
    assert lib.cmtv_part_set_proofs(None, _p8(data), 100, 2**32 - 99, ctypes.byref(total), *ps) == N.CMTV_EINVAL
    assert lib.cmtv_part_set_proofs(None, _p8(data), 2**32 - 1, 2, ctypes.byref(total), *ps) == N.CMTV_EINVAL
    assert lib.cmtv_part_set_proofs(None, None, 100, 7, ctypes.byref(total), *ps) == N.CMTV_EINVAL
    assert lib.cmtv_part_set_proofs(None, _p8(data), 100, 7, None, *ps) == N.CMTV_EINVAL
    assert untouched()


def test_verify_call_refuses_bad_arguments_and_writes_nothing():
    lib = N.lib()
    n = 2
    total, index = np.array([2, 2], np.int64), np.array([0, 1], np.int64)
    i64 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))  # noqa: E731
    lh, aunts, roots = np.zeros(64, np.uint8), np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    aunt_off = np.array([0, 1, 2], np.uint32)
    leaves, leaf_off = np.zeros(8, np.uint8), np.array([0, 2, 4], np.uint32)
    status, out = _canary(n), _canary(32 * n)
    ok = ctypes.c_int(77)

    def call(**kw):
        a = dict(total=i64(total), index=i64(index), lh=_p8(lh), aunt_off=_p32(aunt_off), aunts=_p8(aunts), n_roots=n,
                 roots=_p8(roots), root_idx=None, leaves=_p8(leaves), leaf_off=_p32(leaf_off), kind=N.PROOF_LEAF_ITEM,
                 status=_p8(status), out=_p8(out), n=n)
        a.update(kw)
        return lib.cmtv_merkle_proofs_verify(None, a["n"], a["total"], a["index"], a["lh"], a["aunt_off"], a["aunts"],
                                             a["n_roots"], a["roots"], a["root_idx"], a["leaves"], a["leaf_off"],
                                             a["kind"], a["status"], a["out"], ctypes.byref(ok))

    assert call() == N.CMTV_EINVAL  # no context
    for name in ("total", "index", "lh", "aunt_off", "aunts", "status", "leaf_off"):
        assert call(**{name: None}) == N.CMTV_EINVAL, name
    assert call(leaves=None) == N.CMTV_EINVAL          # leaf bytes promised by leaf_off
    assert call(roots=None, out=None) == N.CMTV_EINVAL  # neither a root to compare nor a place for the result
    assert call(n_roots=3) == N.CMTV_EINVAL             # root_idx NULL: one root a proof
    assert call(root_idx=_p32(np.array([0, 2], np.uint32))) == N.CMTV_EINVAL
    assert call(aunt_off=_p32(np.array([0, 2, 1], np.uint32))) == N.CMTV_EINVAL
    assert call(leaf_off=_p32(np.array([0, 3, 2], np.uint32))) == N.CMTV_EINVAL
    assert call(kind=2) == N.CMTV_EINVAL
    assert call(n=2**31 + 1) == N.CMTV_EINVAL
    assert set(status.tolist()) == {CANARY} and set(out.tolist()) == {CANARY} and ok.value == 77


def test_abi_version_and_stats_layout_unchanged():
    assert N.lib().cmtv_abi_version() == 11
    assert ctypes.sizeof(N.cmtv_stats) == 200
    with open(os.path.join(ROOT, "include", "cmtverify.h")) as f:
        assert "#define CMTV_ABI_VERSION 11" in f.read()
    assert [N.PROOF_OK, N.PROOF_ENEGTOTAL, N.PROOF_ENEGINDEX, N.PROOF_ELEAF, N.PROOF_EINDEX, N.PROOF_EEXTRA,
            N.PROOF_EMISSING, N.PROOF_EROOT] == [P.OK, P.ENEGTOTAL, P.ENEGINDEX, P.ELEAF, P.EINDEX, P.EEXTRA,
                                                 P.EMISSING, P.EROOT] == list(range(8))


# crypto/merkle/proof_test.go TestProofValidateBasic: apple / watermelon / kiwi
VALIDATE_BASIC = [
    ("Good", lambda p: None, None),
    ("Negative Total", lambda p: setattr(p, "total", -1), "negative Total"),
    ("Negative Index", lambda p: setattr(p, "index", -1), "negative Index"),
    ("Invalid LeafHash", lambda p: setattr(p, "leaf_hash", bytes(10)), "expected LeafHash size to be 32, got 10"),
    ("Too many Aunts", lambda p: setattr(p, "aunts", [bytes(32)] * (T.MAX_AUNTS + 1)),
     "expected no more than 100 aunts, got 101"),
    ("Invalid Aunt", lambda p: p.aunts.__setitem__(0, bytes(10)), "expected Aunts#0 size to be 32, got 10"),
]


@pytest.mark.parametrize("name,malleate,want", VALIDATE_BASIC, ids=[c[0] for c in VALIDATE_BASIC])
def test_validate_basic(name, malleate, want):
    items = [b"apple", b"watermelon", b"kiwi"]
    _, proofs = P.proofs_from_byte_slices(items)
    p = T.Proof(*proofs[0][:3], list(proofs[0][3]))
    malleate(p)
    assert P.validate_basic(p.total, p.index, p.leaf_hash, p.aunts) == want
    if want is None:
        p.validate_basic()
    else:
        with pytest.raises(ValueError) as e:
            p.validate_basic()
        assert str(e.value) == want
