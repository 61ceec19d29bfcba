"""RFC 6962 merkle roots on the device (cmtv_merkle_root[s],
cmtv_valset_hash[es], cmtv_commit_hash[es]; cometbft_amd/csrc/merkle.hip)
against tests/merkle_ref.py: the generic path over every tree size around
the block size B and the pass thresholds, validator sets and commits of every
key type, flag and size class, the host-encoded route of a long signature, a
call large enough to be cut into runs, the Python wrappers, pinned argument
memory, CMTV_FAULT_AT and the argument rules that need an open context."""
import ctypes
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
import merkle_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(ROOT, "cometbft_amd", "csrc", "merkle.h")) as _f:
    B = int(re.search(r"#define\s+CMTV_MERKLE_BLOCK_LEAVES\s+(\d+)", _f.read()).group(1))
CANARY = 0xA5
_p8, _p32 = T._p8, T._p32
_p64 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))  # noqa: E731
_pi32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))  # noqa: E731


def _offsets(lens):
    off = np.zeros(len(lens) + 1, np.uint32)
    if len(lens):
        off[1:] = np.cumsum(lens)
    return off


def _blob(parts):
    return np.frombuffer(b"".join(parts) + b"\0\0\0\0", np.uint8).copy()


def _out(n):
    return (ctypes.c_uint8 * (32 * max(n, 1)))(*([CANARY] * (32 * max(n, 1))))


def _split(out, n):
    raw = bytes(out)
    return [raw[32 * i: 32 * i + 32] for i in range(n)]


def c_merkle_roots(ctx, trees):
    items = [it for t in trees for it in t]
    out = _out(len(trees))
    rc = N.lib().cmtv_merkle_roots(ctx.handle, len(trees), _p32(_offsets([len(t) for t in trees])), _p8(_blob(items)),
                                   _p32(_offsets([len(i) for i in items])), out)
    assert rc == N.CMTV_OK, rc
    return _split(out, len(trees))


def c_merkle_root(ctx, items):
    out = _out(1)
    rc = N.lib().cmtv_merkle_root(ctx.handle, len(items), _p8(_blob(items)), _p32(_offsets([len(i) for i in items])),
                                  out)
    assert rc == N.CMTV_OK, rc
    return bytes(out)


class ValSet:
    """A validator set in the C struct-of-arrays form, and its reference root."""

    def __init__(self, keys, powers, types):
        self.keys, self.powers, self.types = list(keys), list(powers), list(types)
        self.pk = _blob(self.keys)
        self.off = _offsets([len(k) for k in self.keys])
        self.vp = np.array(self.powers + [0], np.int64)
        self.kt = np.array(self.types + [0], np.uint8)
        self.c = N.cmtv_valset(n_vals=len(self.keys), pubkeys=_p8(self.pk), pk_off=_p32(self.off),
                               voting_power=_p64(self.vp), addrs=None, proposer_priority=None)

    def ref(self):
        return R.valset_hash(list(zip(self.types, self.keys, self.powers)))

    def hash(self, ctx, key_types=True):
        out = _out(1)
        rc = N.lib().cmtv_valset_hash(ctx.handle, ctypes.byref(self.c), _p8(self.kt) if key_types else None, out)
        assert rc == N.CMTV_OK, rc
        return bytes(out)


def gen_valset(rng, n, kind):
    """kind: 'ed', 'secp' or 'mixed'; powers include 0 and a negative one."""
    types = [{"ed": 0, "secp": 1}.get(kind, rng.randrange(2)) for _ in range(n)]
    keys = [rng.randbytes(33 if t else 32) for t in types]
    powers = [rng.choice([0, -5, 1, 127, 128, rng.randrange(1, 2**62)]) for _ in range(n)]
    if n > 2:
        powers[1], powers[2] = 0, -1
    return ValSet(keys, powers, types)


def c_valset_hashes(ctx, sets, key_types=True):
    arr = (N.cmtv_valset * len(sets))(*[s.c for s in sets])
    kts = (ctypes.POINTER(ctypes.c_uint8) * len(sets))(*[_p8(s.kt) for s in sets]) if key_types else None
    out = _out(len(sets))
    rc = N.lib().cmtv_valset_hashes(ctx.handle, len(sets), arr, kts, out)
    assert rc == N.CMTV_OK, rc
    return _split(out, len(sets))


class Commit:
    """A commit's signatures in the C struct-of-arrays form. put: where the
    arrays live (a function from a numpy array to the copy the struct points at)."""

    def __init__(self, sigs, put=lambda a: a):
        self.rows = list(sigs)  # (flag, addr20, seconds, nanos, sig)
        n = len(self.rows)
        self.flags = put(np.array([r[0] for r in self.rows] + [0], np.uint8))
        self.addrs = put(_blob([r[1] for r in self.rows]))
        self.sec = put(np.array([r[2] for r in self.rows] + [0], np.int64))
        self.nanos = put(np.array([r[3] for r in self.rows] + [0], np.int32))
        self.sigs = put(_blob([r[4] for r in self.rows]))
        self.off = put(_offsets([len(r[4]) for r in self.rows]))
        self.c = N.cmtv_commit(height=1, round=0, n_sigs=n, flags=_p8(self.flags), ts_seconds=_p64(self.sec),
                               ts_nanos=_pi32(self.nanos), sigs=_p8(self.sigs), sig_off=_p32(self.off),
                               val_addrs=_p8(self.addrs))

    def ref(self):
        return R.commit_hash(self.rows)

    def hash(self, ctx):
        out = _out(1)
        rc = N.lib().cmtv_commit_hash(ctx.handle, ctypes.byref(self.c), out)
        assert rc == N.CMTV_OK, rc
        return bytes(out)


def gen_sig_row(rng, flag=None, sig_len=64):
    flag = rng.choice([R.FLAG_COMMIT] * 6 + [R.FLAG_NIL, R.FLAG_ABSENT]) if flag is None else flag
    if flag == R.FLAG_ABSENT:  # NewCommitSigAbsent: the Go zero time, no signature
        return (flag, bytes(20), R.GO_ZERO_TIME_SECONDS, 0, b"")
    return (flag, rng.randbytes(20), 1_700_000_000 + rng.randrange(10**6), rng.choice([0, rng.randrange(10**9)]),
            rng.randbytes(sig_len))


def gen_commit(rng, n, **kw):
    rows = [gen_sig_row(rng) for _ in range(n)]
    if n >= 3:  # every flag present
        rows[0], rows[1], rows[2] = (gen_sig_row(rng, f) for f in (R.FLAG_COMMIT, R.FLAG_NIL, R.FLAG_ABSENT))
    return Commit(rows, **kw)


def c_commit_hashes(ctx, commits):
    arr = (N.cmtv_commit * len(commits))(*[c.c for c in commits])
    out = _out(len(commits))
    rc = N.lib().cmtv_commit_hashes(ctx.handle, len(commits), arr, out)
    assert rc == N.CMTV_OK, rc
    return _split(out, len(commits))


# ------------------------------------------------------------------ generic path
def test_kat_file(gpu_ctx):
    with open(os.path.join(ROOT, "tests", "golden", "merkle_kat.json")) as f:
        kat = json.load(f)
    trees = [[bytes.fromhex(i) for i in t["items"]] for t in kat["trees"]]
    want = [bytes.fromhex(t["root"]) for t in kat["trees"]]
    trees.append([bytes.fromhex(x) for x in kat["header_hash"]["leaves"]])
    want.append(bytes.fromhex(kat["header_hash"]["root"]))
    for c in kat["rfc6962"]:
        if c["kind"] == "tree":
            trees.append([bytes.fromhex(i) for i in c["items"]])
            want.append(bytes.fromhex(c["want"]))
        elif c["kind"] == "leaf":  # a one-leaf tree is its leaf hash
            trees.append([bytes.fromhex(c["item"])])
            want.append(bytes.fromhex(c["want"]))
    assert c_merkle_roots(gpu_ctx, trees) == want
    assert [c_merkle_root(gpu_ctx, t) for t in trees] == want


def test_every_tree_size_in_one_call(gpu_ctx):
    rng = random.Random(31)
    trees = [[rng.randbytes(rng.randrange(131)) for _ in range(n)] for n in range(2 * B + 3)]
    got = c_merkle_roots(gpu_ctx, trees)
    for n, t in enumerate(trees):
        assert got[n] == R.root(t), n


@pytest.mark.parametrize("n", [0, 1, 2, 3, B - 1, B, B + 1, 2 * B + 1, 10_000])
def test_single_tree(gpu_ctx, n):
    rng = random.Random(32 + n)
    items = [rng.randbytes(rng.randrange(131)) for _ in range(n)]
    assert c_merkle_root(gpu_ctx, items) == R.root(items)


def test_third_pass(gpu_ctx):
    """B^2 + 1 one-byte items: the smallest tree whose block nodes need a third pass."""
    items = [bytes([i * 7 & 0xFF]) for i in range(B * B + 1)]
    assert c_merkle_root(gpu_ctx, items) == R.root(items)


# ------------------------------------------------------------------ validator sets
@pytest.mark.parametrize("n", [1, 2, 150, B + 1, 10_000])
def test_valset_hash(gpu_ctx, n):
    rng = random.Random(40 + n)
    ed = gen_valset(rng, n, "ed")
    want = ed.ref()
    assert ed.hash(gpu_ctx, key_types=False) == want  # key_types NULL: every key Ed25519
    assert ed.hash(gpu_ctx, key_types=True) == want
    for kind in ("secp", "mixed"):
        vs = gen_valset(rng, n, kind)
        assert vs.hash(gpu_ctx) == vs.ref(), kind


def test_valset_hashes_many_sets(gpu_ctx):
    rng = random.Random(41)
    sets = [gen_valset(rng, 150, rng.choice(["ed", "mixed"])) for _ in range(300)]
    sets[7] = ValSet([], [], [])
    sets[200] = gen_valset(rng, B + 3, "mixed")
    got = c_valset_hashes(gpu_ctx, sets)
    assert got == [s.ref() for s in sets]
    assert got[7] == R.EMPTY_ROOT
    for i in (0, 7, 200, 299):
        assert sets[i].hash(gpu_ctx) == got[i]
    # the array of key-type arrays may be NULL, or hold NULL for a set
    eds = [gen_valset(rng, 5, "ed") for _ in range(3)]
    assert c_valset_hashes(gpu_ctx, eds, key_types=False) == [s.ref() for s in eds]


# ------------------------------------------------------------------ commits
@pytest.mark.parametrize("n", [1, 3, 150, B + 1, 10_000])
def test_commit_hash(gpu_ctx, n):
    cm = gen_commit(random.Random(50 + n), n)
    assert cm.hash(gpu_ctx) == cm.ref()


def test_commit_hash_edge_fields(gpu_ctx):
    """Every flag value class, signature length 0..64 and timestamp edge."""
    rng = random.Random(51)
    rows = []
    for flag in (0, 1, 2, 3, 127, 128, 255):
        for sec in (0, R.GO_ZERO_TIME_SECONDS, 2**31, R.LAST_VALID_SECOND):
            for nanos in (0, 1, 999_999_999):
                rows.append((flag, rng.randbytes(20), sec, nanos, rng.randbytes(rng.choice([0, 1, 63, 64]))))
    rows += [(2, rng.randbytes(20), 1_700_000_000, 5, rng.randbytes(sl)) for sl in range(65)]
    cm = Commit(rows)
    assert cm.hash(gpu_ctx) == cm.ref()


def test_commit_with_a_long_signature_takes_the_host_encoded_route(gpu_ctx):
    rng = random.Random(52)
    rows = [gen_sig_row(rng) for _ in range(150)]
    rows[77] = gen_sig_row(rng, R.FLAG_COMMIT, sig_len=65)
    wide = Commit(rows)
    assert wide.hash(gpu_ctx) == wide.ref()
    # beside commits that take the device builder, in one call
    others = [gen_commit(rng, 20), gen_commit(rng, 0), gen_commit(rng, B + 1)]
    mix = [others[0], wide, others[1], others[2], Commit([gen_sig_row(rng, 2, sig_len=200)])]
    assert c_commit_hashes(gpu_ctx, mix) == [c.ref() for c in mix]


def test_commit_hashes_many_commits(gpu_ctx):
    rng = random.Random(53)
    commits = [gen_commit(rng, 150) for _ in range(300)]
    got = c_commit_hashes(gpu_ctx, commits)
    assert got == [c.ref() for c in commits]
    assert commits[5].hash(gpu_ctx) == got[5]


def test_a_call_cut_into_runs(gpu_ctx):
    """2,500 commits of 150 signatures stage about 38 MB: more than one run
    (merkle.cpp kRunBytes). The structs share five commits' arrays."""
    rng = random.Random(54)
    base = [gen_commit(rng, 150) for _ in range(5)]
    refs = [c.ref() for c in base]
    pick = [rng.randrange(5) for _ in range(2500)]
    got = c_commit_hashes(gpu_ctx, [base[k] for k in pick])
    assert got == [refs[k] for k in pick]


def test_all_absent_commit_needs_no_addresses(gpu_ctx):
    cm = Commit([gen_sig_row(random.Random(55), R.FLAG_ABSENT) for _ in range(7)])
    want = cm.ref()
    cm.c.val_addrs = None
    assert cm.hash(gpu_ctx) == want


# ------------------------------------------------------------------ properties
def test_one_differing_byte_changes_the_root(gpu_ctx):
    rng = random.Random(60)
    vs = gen_valset(rng, 150, "mixed")
    root = vs.hash(gpu_ctx)
    key = bytearray(vs.keys[33])
    key[5] ^= 1
    k2 = ValSet(vs.keys[:33] + [bytes(key)] + vs.keys[34:], vs.powers, vs.types)
    p2 = ValSet(vs.keys, vs.powers[:90] + [vs.powers[90] + 1] + vs.powers[91:], vs.types)
    cm = Commit([gen_sig_row(rng, R.FLAG_COMMIT) for _ in range(150)])
    croot = cm.hash(gpu_ctx)

    def changed(i, field, value):
        row = cm.rows[i][:field] + (value,) + cm.rows[i][field + 1:]
        return Commit(cm.rows[:i] + [row] + cm.rows[i + 1:])

    sig = bytearray(cm.rows[149][4])
    sig[63] ^= 0x80
    # one flag, one nanos value, one signature bit
    variants = [changed(10, 0, R.FLAG_NIL), changed(20, 3, cm.rows[20][3] ^ 1), changed(149, 4, bytes(sig))]
    roots = [k2.hash(gpu_ctx), p2.hash(gpu_ctx)] + [v.hash(gpu_ctx) for v in variants]
    for r, v in zip(roots, [k2, p2] + variants):
        assert r == v.ref()
    assert all(r != root for r in roots[:2]) and all(r != croot for r in roots[2:])
    assert len(set(roots)) == 5


def test_python_wrappers_agree_with_the_c_calls(gpu_ctx):
    rng = random.Random(61)
    trees = [[rng.randbytes(rng.randrange(40)) for _ in range(n)] for n in (0, 1, 5, B + 2)]
    assert T.merkle_roots(trees, gpu_ctx) == c_merkle_roots(gpu_ctx, trees) == [R.root(t) for t in trees]
    assert T.merkle_root(trees[2], gpu_ctx) == R.root(trees[2])
    assert T.merkle_root([], gpu_ctx) == R.EMPTY_ROOT and T.merkle_roots([], gpu_ctx) == []
    sets = []
    for kinds in (["ed25519"] * 9, ["secp256k1"] * 4, ["ed25519", "secp256k1", "ed25519"]):
        sets.append(T.ValidatorSet([T.Validator(rng.randbytes(33 if k == "secp256k1" else 32), rng.choice([0, -3, 77]),
                                                key_type=k) for k in kinds]))
    want = [R.root([v.bytes() for v in s.validators]) for s in sets]
    assert want == [R.valset_hash([(N.KEY_TYPES[v.key_type], v.pub_key, v.voting_power) for v in s.validators])
                    for s in sets]
    assert [s.hash(gpu_ctx) for s in sets] == want
    assert T.valset_hashes(sets, gpu_ctx) == want
    import cometbft_amd

    assert cometbft_amd.valset_hashes is T.valset_hashes and cometbft_amd.commit_hashes is T.commit_hashes
    assert cometbft_amd.merkle_root is T.merkle_root and cometbft_amd.merkle_roots is T.merkle_roots
    commits = []
    for n in (0, 4, 150):
        sigs = [T.CommitSig(f, a, (s, ns), sg) for f, a, s, ns, sg in (gen_sig_row(rng) for _ in range(n))]
        commits.append(T.Commit(3, 0, T.BlockID(), sigs))
    want = [R.commit_hash([(s.block_id_flag, s.validator_address, s.timestamp[0], s.timestamp[1], s.signature)
                           for s in c.signatures]) for c in commits]
    assert [c.hash(gpu_ctx) for c in commits] == want
    assert T.commit_hashes(commits, gpu_ctx) == want


def test_arguments_in_pinned_memory(gpu_ctx):
    rng = random.Random(62)
    block = gpu_ctx.alloc_pinned(1 << 20)
    try:
        arena = T._Arena(block)
        cms = [gen_commit(rng, n, put=arena.put) for n in (150, B + 1)]
        assert c_commit_hashes(gpu_ctx, cms) == [c.ref() for c in cms]
        items = [rng.randbytes(rng.randrange(100)) for _ in range(300)]
        blob, off = arena.put(_blob(items)), arena.put(_offsets([len(i) for i in items]))
        out = _out(1)
        assert N.lib().cmtv_merkle_root(gpu_ctx.handle, len(items), _p8(blob), _p32(off), out) == N.CMTV_OK
        assert bytes(out) == R.root(items)
    finally:
        block.free()


def test_fault_at_fails_the_call_and_the_next_one_succeeds():
    """CMTV_FAULT_AT fails a launch on the host without running it."""
    from conftest import _env_ctx

    ctx = _env_ctx(CMTV_FAULT_AT=1)
    try:
        cm = gen_commit(random.Random(63), 150)
        out = _out(1)
        assert N.lib().cmtv_commit_hash(ctx.handle, ctypes.byref(cm.c), out) == N.CMTV_EHIP
        assert set(bytes(out)) == {CANARY}
        assert cm.hash(ctx) == cm.ref()
        assert ctx.stats()["faults_injected"] == 1
    finally:
        ctx.close()


# ------------------------------------------------------------------ argument rules
def test_argument_errors_write_nothing(gpu_ctx):
    lib, h = N.lib(), gpu_ctx.handle
    rng = random.Random(64)
    out = _out(4)

    def untouched():
        return set(bytes(out)) == {CANARY}

    item, off = _blob([b"abc", b"de"]), _offsets([3, 2])
    tree_off = _offsets([2])
    assert lib.cmtv_merkle_roots(h, 1, None, _p8(item), _p32(off), out) == N.CMTV_EINVAL
    assert lib.cmtv_merkle_roots(h, 1, _p32(tree_off), _p8(item), None, out) == N.CMTV_EINVAL
    assert lib.cmtv_merkle_roots(h, 1, _p32(tree_off), None, _p32(off), out) == N.CMTV_EINVAL
    assert lib.cmtv_merkle_roots(h, 1, _p32(tree_off), _p8(item), _p32(off), None) == N.CMTV_EINVAL
    assert lib.cmtv_merkle_root(h, 2, _p8(item), None, out) == N.CMTV_EINVAL
    down = np.array([0, 3, 2], np.uint32)
    assert lib.cmtv_merkle_root(h, 2, _p8(item), _p32(down), out) == N.CMTV_EINVAL
    assert lib.cmtv_merkle_roots(h, 2, _p32(np.array([0, 2, 1], np.uint32)), _p8(item), _p32(off), out) == N.CMTV_EINVAL
    assert untouched()

    good = gen_valset(rng, 4, "mixed")
    assert lib.cmtv_valset_hash(h, None, None, out) == N.CMTV_EINVAL
    assert lib.cmtv_valset_hash(h, ctypes.byref(good.c), _p8(good.kt), None) == N.CMTV_EINVAL
    for field in ("pubkeys", "pk_off", "voting_power"):
        bad = gen_valset(rng, 4, "ed")
        setattr(bad.c, field, None)
        assert lib.cmtv_valset_hash(h, ctypes.byref(bad.c), None, out) == N.CMTV_EINVAL, field
    for types in ([0, R.KEY_SR25519, 0, 0], [0, 0, 0, 3], [255, 0, 0, 0]):
        bad = ValSet(good.keys, good.powers, types)
        assert lib.cmtv_valset_hash(h, ctypes.byref(bad.c), _p8(bad.kt), out) == N.CMTV_EINVAL, types
    for keys in ([b"", bytes(32)], [bytes(32), bytes(65)]):
        bad = ValSet(keys, [1, 1], [0, 0])
        assert lib.cmtv_valset_hash(h, ctypes.byref(bad.c), None, out) == N.CMTV_EINVAL
    bad = gen_valset(rng, 3, "ed")
    bad.off[2] = bad.off[1] - 1
    assert lib.cmtv_valset_hash(h, ctypes.byref(bad.c), None, out) == N.CMTV_EINVAL
    # one bad set fails the whole plural call
    sets = [good, ValSet([bytes(32)], [1], [R.KEY_SR25519]), good]
    arr = (N.cmtv_valset * 3)(*[s.c for s in sets])
    kts = (ctypes.POINTER(ctypes.c_uint8) * 3)(*[_p8(s.kt) for s in sets])
    assert lib.cmtv_valset_hashes(h, 3, arr, kts, out) == N.CMTV_EINVAL
    assert lib.cmtv_valset_hashes(h, 3, None, kts, out) == N.CMTV_EINVAL
    assert untouched()

    assert lib.cmtv_commit_hash(h, None, out) == N.CMTV_EINVAL
    cm = gen_commit(rng, 5)
    assert lib.cmtv_commit_hash(h, ctypes.byref(cm.c), None) == N.CMTV_EINVAL
    for field in ("flags", "ts_seconds", "ts_nanos", "sig_off", "sigs", "val_addrs"):
        bad = gen_commit(rng, 5)
        setattr(bad.c, field, None)
        assert lib.cmtv_commit_hash(h, ctypes.byref(bad.c), out) == N.CMTV_EINVAL, field
    for sec, nanos in [(R.GO_ZERO_TIME_SECONDS - 1, 0), (R.LAST_VALID_SECOND + 1, 0), (0, -1), (0, 10**9)]:
        bad = Commit([gen_sig_row(rng, 2), (2, bytes(20), sec, nanos, bytes(64))])
        assert lib.cmtv_commit_hash(h, ctypes.byref(bad.c), out) == N.CMTV_EINVAL, (sec, nanos)
    bad = gen_commit(rng, 5)
    bad.off[3] = bad.off[2] - 1
    assert lib.cmtv_commit_hash(h, ctypes.byref(bad.c), out) == N.CMTV_EINVAL
    arr = (N.cmtv_commit * 2)(cm.c, bad.c)
    assert lib.cmtv_commit_hashes(h, 2, arr, out) == N.CMTV_EINVAL
    assert lib.cmtv_commit_hashes(h, 2, None, out) == N.CMTV_EINVAL
    assert untouched()
    # n = 0 is not an error and writes nothing
    assert lib.cmtv_merkle_roots(h, 0, None, None, None, None) == N.CMTV_OK
    assert lib.cmtv_valset_hashes(h, 0, None, None, None) == N.CMTV_OK
    assert lib.cmtv_commit_hashes(h, 0, None, None) == N.CMTV_OK
