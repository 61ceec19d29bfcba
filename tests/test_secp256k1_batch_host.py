"""The batched registered-key secp256k1 device code on the CPU:
tests/host/secpbatchcheck.cpp compiles cometbft_amd/csrc/secp256k1.h with
CMTV_HD = inline and the headers' operand-bound assertions on and runs
secp_verify_keyed_batch_lane<KB> (the function
k_verify_secp256k1_keyed_batch<KB> calls: KB signatures per lane sharing one
inversion mod n) laid out as the kernel lays signatures out over its lanes.

  * the registered-key corpus (776 vectors, 95 keys) in two fixed
    permutations, KB = 4 and 8: every verdict equals secp_verify_keyed_one's
    and the corpus's, and every invalid category shares a lane with a valid
    signature
  * directed lanes: s = 0 and s = n in the first, a middle and the last
    round, r = 0, high-S, a rejected key, a key index out of range, one
    active round, s = 1 throughout
  * the same program, AddressSanitizer + UBSan
"""
import os
import random
import struct
import subprocess
import sys

import numpy as np
import pytest

from tests.host import hostbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import secp256k1_keyed_vectors as V  # noqa: E402
import secp256k1_ref as S  # noqa: E402

SRC = os.path.join(ROOT, "tests", "host", "secpbatchcheck.cpp")
BIN = os.path.join(ROOT, "build", "secpbatchcheck")
BIN_SAN = os.path.join(ROOT, "build", "secpbatchcheck_san")
KBS = (4, 8)


@pytest.fixture(scope="module")
def check():
    return hostbuild.build(SRC, BIN, ["-std=c++17"])


@pytest.fixture(scope="module")
def corpus():
    keys, idx, vecs = V.corpus_indexed()
    entries = [(k, bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"])) for k, v in zip(idx, vecs)]
    return keys, entries, [int(v["valid"]) for v in vecs], [v["cat"] for v in vecs]


def run(binary, kb, lanes, keys, entries):
    """(batched verdicts, secp_verify_keyed_one's verdicts) for entries
    [(key_idx, sig, msg)] over `lanes` lanes of kb rounds per launch."""
    buf = [struct.pack("<I", len(keys)), b"".join(keys), struct.pack("<I", len(entries))]
    for k, sig, m in entries:
        buf += [struct.pack("<I", k), sig, struct.pack("<I", len(m)), m]
    r = subprocess.run([binary, str(kb), str(lanes)], input=b"".join(buf), capture_output=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stderr[-800:])
    n = len(entries)
    assert len(r.stdout) == 2 * n
    return np.frombuffer(r.stdout[:n], np.uint8), np.frombuffer(r.stdout[n:], np.uint8)


def lane_of(i, kb, lanes):
    """The (launch, lane) that holds signature i."""
    return i // (lanes * kb), i % lanes


def assert_corpus(binary, corpus, kb, seed):
    keys, entries, valid, cats = corpus
    n = len(entries)
    perm = list(range(n))
    random.Random(seed).shuffle(perm)
    # 64 lanes: launches of 64 kb signatures, the last one partial with wholly inactive rounds
    lanes = 64
    got, one = run(binary, kb, lanes, keys, [entries[p] for p in perm])
    exp = np.array([valid[p] for p in perm], np.uint8)
    bad = np.nonzero((got != exp) | (one != exp))[0]
    assert bad.size == 0, [(int(i), cats[perm[int(i)]], int(got[i]), int(one[i])) for i in bad[:10]]
    # the layout put every invalid category beside a valid signature in one lane
    holds_valid = {lane_of(i, kb, lanes) for i in range(n) if exp[i]}
    shared = {cats[perm[i]] for i in range(n) if not exp[i] and lane_of(i, kb, lanes) in holds_valid}
    assert shared == {cats[i] for i in range(n) if not valid[i]}


@pytest.mark.parametrize("kb", KBS)
def test_corpus_two_permutations(check, corpus, kb):
    assert len(corpus[1]) == 776 and len(corpus[0]) == 95
    for seed in (0xB47C4, 0xB47C8):
        assert_corpus(check, corpus, kb, seed)


def directed_lanes(kb):
    """(keys, entries, expected): lanes of kb rounds, one per directed case
    (lanes = number of cases, so case c is lane c and its round r is entry
    c + r * lanes)."""
    rng = random.Random(0xD1EC7)
    privs = [rng.randbytes(32) for _ in range(3)]
    keys = [S.pubkey_from_priv(p) for p in privs]
    rejected = bytes([4]) + keys[0][1:]
    keys.append(rejected)
    n_int = S.N

    def good(j, tag):
        m = b"batch lane %d %s" % (j, tag)
        return (j % 3, S.sign(privs[j % 3], m), m, 1)

    def with_s(sig, s_bytes):
        return sig[:32] + s_bytes

    lanes = []
    zero, n_bytes = bytes(32), n_int.to_bytes(32, "big")
    for name, s_bytes in ((b"s0", zero), (b"sn", n_bytes)):
        for at in (0, kb // 2, kb - 1):  # the first, a middle and the last round
            lane = [good(r, name + b"%d" % at) for r in range(kb)]
            k, sig, m, _ = lane[at]
            lane[at] = (k, with_s(sig, s_bytes), m, 0)
            lanes.append(lane)
    # r = 0; r bytes = n (reduces to 0)
    for r_bytes in (zero, n_bytes):
        lane = [good(r, b"r0") for r in range(kb)]
        k, sig, m, _ = lane[1]
        lane[1] = (k, r_bytes + sig[32:], m, 0)
        lanes.append(lane)
    # the high-S twin of a valid signature, beside the signature itself
    lane = [good(r, b"hs") for r in range(kb)]
    k, sig, m, _ = lane[0]
    lane[2] = (k, sig, m, 1)
    lane[3] = (k, with_s(sig, (n_int - int.from_bytes(sig[32:], "big")).to_bytes(32, "big")), m, 0)
    lanes.append(lane)
    # a key the parser rejects; a key index out of range
    for bad_key in (3, len(keys), 0xFFFFFFFF):
        lane = [good(r, b"key") for r in range(kb)]
        k, sig, m, _ = lane[kb - 2]
        lane[kb - 2] = (bad_key, sig, m, 0)
        lanes.append(lane)
    # every s equal to 1: valid signatures under recovered keys
    lane = []
    for r in range(kb):
        m = b"s is one %d" % r
        while True:
            kk = rng.randrange(1, n_int)
            rp = S.gmul(kk)
            x = S.to_affine(rp)[0]
            q = S.recover_key(rp, x, 1, m) if 0 < x < n_int else None
            if q is not None:
                break
        sig = x.to_bytes(32, "big") + (1).to_bytes(32, "big")
        pk = S.encode_point(q)
        assert S.verify(pk, m, sig)
        keys.append(pk)
        lane.append((len(keys) - 1, sig, m, 1))
    lane[kb - 1] = (lane[kb - 1][0], lane[kb - 1][1], lane[kb - 1][2] + b"x", 0)
    lanes.append(lane)
    entries, exp = [], []
    for r in range(kb):
        for lane in lanes:
            entries.append(lane[r][:3])
            exp.append(lane[r][3])
    for (k, sig, m), e in zip(entries, exp):
        assert int(k < len(keys) and S.verify(keys[k], m, sig)) == e
    return keys, entries, exp, len(lanes)


@pytest.mark.parametrize("kb", KBS)
def test_directed_lanes(check, kb):
    keys, entries, exp, lanes = directed_lanes(kb)
    got, one = run(check, kb, lanes, keys, entries)
    assert got.tolist() == exp and one.tolist() == exp


@pytest.mark.parametrize("kb", KBS)
def test_one_active_round(check, kb):
    """n = 1: the lane's other rounds are inactive and enter the product as
    1; so does every round of the launch's other lanes."""
    rng = random.Random(0xA11)
    priv = rng.randbytes(32)
    m = b"alone in its lane"
    for sig, e in ((S.sign(priv, m), 1), (S.sign(priv, m + b"x"), 0)):
        got, one = run(check, kb, 2, [S.pubkey_from_priv(priv)], [(0, sig, m)])
        assert got.tolist() == one.tolist() == [e]


def test_under_sanitizers(corpus):
    """The same program, AddressSanitizer + UBSan: a plain executable on the
    CPU, over the directed lanes and a slice of the corpus that ends in a
    partial launch."""
    san = hostbuild.build(SRC, BIN_SAN, ["-std=c++17", "-g", "-fsanitize=address,undefined",
                                         "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    for kb in KBS:
        keys, entries, exp, lanes = directed_lanes(kb)
        got, one = run(san, kb, lanes, keys, entries)
        assert got.tolist() == exp and one.tolist() == exp
    keys, entries, valid, _ = corpus
    pick = list(range(0, 764, 7))  # 110 signatures: 64 lanes x 4 rounds leaves round 1 partial, 2-3 inactive
    got, one = run(san, 4, 64, keys, [entries[i] for i in pick])
    assert got.tolist() == one.tolist() == [valid[i] for i in pick]
