"""secp256k1 key derivation and RFC 6979 signing on the device
(cmtv_pubkeys_secp256k1 / cmtv_sign_secp256k1, secp256k1_sign.hip) against the
restatement tests/secp256k1_sign_ref.py, bit-exact; the round trip through the
Python and the device verifier; the launch seam at kChunk; typed commits made
by the testutil helpers."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import merkle_ref as M  # noqa: E402
import secp256k1_ref as S  # noqa: E402
import secp256k1_sign_cases as C  # noqa: E402
import secp256k1_sign_ref as R  # noqa: E402

from cometbft_amd import _native as N  # noqa: E402
from cometbft_amd import testutil as TU  # noqa: E402
from cometbft_amd import types as T  # noqa: E402
from cometbft_amd.crypto import Secp256k1KeySet, pack_messages  # noqa: E402

pytestmark = pytest.mark.gpu

K_CHUNK = 1 << 18  # runtime_state.h kChunk: signatures per launch
LOW_S_NEGATED = 139  # of the 257 (tests/secp256k1_sign_cases.py), counted by the restatement


@pytest.fixture(scope="module")
def signed(gpu_ctx):
    """The 257 signatures of the shared cases, made once on the device."""
    idx, msgs = C.sign_inputs()
    m, off = pack_messages(list(msgs))
    priv = C.keys_array(C.N_SIGN_KEYS)
    sig = gpu_ctx.sign_secp256k1(priv, m, off, np.array(idx, np.uint32))
    pk = gpu_ctx.pubkeys_secp256k1(priv)
    return priv, pk, np.array(idx, np.uint32), msgs, m, off, sig


# ------------------------------------------------------------------ public keys

@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_pubkeys_and_addresses(gpu_ctx, n):
    pk_exp, addr_exp = C.expected_pubkeys(257)
    pk, addr = gpu_ctx.pubkeys_secp256k1(C.keys_array(257)[:n], with_addresses=True)
    assert pk.shape == (n, 33) and addr.shape == (n, 20)
    assert np.array_equal(pk, pk_exp[:n]), np.nonzero((pk != pk_exp[:n]).any(axis=1))[0][:10]
    assert np.array_equal(addr, addr_exp[:n]), np.nonzero((addr != addr_exp[:n]).any(axis=1))[0][:10]
    # without addresses (out_addr = NULL): the same keys
    assert np.array_equal(gpu_ctx.pubkeys_secp256k1(C.keys_array(257)[:n]), pk_exp[:n])


def test_known_answer_key(gpu_ctx):
    key = C.KAT["key"]
    pk, addr = gpu_ctx.pubkeys_secp256k1(np.frombuffer(bytes.fromhex(key["priv"]), np.uint8), with_addresses=True)
    assert pk[0].tobytes().hex() == key["pub"] and addr[0].tobytes().hex() == key["address"]


# ------------------------------------------------------------------ signatures

def test_signatures_match_the_restatement(signed):
    sig = signed[6]
    exp, negated = C.expected_signatures()
    assert negated == LOW_S_NEGATED and 64 <= negated <= 193
    bad = np.nonzero((sig != exp).any(axis=1))[0]
    assert bad.size == 0, bad[:10]
    kat = C.KAT["signature"]
    assert sig[0].tobytes().hex() == kat["r"] + kat["s"]


def test_signatures_without_key_indices(gpu_ctx, signed):
    priv, msgs = signed[0], signed[3]
    m, off = pack_messages(list(msgs[:C.N_SIGN_KEYS]))
    sig = gpu_ctx.sign_secp256k1(priv, m, off)
    assert np.array_equal(sig, C.expected_signatures_in_order())


def test_round_trip(gpu_ctx, signed):
    _, pk, idx, msgs, m, off, sig = signed
    for i in range(len(msgs)):
        assert S.verify(pk[idx[i]].tobytes(), msgs[i], sig[i].tobytes()), i
    assert gpu_ctx.verify_secp256k1(pk[idx], sig, m, off).all()
    # one flipped bit of sig[3], one of the message (the empty messages have none)
    bad = sig.copy()
    bad[:, 3] ^= 0x01
    assert not gpu_ctx.verify_secp256k1(pk[idx], bad, m, off).any()
    m2 = m.copy()
    has = np.nonzero(off[1:] > off[:-1])[0]
    m2[off[has]] ^= 0x01
    got = gpu_ctx.verify_secp256k1(pk[idx], sig, m2, off)
    assert not got[has].any() and got[np.setdiff1d(np.arange(len(msgs)), has)].all()
    for i in (0, 1, 100):
        assert not S.verify(pk[idx[i]].tobytes(), msgs[i], bad[i].tobytes())


def test_chunk_seam(gpu_ctx):
    n, n_keys, mlen = K_CHUNK + 1, 150, 116
    rng = np.random.default_rng(262145)
    priv = C.keys_array(n_keys)
    msg = rng.integers(0, 256, n * mlen + 1, dtype=np.uint8)
    off = (np.arange(n + 1, dtype=np.uint64) * mlen).astype(np.uint32)
    idx = rng.integers(0, n_keys, n, dtype=np.uint32)
    sig = gpu_ctx.sign_secp256k1(priv, msg, off, idx)
    pk = gpu_ctx.pubkeys_secp256k1(priv)
    ks = Secp256k1KeySet(gpu_ctx, pk)
    try:
        got = gpu_ctx.verify_secp256k1_indexed(ks, idx, sig, msg, off)
    finally:
        ks.free()
    assert got.all(), np.nonzero(got == 0)[0][:10]
    sl = slice(K_CHUNK - 4095, K_CHUNK + 1)  # the generic verifier on 4,096 signatures over the seam
    o = off[sl.start: sl.stop + 1]
    assert gpu_ctx.verify_secp256k1(pk[idx[sl]], sig[sl], msg[o[0]: o[-1] + 1], o - o[0]).all()
    keys = C.keys(n_keys)
    # the first 8, and the 16 that end at index kChunk: the first launch's last 15 signatures
    # and the second launch's only one (which are also the call's last 8)
    for i in list(range(8)) + list(range(K_CHUNK - 15, K_CHUNK + 1)):
        assert sig[i].tobytes() == R.sign(keys[idx[i]], msg[i * mlen: (i + 1) * mlen].tobytes()), i


# ------------------------------------------------------------------ argument checks

def test_refused_calls_write_nothing_with_a_live_context(gpu_ctx):
    C.assert_refused(gpu_ctx.handle)
    lib = N.lib()
    assert lib.cmtv_pubkeys_secp256k1(gpu_ctx.handle, 0, None, None, None) == N.CMTV_OK
    assert lib.cmtv_sign_secp256k1(gpu_ctx.handle, 0, None, 0, None, None, None, None) == N.CMTV_OK
    # n = 0 with keys and indices: still nothing to do
    one = np.frombuffer((1).to_bytes(32, "big"), np.uint8).copy()
    off = np.zeros(1, np.uint32)
    out = np.full(64, C.CANARY, np.uint8)
    idx = np.zeros(1, np.uint32)
    rc = lib.cmtv_sign_secp256k1(gpu_ctx.handle, 1, C.p8(one), 0, C.p32(idx), None, C.p32(off), C.p8(out))
    assert rc == N.CMTV_OK
    assert (out == C.CANARY).all()
    assert lib.cmtv_abi_version() == 11 and ctypes.sizeof(N.cmtv_stats) == 200


# ------------------------------------------------------------------ typed commits

@pytest.mark.parametrize("n_secp,n_ed", [(150, 0), (50, 100)], ids=["secp256k1", "mixed"])
def test_typed_commit_from_the_helpers(gpu_ctx, n_secp, n_ed):
    sv = TU.make_secp256k1_validator_set(gpu_ctx, n_secp, n_ed25519=n_ed)
    vals = sv.valset.validators
    assert len(vals) == n_secp + n_ed and sv.key_types.count("secp256k1") == n_secp
    assert [v.address for v in vals] == sorted(v.address for v in vals)
    for v, kt, secret in zip(vals[:20], sv.key_types, sv.secrets):
        if kt == "secp256k1":
            assert v.pub_key == R.pubkey(secret.tobytes()) and v.address == R.address(v.pub_key)
    height = 12
    commit, msgs, sigs = TU.make_secp256k1_commit(gpu_ctx, sv, height)
    bid = TU.block_id_for_height(height)
    sv.valset.verify_commit(TU.CHAIN_ID, bid, height, commit, ctx=gpu_ctx)
    sv.valset.verify_commit_light(TU.CHAIN_ID, bid, height, commit, ctx=gpu_ctx)
    first_secp = sv.key_types.index("secp256k1")
    for i in (first_secp, len(vals) - 1):
        if sv.key_types[i] == "secp256k1":
            assert sigs[i].tobytes() == R.sign(sv.secrets[i].tobytes(), msgs[i])
        bad = bytearray(commit.signatures[i].signature)
        bad[3] ^= 0x01
        css = list(commit.signatures)
        css[i] = T.CommitSig(css[i].block_id_flag, css[i].validator_address, css[i].timestamp, bytes(bad))
        with pytest.raises(T.ErrWrongSignature) as e:
            sv.valset.verify_commit(TU.CHAIN_ID, bid, height, T.Commit(height, 0, bid, css), ctx=gpu_ctx)
        assert str(e.value) == "wrong signature (#%d): %s" % (i, bytes(bad).hex().upper()) and e.value.index == i
    want = M.valset_hash([(N.KEY_TYPES[v.key_type], v.pub_key, v.voting_power) for v in vals])
    assert sv.valset.hash(gpu_ctx) == want
