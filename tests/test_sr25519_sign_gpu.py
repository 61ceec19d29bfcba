"""sr25519 key derivation and signing on the device (cmtv_pubkeys_sr25519 /
cmtv_sign_sr25519, sr25519_sign.hip) against the restatement
oracle/sr25519_ref.py, bit-exact; the round trip through the device and the
Python verifier; the launch seam at kChunk; typed commits of sr25519 and
three-way mixed sets made by the testutil helpers."""
import ctypes
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sr25519_sign_cases as C  # noqa: E402

from cometbft_amd import _native as N  # noqa: E402
from cometbft_amd import testutil as TU  # noqa: E402
from cometbft_amd import types as T  # noqa: E402
from cometbft_amd.crypto import pack_messages  # noqa: E402
from oracle import sr25519_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

K_CHUNK = 1 << 18  # runtime_state.h kChunk: signatures per launch


@pytest.fixture(scope="module")
def signed(gpu_ctx):
    """The 257 signatures of the shared cases, made once on the device."""
    idx, msgs = C.sign_inputs()
    m, off = pack_messages(list(msgs))
    mini = C.keys_array(C.N_SIGN_KEYS)
    sig = gpu_ctx.sign_sr25519(mini, m, off, np.array(idx, np.uint32))
    pk = gpu_ctx.pubkeys_sr25519(mini)
    return mini, pk, np.array(idx, np.uint32), msgs, m, off, sig


# ------------------------------------------------------------------ public keys

@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_pubkeys_and_addresses(gpu_ctx, n):
    pk_exp, addr_exp = C.expected_pubkeys(257)
    pk, addr = gpu_ctx.pubkeys_sr25519(C.keys_array(257)[:n], with_addresses=True)
    assert pk.shape == (n, 32) and addr.shape == (n, 20)
    assert np.array_equal(pk, pk_exp[:n]), np.nonzero((pk != pk_exp[:n]).any(axis=1))[0][:10]
    assert np.array_equal(addr, addr_exp[:n]), np.nonzero((addr != addr_exp[:n]).any(axis=1))[0][:10]
    # without addresses (out_addr = NULL): the same keys
    assert np.array_equal(gpu_ctx.pubkeys_sr25519(C.keys_array(257)[:n]), pk_exp[:n])


# ------------------------------------------------------------------ signatures

def test_signatures_match_the_restatement(signed):
    sig = signed[6]
    bad = np.nonzero((sig != C.expected_signatures()).any(axis=1))[0]
    assert bad.size == 0, bad[:10]


def test_signatures_without_key_indices(gpu_ctx, signed):
    mini, msgs = signed[0], signed[3]
    m, off = pack_messages(list(msgs[:C.N_SIGN_KEYS]))
    sig = gpu_ctx.sign_sr25519(mini, m, off)
    assert np.array_equal(sig, C.expected_signatures_in_order())


def test_round_trip(gpu_ctx, signed):
    _, pk, idx, msgs, m, off, sig = signed
    n = len(msgs)
    assert gpu_ctx.verify_sr25519(pk[idx], sig, m, off).all()
    sample = list(range(len(C.MSG_LENGTHS))) + [100, n - 1]
    for i in sample:
        assert S.verify(pk[idx[i]].tobytes(), msgs[i], sig[i].tobytes()), i
    # a flipped bit in R, one in s, a cleared marker bit
    for col, mask in ((3, 0x01), (40, 0x01), (63, 0x80)):
        bad = sig.copy()
        bad[:, col] ^= mask
        assert not gpu_ctx.verify_sr25519(pk[idx], bad, m, off).any(), col
        assert not S.verify(pk[idx[1]].tobytes(), msgs[1], bad[1].tobytes()), col
    # a flipped message byte (the empty messages have none)
    m2 = m.copy()
    has = np.nonzero(off[1:] > off[:-1])[0]
    m2[off[has]] ^= 0x01
    got = gpu_ctx.verify_sr25519(pk[idx], sig, m2, off)
    assert not got[has].any() and got[np.setdiff1d(np.arange(n), has)].all()
    assert 0 < n - has.size < n


def test_chunk_seam(gpu_ctx):
    n, n_keys, mlen = K_CHUNK + 1, 150, 116
    rng = np.random.default_rng(262145)
    mini = C.keys_array(n_keys)
    msg = rng.integers(0, 256, n * mlen + 1, dtype=np.uint8)
    off = (np.arange(n + 1, dtype=np.uint64) * mlen).astype(np.uint32)
    idx = rng.integers(0, n_keys, n, dtype=np.uint32)
    sig = gpu_ctx.sign_sr25519(mini, msg, off, idx)
    pk = gpu_ctx.pubkeys_sr25519(mini)
    got = gpu_ctx.verify_sr25519(pk[idx], sig, msg, off)
    assert got.all(), np.nonzero(got == 0)[0][:10]
    keys = C.keys(n_keys)
    # the first 8, and the 16 that end at index kChunk: the first launch's last 15 signatures
    # and the second launch's only one
    for i in list(range(8)) + list(range(K_CHUNK - 15, K_CHUNK + 1)):
        assert sig[i].tobytes() == S.sign(keys[idx[i]], msg[i * mlen: (i + 1) * mlen].tobytes()), i


# ------------------------------------------------------------------ argument checks

def test_refused_calls_write_nothing_with_a_live_context(gpu_ctx):
    C.assert_refused(gpu_ctx.handle)
    lib = N.lib()
    assert lib.cmtv_pubkeys_sr25519(gpu_ctx.handle, 0, None, None, None) == N.CMTV_OK
    assert lib.cmtv_sign_sr25519(gpu_ctx.handle, 0, None, 0, None, None, None, None) == N.CMTV_OK
    # n = 0 with keys and indices: still nothing to do
    one = C.keys_array(1)
    off = np.zeros(1, np.uint32)
    out = np.full(64, C.CANARY, np.uint8)
    idx = np.zeros(1, np.uint32)
    rc = lib.cmtv_sign_sr25519(gpu_ctx.handle, 1, C.p8(one), 0, C.p32(idx), None, C.p32(off), C.p8(out))
    assert rc == N.CMTV_OK
    assert (out == C.CANARY).all()
    assert lib.cmtv_abi_version() == 11 and ctypes.sizeof(N.cmtv_stats) == 200


# ------------------------------------------------------------------ typed commits

@pytest.mark.parametrize("n_ed,n_secp,n_sr", [(0, 0, 150), (50, 50, 50)], ids=["sr25519", "mixed"])
def test_typed_commit_from_the_helpers(gpu_ctx, n_ed, n_secp, n_sr):
    sv = TU.make_typed_validator_set(gpu_ctx, n_ed25519=n_ed, n_secp256k1=n_secp, n_sr25519=n_sr)
    vals = sv.valset.validators
    assert len(vals) == n_ed + n_secp + n_sr
    assert [sv.key_types.count(k) for k in ("ed25519", "secp256k1", "sr25519")] == [n_ed, n_secp, n_sr]
    assert [v.address for v in vals] == sorted(v.address for v in vals)
    sr_at = [i for i, kt in enumerate(sv.key_types) if kt == "sr25519"]
    for i in sr_at:
        assert vals[i].key_type == "sr25519" and vals[i].address == hashlib.sha256(vals[i].pub_key).digest()[:20]
    for i in sr_at[:4]:
        assert vals[i].pub_key == S.pubkey_from_mini(sv.secrets[i].tobytes())
    height = 12
    commit, msgs, sigs = TU.make_typed_commit(gpu_ctx, sv, height)
    bid = TU.block_id_for_height(height)
    sv.valset.verify_commit(TU.CHAIN_ID, bid, height, commit, ctx=gpu_ctx)
    sv.valset.verify_commit_light(TU.CHAIN_ID, bid, height, commit, ctx=gpu_ctx)
    for i in (sr_at[0], sr_at[-1]):
        assert sigs[i].tobytes() == S.sign(sv.secrets[i].tobytes(), msgs[i])
        bad = bytearray(commit.signatures[i].signature)
        bad[3] ^= 0x01
        css = list(commit.signatures)
        css[i] = T.CommitSig(css[i].block_id_flag, css[i].validator_address, css[i].timestamp, bytes(bad))
        with pytest.raises(T.ErrWrongSignature) as e:
            sv.valset.verify_commit(TU.CHAIN_ID, bid, height, T.Commit(height, 0, bid, css), ctx=gpu_ctx)
        assert str(e.value) == "wrong signature (#%d): %s" % (i, bytes(bad).hex().upper()) and e.value.index == i
