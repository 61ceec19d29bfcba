"""CPU tests of the typed commit entry point's surface (no GPU compute): the
symbol, its argument checks that need no device, and the Python types' key
type field, addresses and packing."""
import ctypes
import hashlib

import numpy as np
import pytest

from cometbft_amd import _native as N
from cometbft_amd import types as T
from cometbft_amd.ripemd160 import ripemd160


def test_symbol_is_exported_and_bound():
    lib = N.lib()
    assert hasattr(lib, "cmtv_verify_commit_typed")
    assert "cmtv_verify_commit_typed" in N.EXPORTS
    assert lib.cmtv_abi_version() == 11  # additive: the version stays
    assert (N.KEY_ED25519, N.KEY_SECP256K1, N.KEY_SR25519) == (0, 1, 2)


def test_null_context_is_einval():
    vals = T.ValidatorSet([T.Validator(bytes(33), 10, 0, "secp256k1")])
    commit = T.Commit(1, 0, T.BlockID(), [T.CommitSig(T.BLOCK_ID_FLAG_COMMIT, bytes(20), (1, 1), bytes(64))])
    vs, keep_v = vals._pack()
    cm, keep_c = T._pack_commit(commit)
    bid, keep_b = T.BlockID()._c()
    res = N.cmtv_commit_result()
    kt = keep_v[5].ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    lib = N.lib()
    assert lib.cmtv_verify_commit_typed(None, N.VERIFY_COMMIT, 0, b"c", 1, ctypes.byref(vs), kt, ctypes.byref(bid), 1,
                                        ctypes.byref(cm), 0, 0, ctypes.byref(res), None, 0) == N.CMTV_EINVAL
    assert lib.cmtv_verify_commit_typed(None, N.VERIFY_COMMIT, 0, b"c", 1, None, None, None, 1, None, 0, 0, None,
                                        None, 0) == N.CMTV_EINVAL


def test_validator_key_type_field_address_and_packing():
    pk = bytes([2]) + hashlib.sha256(b"k").digest()
    assert T.Validator(pk[1:], 5).key_type == "ed25519"
    assert T.Validator(pk[1:], 5).address == hashlib.sha256(pk[1:]).digest()[:20]
    assert T.Validator(pk[1:], 5, 0, "sr25519").address == hashlib.sha256(pk[1:]).digest()[:20]
    # secp256k1: RIPEMD160(SHA256(key)) (crypto/secp256k1/secp256k1.go:156-167)
    assert T.Validator(pk, 5, 0, "secp256k1").address == ripemd160(hashlib.sha256(pk).digest())
    assert ripemd160(b"abc").hex() == "8eb208f7e05d987a9b044a8e98c6b087f15a0bfc"
    with pytest.raises(ValueError):
        T.Validator(pk, 5, 0, "bls12381").address
    vs = T.ValidatorSet([T.Validator(pk[1:], 1), T.Validator(pk, 2, 0, "secp256k1"),
                         T.Validator(pk[1:], 3, 0, "sr25519")])
    s, keep = vs._pack()
    assert list(keep[5][:3]) == [N.KEY_ED25519, N.KEY_SECP256K1, N.KEY_SR25519]
    assert list(keep[1]) == [0, 32, 65, 97]
    assert np.array_equal(keep[4][20:40], np.frombuffer(ripemd160(hashlib.sha256(pk).digest()), np.uint8))
