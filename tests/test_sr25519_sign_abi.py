"""CPU tests of the sr25519 test-data additions to the C ABI: the new symbols
are declared, bound and exported; every refused call returns CMTV_EINVAL with
its outputs untouched, as far as that shows without a device (a context cannot
be opened here, so each case is also run against a live one in
tests/test_sr25519_sign_gpu.py); the addition left the ABI version and
cmtv_stats alone; and the contract's reference, oracle/sr25519_ref.py, verifies
what it signs and agrees with the C oracle."""
import ctypes
import os
import sys

import numpy as np

from cometbft_amd import _native as N
from cometbft_amd import crypto, testutil
from oracle import coracle
from oracle import sr25519_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sr25519_sign_cases as C  # noqa: E402

NAMES = ("cmtv_pubkeys_sr25519", "cmtv_sign_sr25519")
CANARY = C.CANARY


def test_symbols_are_declared_bound_and_exported():
    lib = N.lib()
    with open(os.path.join(ROOT, "include", "cmtverify.h")) as f:
        src = f.read()
    for name in NAMES:
        assert name in N.EXPORTS and getattr(lib, name).argtypes is not None and f" {name}(" in src, name
    block = src[src.index("The same for sr25519"):]
    for phrase in ("variable-time", "HBM", "cmtverify/sr25519-witness", "OS randomness", "mini secret"):
        assert phrase in block, phrase
    for name in ("pubkeys_sr25519", "sign_sr25519"):
        assert callable(getattr(crypto.Context, name))
    for name in ("sr25519_validator_minis", "make_typed_validator_set", "make_typed_commit"):
        assert callable(getattr(testutil, name))


def test_the_product_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "cometbft_amd")
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            with open(os.path.join(pkg, f)) as fh:
                text = fh.read()
            assert "import oracle" not in text and "from oracle" not in text, f


def test_synthetic_mini_secrets():
    import hashlib

    m = testutil.sr25519_validator_minis(3, offset=5)
    assert m.shape == (3, 32) and m.dtype == np.uint8
    assert [r.tobytes() for r in m] == [hashlib.sha256(b"cmtverify/val/sr25519/%d" % i).digest() for i in (5, 6, 7)]


def test_refused_calls_write_nothing_without_a_context():
    C.assert_refused(None)
    # and so is every well-formed call, n = 0 included, without a context
    lib = N.lib()
    out = np.full(64, CANARY, np.uint8)
    assert lib.cmtv_pubkeys_sr25519(None, 0, None, None, None) == N.CMTV_EINVAL
    assert lib.cmtv_sign_sr25519(None, 0, None, 0, None, None, None, None) == N.CMTV_EINVAL
    one = C.keys_array(1)
    assert lib.cmtv_pubkeys_sr25519(None, 1, C.p8(one), C.p8(out), None) == N.CMTV_EINVAL
    assert (out == CANARY).all()


def test_abi_version_and_stats_layout_unchanged():
    assert N.lib().cmtv_abi_version() == 11
    assert ctypes.sizeof(N.cmtv_stats) == 200
    with open(os.path.join(ROOT, "include", "cmtverify.h")) as f:
        assert "#define CMTV_ABI_VERSION 11" in f.read()


def test_the_restatement_verifies_what_it_signs():
    idx, msgs = C.sign_inputs()
    ks = C.keys(C.N_SIGN_KEYS)
    exp = C.expected_signatures()
    for j in range(len(C.MSG_LENGTHS)):  # one of each message length
        pk = S.pubkey_from_mini(ks[idx[j]])
        sig = exp[j].tobytes()
        assert S.verify(pk, msgs[j], sig), j
        assert not S.verify(pk, msgs[j] + b"x", sig), j


def test_c_oracle_equals_the_restatement_on_8_signatures():
    idx, msgs = C.sign_inputs()
    m, off = coracle.pack_msgs(list(msgs[:8]))
    got = coracle.sr25519_sign_batch(C.keys_array(C.N_SIGN_KEYS), m, off, np.array(idx[:8], np.uint32))
    assert np.array_equal(got, C.expected_signatures()[:8])
    assert np.array_equal(coracle.sr25519_pubkeys(C.keys_array(8)), C.expected_pubkeys(257)[0][:8])
