"""CPU tests of the secp256k1 test-data additions to the C ABI: the new symbols
are declared, bound and exported; cmtv_privkey_secp256k1_from_secret (host
only) against tests/secp256k1_sign_ref.py; every refused call returns
CMTV_EINVAL with its outputs untouched, as far as that shows without a device
(a context cannot be opened here, so each case is also run against a live one
in tests/test_secp256k1_sign_gpu.py); the addition left the ABI version and
cmtv_stats alone."""
import ctypes
import os
import sys

import numpy as np

from cometbft_amd import _native as N
from cometbft_amd import crypto

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import secp256k1_sign_cases as C  # noqa: E402
import secp256k1_sign_ref as R  # noqa: E402

NAMES = ("cmtv_privkey_secp256k1_from_secret", "cmtv_pubkeys_secp256k1", "cmtv_sign_secp256k1")
CANARY = C.CANARY
# crypto/secp256k1/secp256k1_test.go:95-103
SECRETS = [b"", b"We live in a society exquisitely dependent on science and technology, "
           b"in which hardly anyone knows anything about science and technology.", b"\x00", b"mySecret", b""]
u8p = C.u8p


def test_symbols_are_declared_bound_and_exported():
    lib = N.lib()
    with open(os.path.join(ROOT, "include", "cmtverify.h")) as f:
        src = f.read()
    for name in NAMES:
        assert name in N.EXPORTS and getattr(lib, name).argtypes is not None and f" {name}(" in src, name
    for phrase in ("variable-time", "HBM"):
        assert phrase in src
    for name in ("pubkeys_secp256k1", "sign_secp256k1"):
        assert callable(getattr(crypto.Context, name))


def test_privkey_from_secret_matches_the_restatement():
    for s in SECRETS + [bytes(range(55)), bytes(range(56)), bytes(64), b"\xff" * 1000]:
        got = crypto.secp256k1_privkey_from_secret(s)
        assert got == R.privkey_from_secret(s), s
        assert 1 <= int.from_bytes(got, "big") <= R.N - 1
    # the secret is read where it lies: an unaligned view into a larger buffer
    buf = (ctypes.c_uint8 * 64)(*range(64))
    out = (ctypes.c_uint8 * 32)()
    for a in range(1, 5):
        ptr = ctypes.cast(ctypes.addressof(buf) + a, u8p)
        assert N.lib().cmtv_privkey_secp256k1_from_secret(ptr, 21, out) == N.CMTV_OK
        assert bytes(out) == R.privkey_from_secret(bytes(range(a, a + 21)))


def test_privkey_from_secret_einval_writes_nothing():
    lib = N.lib()
    out = (ctypes.c_uint8 * 32)(*([CANARY] * 32))
    one = (ctypes.c_uint8 * 1)(7)
    assert lib.cmtv_privkey_secp256k1_from_secret(one, 1, None) == N.CMTV_EINVAL
    assert lib.cmtv_privkey_secp256k1_from_secret(None, 1, out) == N.CMTV_EINVAL
    assert set(bytes(out)) == {CANARY}
    # a NULL secret of no length is the empty secret
    assert lib.cmtv_privkey_secp256k1_from_secret(None, 0, out) == N.CMTV_OK
    assert bytes(out) == R.privkey_from_secret(b"")


def test_refused_calls_write_nothing_without_a_context():
    C.assert_refused(None)
    # and so is every well-formed call, n = 0 included, without a context
    lib = N.lib()
    out = np.full(64, CANARY, np.uint8)
    assert lib.cmtv_pubkeys_secp256k1(None, 0, None, None, None) == N.CMTV_EINVAL
    assert lib.cmtv_sign_secp256k1(None, 0, None, 0, None, None, None, None) == N.CMTV_EINVAL
    one = np.frombuffer((1).to_bytes(32, "big"), np.uint8).copy()
    assert lib.cmtv_pubkeys_secp256k1(None, 1, C.p8(one), C.p8(out), None) == N.CMTV_EINVAL
    assert (out == CANARY).all()


def test_abi_version_and_stats_layout_unchanged():
    assert N.lib().cmtv_abi_version() == 11
    assert ctypes.sizeof(N.cmtv_stats) == 200
    with open(os.path.join(ROOT, "include", "cmtverify.h")) as f:
        assert "#define CMTV_ABI_VERSION 11" in f.read()
