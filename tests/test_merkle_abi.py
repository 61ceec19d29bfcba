"""CPU tests of the merkle additions to the C ABI: the two host leaf encoders
(cmtv_validator_bytes, cmtv_commit_sig_bytes) against tests/merkle_ref.py,
their CMTV_EINVAL rules with the output untouched, NULL contexts, and that
the addition left the ABI version and cmtv_stats alone. (The argument rules
of the calls that take a context are in tests/test_merkle_gpu.py: they need
an open one.)"""
import ctypes
import os
import random
import sys

from cometbft_amd import _native as N
from cometbft_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import merkle_ref as R  # noqa: E402

POWERS = [0, 1, 127, 128, 2**63 - 1, -1]
FLAGS = [0, 1, 2, 3, 127, 128, 255]
SECONDS = [0, R.GO_ZERO_TIME_SECONDS, 2**31, R.LAST_VALID_SECOND]
NANOS = [0, 1, 999_999_999]
CANARY = 0xA5


def _buf(data: bytes):
    return (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")


def validator_bytes(key_type, key, power, cap=128):
    out = (ctypes.c_uint8 * max(cap, 1))(*([CANARY] * max(cap, 1)))
    n = N.lib().cmtv_validator_bytes(key_type, _buf(key), len(key), power, out, cap)
    return n, bytes(out)


def commit_sig_bytes(flag, addr, sec, nanos, sig, cap=256):
    out = (ctypes.c_uint8 * max(cap, 1))(*([CANARY] * max(cap, 1)))
    n = N.lib().cmtv_commit_sig_bytes(flag, _buf(addr) if addr is not None else None, sec, nanos, _buf(sig), len(sig),
                                      out, cap)
    return n, bytes(out)


def test_validator_bytes_matches_reference():
    rng = random.Random(21)
    cases = [(kt, rng.randbytes(klen), p) for kt in (0, 1) for klen in (1, 32, 33, 64) for p in POWERS]
    cases += [(rng.randrange(2), rng.randbytes(rng.randrange(1, 65)), rng.randrange(-2**63, 2**63))
              for _ in range(300)]
    for kt, key, power in cases:
        n, out = validator_bytes(kt, key, power)
        want = R.validator_bytes(kt, key, power)
        assert n == len(want) and out[:n] == want, (kt, len(key), power)
        assert set(out[n:]) <= {CANARY}


def test_commit_sig_bytes_matches_reference():
    rng = random.Random(22)
    cases = [(f, rng.randbytes(20), s, ns, rng.randbytes(sl))
             for f in FLAGS for s in SECONDS for ns in NANOS for sl in (0, 1, 63, 64, 65, 200)]
    cases += [(rng.choice(FLAGS + [2**32 - 1]), rng.choice([None, rng.randbytes(20)]),
               rng.randrange(R.GO_ZERO_TIME_SECONDS, R.LAST_VALID_SECOND + 1), rng.randrange(10**9),
               rng.randbytes(rng.randrange(0, 100))) for _ in range(300)]
    for flag, addr, sec, nanos, sig in cases:
        n, out = commit_sig_bytes(flag, addr, sec, nanos, sig, cap=320)
        want = R.commit_sig_bytes(flag, addr, sec, nanos, sig)
        assert n == len(want) and out[:n] == want, (flag, sec, nanos, len(sig))


def test_python_validator_bytes():
    key = bytes(range(32))
    assert T.Validator(key, 10).bytes() == R.validator_bytes(R.KEY_ED25519, key, 10)
    key33 = b"\x02" + key
    assert T.Validator(key33, -1, key_type="secp256k1").bytes() == R.validator_bytes(R.KEY_SECP256K1, key33, -1)


def test_encoders_report_the_length_when_the_buffer_is_short():
    key = bytes(32)
    want = R.validator_bytes(0, key, 5)
    n, out = validator_bytes(0, key, 5, cap=len(want) - 1)
    assert n == len(want) and set(out) == {CANARY}
    n, out = validator_bytes(0, key, 5, cap=len(want))
    assert n == len(want) and out == want
    assert N.lib().cmtv_validator_bytes(0, _buf(key), 32, 5, None, 0) == len(want)
    want = R.commit_sig_bytes(2, bytes(20), 1, 1, bytes(64))
    n, out = commit_sig_bytes(2, bytes(20), 1, 1, bytes(64), cap=len(want) - 1)
    assert n == len(want) and set(out) == {CANARY}
    assert N.lib().cmtv_commit_sig_bytes(2, _buf(bytes(20)), 1, 1, _buf(bytes(64)), 64, None, 0) == len(want)


def test_validator_bytes_einval_rules_leave_out_untouched():
    key = bytes(32)
    bad = [(R.KEY_SR25519, key), (3, key), (255, key), (2**32 - 1, key), (0, b""), (1, b""), (0, bytes(65)),
           (1, bytes(65)), (0, bytes(1000))]
    for kt, k in bad:
        n, out = validator_bytes(kt, k, 1)
        assert n == N.CMTV_EINVAL, (kt, len(k))
        assert set(out) == {CANARY}
    out = (ctypes.c_uint8 * 8)()
    assert N.lib().cmtv_validator_bytes(0, None, 32, 1, out, 8) == N.CMTV_EINVAL
    assert N.lib().cmtv_validator_bytes(0, _buf(key), 32, 1, None, 8) == N.CMTV_EINVAL


def test_commit_sig_bytes_einval_rules_leave_out_untouched():
    bad = [(R.GO_ZERO_TIME_SECONDS - 1, 0), (R.LAST_VALID_SECOND + 1, 0), (-2**63, 0), (2**63 - 1, 0), (0, -1),
           (0, 10**9), (0, 2**31 - 1), (0, -2**31)]
    for sec, nanos in bad:
        n, out = commit_sig_bytes(2, bytes(20), sec, nanos, bytes(64))
        assert n == N.CMTV_EINVAL, (sec, nanos)
        assert set(out) == {CANARY}
    for sec, nanos in [(R.GO_ZERO_TIME_SECONDS, 0), (R.LAST_VALID_SECOND, 999_999_999)]:
        assert commit_sig_bytes(2, bytes(20), sec, nanos, b"")[0] > 0
    out = (ctypes.c_uint8 * 8)()
    assert N.lib().cmtv_commit_sig_bytes(2, None, 0, 0, None, 4, out, 8) == N.CMTV_EINVAL
    assert N.lib().cmtv_commit_sig_bytes(2, None, 0, 0, None, 0, None, 8) == N.CMTV_EINVAL


def test_null_context_is_einval_and_writes_nothing():
    lib = N.lib()
    out = (ctypes.c_uint8 * 64)(*([CANARY] * 64))
    off = (ctypes.c_uint32 * 2)(0, 1)
    item = _buf(b"x")
    assert lib.cmtv_merkle_root(None, 1, item, off, out) == N.CMTV_EINVAL
    assert lib.cmtv_merkle_root(None, 0, None, None, out) == N.CMTV_EINVAL
    assert lib.cmtv_merkle_roots(None, 1, off, item, off, out) == N.CMTV_EINVAL
    vs = N.cmtv_valset()
    assert lib.cmtv_valset_hash(None, ctypes.byref(vs), None, out) == N.CMTV_EINVAL
    assert lib.cmtv_valset_hashes(None, 1, ctypes.byref(vs), None, out) == N.CMTV_EINVAL
    cm = N.cmtv_commit()
    assert lib.cmtv_commit_hash(None, ctypes.byref(cm), out) == N.CMTV_EINVAL
    assert lib.cmtv_commit_hashes(None, 1, ctypes.byref(cm), out) == N.CMTV_EINVAL
    assert set(bytes(out)) == {CANARY}


def test_abi_version_and_stats_layout_unchanged():
    assert N.lib().cmtv_abi_version() == 11
    assert ctypes.sizeof(N.cmtv_stats) == 200
    with open(os.path.join(ROOT, "include", "cmtverify.h")) as f:
        assert "#define CMTV_ABI_VERSION 11" in f.read()
