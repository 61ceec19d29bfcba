"""cmtv_verify_commits_typed in the C ABI, without a GPU: the export is
there and bound, NULL arguments are CMTV_EINVAL, and the addition leaves
CMTV_ABI_VERSION at 11 (tests/test_abi.py compares the header with
_native.EXPORTS)."""
import ctypes
import os
import re

from cometbft_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_export_is_declared_bound_and_present():
    lib = N.lib()
    assert hasattr(lib, "cmtv_verify_commits_typed")
    assert "cmtv_verify_commits_typed" in N.EXPORTS
    assert lib.cmtv_verify_commits_typed.restype is ctypes.c_int
    assert len(lib.cmtv_verify_commits_typed.argtypes) == 17
    with open(os.path.join(ROOT, "include", "cmtverify.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+cmtv_verify_commits_typed\s*\(", src)


def test_null_arguments_are_einval():
    lib = N.lib()
    res = (N.cmtv_commit_result * 1)()
    rcs = (ctypes.c_int * 1)()
    # no context, with and without commits
    assert lib.cmtv_verify_commits_typed(None, 0, 0, b"c", 1, 0, None, None, None, None, None, 0, 0, None, None, None,
                                         0) == N.CMTV_EINVAL
    assert lib.cmtv_verify_commits_typed(None, 0, 0, b"c", 1, 1, None, None, None, None, None, 0, 0, res, rcs, None,
                                         0) == N.CMTV_EINVAL


def test_abi_version_stays_11():
    assert N.lib().cmtv_abi_version() == 11
    with open(os.path.join(ROOT, "include", "cmtverify.h")) as f:
        assert re.search(r"#define\s+CMTV_ABI_VERSION\s+11\b", f.read())


def test_stats_names_the_batched_launch_counter():
    names = [k for k, _ in N.cmtv_stats._fields_]
    assert "secp_batch_launches" in names and "reserved" not in names
    with open(os.path.join(ROOT, "include", "cmtverify.h")) as f:
        assert re.search(r"uint32_t\s+secp_batch_launches;", f.read())
