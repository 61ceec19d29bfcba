"""CPU check of the cross-height typed commit layer
(tests/host/typedcommitscheck.cpp): cmtv_verify_commits_typed in
cometbft_amd/csrc/commit_typed.cpp, with commit.cpp and pipeline.cpp, compiled
unchanged with AddressSanitizer + UBSan against tests/host/fake_runtime.cpp
and tests/host/fake_typed_runtime.cpp (which counts the bulk secp256k1
batches, their signatures and the templates they ship), as a stand-alone
program run directly.

Expected outcomes are tests/typed_commit_ref.py's loops, height by height
(with the sr25519 verifier swapped for the fake runtime's stand-in, as
tests/test_typed_commit_host.py does); the program also compares every
height with cmtv_verify_commit_typed for that height alone. What is under
test is the host work: the grouping of heights by registered set, one
template per height, the partition by key type across heights, the scatter
and the per-height replay."""
import os
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import typed_commit_ref as R  # noqa: E402

from oracle import ed25519_ref as ED  # noqa: E402

CSRC = os.path.join(ROOT, "cometbft_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")
BIN = os.path.join(ROOT, "build", "typedcommitscheck")
SRCS = [os.path.join(HOST, "typedcommitscheck.cpp"), os.path.join(HOST, "fake_runtime.cpp"),
        os.path.join(HOST, "fake_typed_runtime.cpp"), os.path.join(CSRC, "commit.cpp"),
        os.path.join(CSRC, "commit_typed.cpp"), os.path.join(CSRC, "pipeline.cpp")]
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
         "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
KINDS = {"full": 0, "light": 1, "trusting": 2}
CODES = {"set_size": 1, "height": 2, "block_id": 3, "wrong_signature": 4, "not_enough_power": 5, "double_vote": 6,
         "panic": 8}
TYPE_IDS = {"ed25519": 0, "secp256k1": 1, "sr25519": 2}
CHAIN = "typed-heights"


def _build():
    deps = SRCS + [os.path.join(HOST, "case_reader.h"), os.path.join(ROOT, "oracle", "cmtv_oracle.c"),
                   os.path.join(ROOT, "include", "cmtverify.h")] + \
        [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if os.path.exists(BIN) and os.path.getmtime(BIN) >= max(os.path.getmtime(d) for d in deps):
        return BIN
    objdir = os.path.join(ROOT, "build", "typedcommitscheck_obj")
    os.makedirs(objdir, exist_ok=True)
    objs, procs = [], []
    for src in SRCS:
        o = os.path.join(objdir, os.path.basename(src) + ".o")
        procs.append(subprocess.Popen(["g++"] + FLAGS + ["-c", src, "-o", o]))
        objs.append(o)
    o = os.path.join(objdir, "cmtv_oracle.o")
    procs.append(subprocess.Popen(["gcc", "-O2", "-g", "-fsanitize=address,undefined", "-c",
                                   os.path.join(ROOT, "oracle", "cmtv_oracle.c"), "-o", o]))
    objs.append(o)
    for p in procs:
        assert p.wait() == 0, "typedcommitscheck build failed"
    tmp = f"{BIN}.{os.getpid()}"
    subprocess.run(["g++", "-fsanitize=address,undefined", "-o", tmp] + objs + ["-lpthread"], check=True)
    os.replace(tmp, BIN)
    return BIN


@pytest.fixture(scope="module")
def doubles():
    """typed_commit_ref with the sr25519 entries swapped for the fake
    runtime's stand-in (Ed25519, ZIP-215, zero-padded key)."""
    old_v, old_s = R.VERIFIERS["sr25519"], R.SIGNERS["sr25519"]
    R.VERIFIERS["sr25519"] = lambda pk, msg, sig, mode: ED.verify((pk + bytes(32))[:32], msg, sig, 1)
    R.SIGNERS["sr25519"] = ED.sign
    yield
    R.VERIFIERS["sr25519"], R.SIGNERS["sr25519"] = old_v, old_s


def make_vals(types, start):
    out = []
    for i, t in enumerate(types):
        secret, pk = R.keypair("ed25519" if t == "sr25519" else t, start + i)
        out.append(R.Val(t, pk, 10 + i % 3, secret))
    return out


def expect(kind, vals, height, commit, trust):
    if kind == "full":
        return R.verify_commit(vals, CHAIN, commit[2], height, commit)
    if kind == "light":
        return R.verify_commit_light(vals, CHAIN, commit[2], height, commit)
    return R.verify_commit_light_trusting(vals, CHAIN, commit, trust)


def reached(kind, vals, height, commit, trust):
    """How many signatures the loop reaches when every verdict is valid (the
    library's n_verified)."""
    count = [0]
    real = R.verify_signature

    def all_valid(v, msg, sig, mode=0):
        if v.key_type == "ed25519" and len(v.pub_key) != 32:
            raise R.Panic("")
        count[0] += 1
        return True

    R.verify_signature = all_valid
    try:
        e = expect(kind, vals, height, commit, trust)
    finally:
        R.verify_signature = real
    return 0 if e is not None and e[0] in ("set_size", "height", "block_id") else count[0]


def encode_height(kind, vals, height, commit, trust):
    want = expect(kind, vals, height, commit, trust)
    out = [struct.pack("<qI", height, len(vals))]
    for v in vals:
        out.append(struct.pack("<BI", TYPE_IDS[v.key_type], len(v.pub_key)) + v.pub_key +
                   struct.pack("<q", v.power) + v.address)
    h, r, bid, sigs = commit
    out.append(struct.pack("<qi", h, r) + bid[0] + struct.pack("<I", bid[1]) + bid[2] + struct.pack("<I", len(sigs)))
    for s in sigs:
        out.append(struct.pack("<B", s.flag) + (s.address + bytes(20))[:20] + struct.pack("<qiI", s.ts[0], s.ts[1],
                                                                                         len(s.signature)) + s.signature)
    if want is None:
        rc, code, idx, msg = 0, 0, -1, b""
    else:
        rc, code, msg = -6, CODES[want[0]], want[1].encode()
        idx = -2 if want[0] == "panic" else want[2]
        if want[0] == "block_id":
            msg = None
    if msg is None:
        raise AssertionError("no case here fails on its block ID")
    out.append(struct.pack("<iiiI", rc, code, idx, len(msg)) + msg +
               struct.pack("<I", reached(kind, vals, height, commit, trust)))
    return b"".join(out), want


def encode_case(kind, heights, cap=0, trust=(1, 3), types_mode=0, bulk=-1, keyed=-1):
    """heights: [(vals, height, commit)]; returns the case and each height's expectation."""
    blobs, wants = [], []
    for vals, height, commit in heights:
        b, w = encode_height(kind, vals, height, commit, trust)
        blobs.append(b)
        wants.append(w)
    head = struct.pack("<IIQQI", KINDS[kind], cap, trust[0], trust[1], len(CHAIN)) + CHAIN.encode() + \
        struct.pack("<IIii", types_mode, len(heights), bulk, keyed)
    return head + b"".join(blobs), wants


def flip(commit, i):
    h, r, bid, sigs = commit
    sigs = list(sigs)
    s = sigs[i]
    sigs[i] = R.Sig(s.flag, s.address, s.ts, s.signature[:9] + bytes([s.signature[9] ^ 2]) + s.signature[10:])
    return (h, r, bid, sigs)


def test_cross_height_typed_commits_under_asan(doubles, tmp_path):
    set_a = make_vals(["secp256k1"] * 20, 900)
    set_b = make_vals(["secp256k1"] * 20, 950)
    mixed = make_vals(["ed25519", "secp256k1", "sr25519", "secp256k1"] * 5, 1000)
    eds = make_vals(["ed25519"] * 20, 1100)
    flags = [R.COMMIT] * 20
    flags[3], flags[11] = R.NIL, R.ABSENT

    def chain(vals, h0, n, flags=None):
        return [(vals, h, R.make_commit(vals, CHAIN, h, flags=flags)) for h in range(h0, h0 + n)]

    cases, all_wants = [], []

    def add(*a, **kw):
        blob, wants = encode_case(*a, **kw)
        cases.append(blob)
        all_wants.append(wants)
        return wants

    # 6 heights of one 20-validator secp256k1 set: one group, by key bytes and by registered keys
    six = chain(set_a, 10, 6)
    for kind in ("full", "light", "trusting"):
        assert add(kind, six, cap=0, bulk=1, keyed=0) == [None] * 6
        assert add(kind, six, cap=2, bulk=1, keyed=1) == [None] * 6
    # a change of set after height 3: two groups with the cache on, one batch of key bytes without
    two = chain(set_a, 10, 3) + chain(set_b, 13, 3)
    assert add("full", two, cap=2, bulk=2, keyed=2) == [None] * 6
    assert add("full", two, cap=0, bulk=1, keyed=0) == [None] * 6
    # more distinct sets than the cache holds, coming back to the first
    assert add("full", chain(set_a, 10, 2) + chain(set_b, 12, 2) + chain(set_a, 14, 2), cap=1, bulk=3,
               keyed=3) == [None] * 6
    # a mixed Ed / secp / sr set between two pure ones (nil and absent votes in all)
    between = chain(set_a, 20, 2, flags) + chain(mixed, 22, 2, flags) + chain(set_a, 24, 2, flags)
    assert add("full", between, cap=2, bulk=3, keyed=2) == [None] * 6
    assert add("light", between, cap=0, bulk=1, keyed=0) == [None] * 6
    assert add("trusting", between, cap=2) == [None] * 6
    # a mixed set first, then a registered one: the group that starts at the third height ships its own
    # slice of the templates while the Ed25519 and sr25519 shares still read the first heights' at the end
    assert add("full", chain(mixed, 26, 2, flags) + chain(set_a, 28, 2), cap=2, bulk=2, keyed=1) == [None] * 4
    # a commit that fails its preamble (wrong height) in the middle: no device work for it
    wrong_h = chain(set_a, 30, 5)
    wrong_h[2] = (set_a, 99, wrong_h[2][2])
    w = add("full", wrong_h, cap=2, bulk=1, keyed=1)
    assert [x and x[0] for x in w] == [None, None, "height", None, None]
    # a wrong signature at a different index in two heights, in each part of a mixed chain
    bad = chain(mixed, 40, 4, flags)
    bad[1] = (mixed, 41, flip(bad[1][2], 5))   # secp256k1
    bad[3] = (mixed, 43, flip(flip(bad[3][2], 14), 8))  # sr25519 and Ed25519: the first is reported
    w = add("full", bad, cap=0)
    assert [x and x[2] for x in w] == [None, 5, None, 8]
    bad_s = chain(set_a, 50, 4)
    bad_s[0] = (set_a, 50, flip(bad_s[0][2], 19))
    bad_s[2] = (set_a, 52, flip(bad_s[2][2], 0))
    w = add("full", bad_s, cap=2, bulk=1, keyed=1)
    assert [x and x[2] for x in w] == [19, None, 0, None]
    # VerifyCommitLight stops at +2/3: a flipped signature past it is never reached
    assert add("light", bad_s, cap=2)[0] is None
    # a LightTrusting window: the trusted set against later heights' commits, one of them short of power
    window = chain(set_a, 60, 3)
    sparse = [R.COMMIT if i % 4 == 0 else R.ABSENT for i in range(20)]
    window.append((set_a, 63, R.make_commit(set_a, CHAIN, 63, flags=sparse)))
    w = add("trusting", window, cap=2, trust=(1, 3), bulk=1, keyed=1)
    assert [x and x[0] for x in w] == [None, None, None, "not_enough_power"]
    # n = 1
    assert add("full", chain(set_a, 70, 1), cap=2, bulk=1, keyed=1) == [None]
    assert add("full", [(set_a, 70, flip(chain(set_a, 70, 1)[0][2], 7))], cap=0)[0][2] == 7
    # all Ed25519: key_types NULL, and explicit zeros -- the call is cmtv_verify_commits
    ed_chain = chain(eds, 80, 3, flags)
    ed_chain[1] = (eds, 81, flip(ed_chain[1][2], 2))
    for mode in (1, 2):
        w = add("full", ed_chain, types_mode=mode, bulk=0, keyed=0)
        assert [x and x[2] for x in w] == [None, 2, None]
    # an all-Ed25519 height among typed ones keeps a NULL type array
    assert add("full", chain(set_a, 90, 1) + chain(eds, 91, 1) + chain(set_a, 92, 1), cap=2, bulk=1,
               keyed=1) == [None] * 3

    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<I", len(cases)) + b"".join(cases))
    try:
        b = _build()
    except (OSError, subprocess.CalledProcessError, AssertionError) as e:
        pytest.fail(f"could not build typedcommitscheck: {e}")
    r = subprocess.run([b, str(path)], capture_output=True, text=True, timeout=900,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1",
                            "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert f"typedcommitscheck ok ({len(cases)} cases)" in r.stdout
