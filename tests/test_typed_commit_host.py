"""CPU check of the typed commit layer (tests/host/typedcheck.cpp):
cmtv_verify_commit_typed in cometbft_amd/csrc/commit_typed.cpp, with
commit.cpp and pipeline.cpp, compiled unchanged with AddressSanitizer + UBSan
against tests/host/fake_runtime.cpp and tests/host/fake_typed_runtime.cpp, as
a stand-alone program run directly. The program also holds a single commit to
its own routes: no bulk secp256k1 batch, and a mixed set's Ed25519 share as
one batch without message offsets.

The doubles verify Ed25519 with the C oracle, secp256k1 with the
host-compiled secp256k1.h over messages rebuilt from the templates, and the
"sr25519" batch with what fake_runtime.cpp's verify_host_locked does for any
mode: the C oracle's Ed25519 (ZIP-215 for a non-zero mode) over the key the
layer zero-padded to 32 bytes. So the sr25519 validators here hold Ed25519
keys, and the expected outcomes come from tests/typed_commit_ref.py's loops
with that one verifier swapped: what is under test is the partition by type,
the per-part arrays and the scatter back into plan order, not sr25519."""
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
BIN = os.path.join(ROOT, "build", "typedcheck")
SRCS = [os.path.join(HOST, "typedcheck.cpp"), os.path.join(HOST, "fake_runtime.cpp"),
        os.path.join(HOST, "fake_typed_runtime.cpp"), os.path.join(CSRC, "commit.cpp"),
        os.path.join(CSRC, "commit_typed.cpp"), os.path.join(CSRC, "pipeline.cpp")]
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
         "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
KINDS = {"full": 0, "light": 1, "trusting": 2}
CODES = {"wrong_signature": 4, "not_enough_power": 5, "double_vote": 6, "panic": 8}
TYPE_IDS = {"ed25519": 0, "secp256k1": 1, "sr25519": 2}
CHAIN, HEIGHT = "typed-host", 9


def _build():
    deps = SRCS + [os.path.join(HOST, "case_reader.h"), os.path.join(ROOT, "oracle", "cmtv_oracle.c"),
                   os.path.join(ROOT, "include", "cmtverify.h")] + \
        [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if os.path.exists(BIN) and os.path.getmtime(BIN) >= max(os.path.getmtime(d) for d in deps):
        return BIN
    objdir = os.path.join(ROOT, "build", "typedcheck_obj")
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
        assert p.wait() == 0, "typedcheck build failed"
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


def make_vals(types):
    out = []
    for i, t in enumerate(types):
        secret, pk = R.keypair("ed25519" if t == "sr25519" else t, 500 + i)
        out.append(R.Val(t, pk, 10 + i % 3, secret))
    return out


def reached(kind, vals, commit, trust):
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
        expect(kind, vals, commit, trust)
    finally:
        R.verify_signature = real
    return count[0]


def expect(kind, vals, commit, trust):
    if kind == "full":
        return R.verify_commit(vals, CHAIN, commit[2], HEIGHT, commit)
    if kind == "light":
        return R.verify_commit_light(vals, CHAIN, commit[2], HEIGHT, commit)
    return R.verify_commit_light_trusting(vals, CHAIN, commit, trust)


def encode(kind, vals, commit, cap=0, trust=(1, 3), keyed=0):
    want = expect(kind, vals, commit, trust)
    out = [struct.pack("<IIQQqI", KINDS[kind], cap, trust[0], trust[1], HEIGHT, len(CHAIN)), CHAIN.encode(),
           struct.pack("<I", len(vals))]
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
    out.append(struct.pack("<iiiI", rc, code, idx, len(msg)) + msg +
               struct.pack("<Ii", reached(kind, vals, commit, trust), keyed))
    return b"".join(out), want


def test_partition_and_scatter_under_asan(doubles, tmp_path):
    types = ["ed25519", "secp256k1", "sr25519", "secp256k1", "sr25519", "ed25519", "sr25519"] * 10  # 70, mixed
    vals = make_vals(types)
    flags = [R.COMMIT] * 70
    for i in (3, 9, 10, 44):
        flags[i] = R.NIL
    for i in (5, 30):
        flags[i] = R.ABSENT
    good = R.make_commit(vals, CHAIN, HEIGHT, flags=flags)
    cases, wants = [], []

    def add(*a, **kw):
        blob, want = encode(*a, **kw)
        cases.append(blob)
        wants.append(want)
        return want

    for kind in ("full", "light", "trusting"):
        assert add(kind, vals, good) is None
    # a wrong signature in each part: Ed25519 (#14), secp256k1 (#15), sr25519 (#16), alone and together
    def flip(commit, i):
        h, r, bid, sigs = commit
        sigs = list(sigs)
        s = sigs[i]
        sigs[i] = R.Sig(s.flag, s.address, s.ts, s.signature[:9] + bytes([s.signature[9] ^ 2]) + s.signature[10:])
        return (h, r, bid, sigs)

    for bad in ((14,), (15,), (16,), (16, 15, 14), (60, 16)):
        c = good
        for i in bad:
            c = flip(c, i)
        for kind in ("full", "light"):
            want = add(kind, vals, c)
            assert want[0] == "wrong_signature" and want[2] == min(bad)
    # a sparse LightTrusting plan: a third of the votes nil or absent, half of
    # the rest from addresses the set does not hold, a trust level the loop
    # needs most of the remainder for
    sparse_flags = [R.COMMIT if i % 3 else (R.NIL if i % 2 else R.ABSENT) for i in range(70)]
    sparse = R.make_commit(vals, CHAIN, HEIGHT, flags=sparse_flags)
    h, r, bid, sigs = sparse
    sigs = [R.Sig(s.flag, bytes([i]) * 20 if s.flag == R.COMMIT and i % 4 == 1 else s.address, s.ts, s.signature)
            for i, s in enumerate(sigs)]
    sparse = (h, r, bid, sigs)
    assert add("trusting", vals, sparse, trust=(1, 3)) is None
    assert add("trusting", vals, sparse, trust=(9, 10))[0] == "not_enough_power"
    assert add("trusting", vals, flip(sparse, 26), trust=(9, 10))[2] == 26
    # a double vote by a secp256k1 validator, a short signature, a short Ed25519 key, a short secp256k1 key
    dv = list(good[3])
    dv[20] = R.Sig(dv[20].flag, vals[1].address, dv[20].ts, dv[20].signature)
    want = add("trusting", vals, (good[0], good[1], good[2], dv), trust=(9, 10))
    assert want[0] == "double_vote" and "PubKeySecp256k1{" in want[1]
    short = list(good[3])
    short[22] = R.Sig(short[22].flag, short[22].address, short[22].ts, short[22].signature[:63])
    assert add("full", vals, (good[0], good[1], good[2], short))[2] == 22
    edshort = vals[:21] + [R.Val("ed25519", vals[21].pub_key[:31], 10)] + vals[22:]
    assert add("full", edshort, good)[0] == "panic"
    secpshort = vals[:22] + [R.Val("secp256k1", vals[22].pub_key[:32], 10)] + vals[23:]
    assert add("full", secpshort, good)[2] == 22
    # all secp256k1: by key bytes, and by registered keys with the key-set cache on
    svals = make_vals(["secp256k1"] * 70)
    sgood = R.make_commit(svals, CHAIN, HEIGHT, flags=flags)
    assert add("full", svals, sgood, cap=0, keyed=0) is None
    assert add("full", svals, sgood, cap=2, keyed=1) is None
    assert add("full", svals, flip(sgood, 69), cap=2, keyed=1)[2] == 69
    assert add("trusting", svals, sgood, cap=2, keyed=1) is None
    # every validator signing for the block: the caller's arrays are the batch (no partition)
    sall = R.make_commit(svals, CHAIN, HEIGHT)
    assert add("full", svals, sall, cap=0, keyed=0) is None
    assert add("full", svals, sall, cap=2, keyed=1) is None
    assert add("full", svals, flip(sall, 0), cap=2, keyed=1)[2] == 0
    assert add("light", svals, flip(sall, 69), cap=0, keyed=0) is None
    # a mixed set never registers
    assert add("full", vals, good, cap=2, keyed=0) is None

    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<I", len(cases)) + b"".join(cases))
    try:
        b = _build()
    except (OSError, subprocess.CalledProcessError, AssertionError) as e:
        pytest.fail(f"could not build typedcheck: {e}")
    r = subprocess.run([b, str(path)], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1",
                            "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    assert f"typedcheck ok ({len(cases)} cases)" in r.stdout
