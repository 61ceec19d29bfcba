"""The secp256k1 templated per-lane functions on the CPU:
tests/host/secptmplcheck.cpp compiles cometbft_amd/csrc/secp256k1.h's
secp_verify_tmpl_one / secp_verify_keyed_tmpl_one (the body of
k_verify_secp256k1_tmpl / _keyed_tmpl: sb_write into the lane's slot, then
SHA-256 and the verdict over it) with CMTV_HD = inline and the bound
assertions on. The messages it builds must be the oracle's sign-bytes and the
verdicts tests/secp256k1_ref.verify's over them, across every SHA-256 padding
boundary a commit vote can meet."""
import os
import struct
import subprocess
import sys

import pytest

from oracle import signbytes as SB
from tests.host import hostbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import secp256k1_ref as S  # noqa: E402

SRC = os.path.join(ROOT, "tests", "host", "secptmplcheck.cpp")
BIN = os.path.join(ROOT, "build", "secptmplcheck")
HEIGHT, ROUND = 12345, 0
BLOCK_ID = (bytes(range(32)), 1, bytes(range(32, 64)))
BOUNDARIES = {55, 56, 63, 64, 119, 120}  # one- and two-block SHA-256 padding edges
N_KEYS = 3


@pytest.fixture(scope="module")
def secptmplcheck():
    return hostbuild.build(SRC, BIN, ["-std=c++17"])


def template(chain_id, height=HEIGHT, round_=ROUND, block_id=BLOCK_ID):
    """(pre(Commit), pre(Nil), post) of signbytes.h: the CanonicalVote fields
    before the timestamp with and without the BlockID, and the chain-id field."""
    head = b"\x08" + SB.uvarint(SB.PRECOMMIT) + b"\x11" + struct.pack("<q", height)
    if round_:
        head += b"\x19" + struct.pack("<q", round_)
    pre_commit = head + SB._bytes_field(0x22, SB.canonical_block_id(*block_id))
    post = SB._bytes_field(0x32, chain_id.encode()) if chain_id else b""
    return pre_commit, head, post


def record(pk, sig, tmpl, flag, sec, nanos):
    return (pk + sig + struct.pack("<3I", *(len(t) for t in tmpl)) + b"".join(tmpl) +
            struct.pack("<Bqi", 1 if flag else 0, sec, nanos))


def run(binary, records):
    inp = struct.pack("<I", len(records)) + b"".join(records)
    r = subprocess.run([binary], input=inp, capture_output=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-400:])
    out, at = [], 0
    for _ in records:
        v, vk, mlen = struct.unpack_from("<BBI", r.stdout, at)
        out.append((v, vk, r.stdout[at + 6: at + 6 + mlen]))
        at += 6 + mlen
    assert at == len(r.stdout)
    return out


def test_sweep_matches_oracle_sign_bytes_and_reference_verdicts(secptmplcheck):
    privs = [bytes([7 + k]) * 32 for k in range(N_KEYS)]
    pks = [S.pubkey_from_priv(p) for p in privs]
    cases = []  # (pk, sig, tmpl, flag, sec, nanos, oracle message)
    k = 0
    for clen in range(0, 81):
        chain = ("chain-id-" * 9)[:clen]
        tmpl = template(chain)
        for flag in (True, False):
            # seconds and nanos each zero and non-zero (a zero field is omitted)
            for sec, nanos in ((0, 0), (1700000000 + clen, 0), (0, 999 + clen), (1700000000 + clen, 123456789)):
                msg = SB.vote_sign_bytes(chain, SB.PRECOMMIT, HEIGHT, ROUND, BLOCK_ID if flag else None, sec, nanos)
                cases.append((pks[k % N_KEYS], S.sign(privs[k % N_KEYS], msg), tmpl, flag, sec, nanos, msg))
                k += 1
    lengths = {len(c[6]) for c in cases}
    assert BOUNDARIES <= lengths, sorted(BOUNDARIES - lengths)
    assert max(lengths) <= 192
    # a high-S twin (same r, s -> n - s) and a flipped message bit (the chain
    # id's first byte in the template: the signature is over the unflipped one)
    pk, sig, tmpl, flag, sec, nanos, msg = cases[300]
    twin = sig[:32] + (S.N - int.from_bytes(sig[32:], "big")).to_bytes(32, "big")
    cases.append((pk, twin, tmpl, flag, sec, nanos, msg))
    pk, sig, tmpl, flag, sec, nanos, msg = cases[301]
    post = tmpl[2][:2] + bytes([tmpl[2][2] ^ 0x04]) + tmpl[2][3:]
    at = len(msg) - len(post) + 2
    cases.append((pk, sig, (tmpl[0], tmpl[1], post), flag, sec, nanos, msg[:at] + bytes([msg[at] ^ 0x04]) + msg[at + 1:]))
    # ... and a key ParsePubKey rejects (prefix 4)
    pk, sig, tmpl, flag, sec, nanos, msg = cases[302]
    cases.append((b"\x04" + pk[1:], sig, tmpl, flag, sec, nanos, msg))
    got = run(secptmplcheck, [record(*c[:6]) for c in cases])
    want = [S.verify(c[0], c[6], c[1]) for c in cases]
    assert want[:-3] == [True] * (len(cases) - 3) and want[-3:] == [False] * 3
    for i, (c, (v, vk, built)) in enumerate(zip(cases, got)):
        assert built == c[6], (i, len(c[6]))
        assert (v, vk) == (int(want[i]), int(want[i])), (i, len(c[6]), c[3], c[4], c[5])
