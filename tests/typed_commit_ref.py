"""The reference's three commit-verification loops restated in Python over
per-type signature verifiers, for validator sets of Ed25519, secp256k1 and
sr25519 keys (and sets that mix them): where the typed commit tests take
their expected outcomes from.

  VerifyCommit               types/validator_set.go:667-714
  VerifyCommitLight          types/validator_set.go:722-765
  VerifyCommitLightTrusting  types/validator_set.go:775-826
  PubKey.VerifySignature     crypto/ed25519/ed25519.go:148, crypto/secp256k1/secp256k1.go:192,
                             crypto/sr25519/pubkey.go:34
  PubKey.Address / String    the same files; Validator.String types/validator.go

Verifiers: oracle/ed25519_ref.verify, tests/secp256k1_ref.verify,
oracle/sr25519_ref.verify; sign-bytes: oracle/signbytes.py; signatures: the
three reference signers. An outcome is None (nil) or (kind, message, index)
with kind one of "set_size", "height", "block_id", "wrong_signature",
"not_enough_power", "double_vote", "trust_level", "panic".
"""
from __future__ import annotations

import hashlib
import os
import sys
from dataclasses import dataclass
from functools import lru_cache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import secp256k1_ref as SECP  # noqa: E402

from cometbft_amd.ripemd160 import ripemd160  # noqa: E402
from oracle import ed25519_ref as ED  # noqa: E402
from oracle import signbytes as SB  # noqa: E402
from oracle import sr25519_ref as SR  # noqa: E402

ABSENT, COMMIT, NIL = 1, 2, 3
KEY_NAMES = {"ed25519": "PubKeyEd25519", "secp256k1": "PubKeySecp256k1", "sr25519": "PubKeySr25519"}


class Panic(Exception):
    pass


@dataclass
class Val:
    key_type: str
    pub_key: bytes
    power: int
    secret: bytes = b""
    priority: int = 0

    @property
    def address(self) -> bytes:
        h = hashlib.sha256(self.pub_key).digest()
        return ripemd160(h) if self.key_type == "secp256k1" else h[:20]

    def string(self) -> str:
        return "Validator{%s %s{%s} VP:%d A:%d}" % (self.address.hex().upper(), KEY_NAMES[self.key_type],
                                                    self.pub_key.hex().upper(), self.power, self.priority)


@dataclass
class Sig:
    flag: int
    address: bytes = b""
    ts: tuple = (SB.GO_ZERO_TIME_SECONDS, 0)
    signature: bytes = b""


@lru_cache(maxsize=None)
def keypair(key_type: str, i: int):
    """Deterministic validator i of a type: (secret, public key)."""
    secret = hashlib.sha256(b"typed-commit/%s/%d" % (key_type.encode(), i)).digest()
    if key_type == "ed25519":
        return secret, ED.pubkey_from_seed(secret)
    if key_type == "secp256k1":
        return secret, SECP.pubkey_from_priv(secret)
    return secret, SR.pubkey_from_mini(secret)


# The per-type verifiers the loops call. A host test that links the commit
# layer against a double of the runtime whose "sr25519 device" is another
# algorithm swaps that entry for the double's (and signs accordingly).
VERIFIERS = {"ed25519": lambda pk, msg, sig, mode: ED.verify(pk, msg, sig, mode),
             "secp256k1": lambda pk, msg, sig, mode: SECP.verify(pk, msg, sig),
             "sr25519": lambda pk, msg, sig, mode: SR.verify(pk, msg, sig)}
SIGNERS = {"ed25519": ED.sign, "secp256k1": SECP.sign, "sr25519": SR.sign}


_memo = {}


def sign(key_type: str, secret: bytes, msg: bytes) -> bytes:
    k = (SIGNERS[key_type], secret, msg)
    if k not in _memo:
        _memo[k] = SIGNERS[key_type](secret, msg)
    return _memo[k]


def verify_signature(v: Val, msg: bytes, sig: bytes, mode: int = 0) -> bool:
    """val.PubKey.VerifySignature(msg, sig) by the key's type."""
    if len(sig) != 64:  # all three wrappers, before anything else
        return False
    if v.key_type == "ed25519" and len(v.pub_key) != 32:
        raise Panic("ed25519: bad public key length: %d" % len(v.pub_key))  # Go's ed25519.Verify
    k = (VERIFIERS[v.key_type], v.pub_key, msg, sig, mode)
    if k not in _memo:
        _memo[k] = VERIFIERS[v.key_type](v.pub_key, msg, sig, mode)
    return _memo[k]


def sign_bytes(chain_id: str, height: int, round_: int, block_id: tuple, s: Sig) -> bytes:
    """Commit.VoteSignBytes: CommitSig.BlockID(commit.BlockID) (types/block.go:652-665)."""
    if s.flag == COMMIT:
        bid = block_id
    elif s.flag in (ABSENT, NIL):
        bid = None
    else:
        raise Panic("Unknown BlockIDFlag: %d" % s.flag)
    return SB.vote_sign_bytes(chain_id, SB.PRECOMMIT, height, round_, bid, s.ts[0], s.ts[1])


def _wrong(idx, sig):
    return ("wrong_signature", "wrong signature (#%d): %s" % (idx, sig.hex().upper()), idx)


def _not_enough(got, needed):
    return ("not_enough_power",
            "invalid commit -- insufficient voting power: got %d, needed more than %d" % (got, needed), -1)


def _preamble(vals, block_id, height, c_height, c_block_id, sigs):
    if len(vals) != len(sigs):
        return ("set_size", "Invalid commit -- wrong set size: %d vs %d" % (len(vals), len(sigs)), -1)
    if height != c_height:
        return ("height", "Invalid commit -- wrong height: %d vs %d" % (height, c_height), -1)
    if block_id != c_block_id:  # (the message's "want ..., got ..." tail is not restated here)
        return ("block_id", "invalid commit -- wrong block ID", -1)
    return None


def verify_commit(vals, chain_id, block_id, height, commit, mode=0):
    """commit = (height, round, block_id tuple, [Sig])."""
    c_height, c_round, c_bid, sigs = commit
    try:
        e = _preamble(vals, block_id, height, c_height, c_bid, sigs)
        if e:
            return e
        tally, needed = 0, sum(v.power for v in vals) * 2 // 3
        for idx, s in enumerate(sigs):
            if s.flag == ABSENT:
                continue
            msg = sign_bytes(chain_id, c_height, c_round, c_bid, s)
            if not verify_signature(vals[idx], msg, s.signature, mode):
                return _wrong(idx, s.signature)
            if s.flag == COMMIT:
                tally += vals[idx].power
        return None if tally > needed else _not_enough(tally, needed)
    except Panic as p:
        return ("panic", str(p), -1)


def verify_commit_light(vals, chain_id, block_id, height, commit, mode=0):
    c_height, c_round, c_bid, sigs = commit
    try:
        e = _preamble(vals, block_id, height, c_height, c_bid, sigs)
        if e:
            return e
        tally, needed = 0, sum(v.power for v in vals) * 2 // 3
        for idx, s in enumerate(sigs):
            if s.flag != COMMIT:
                continue
            msg = sign_bytes(chain_id, c_height, c_round, c_bid, s)
            if not verify_signature(vals[idx], msg, s.signature, mode):
                return _wrong(idx, s.signature)
            tally += vals[idx].power
            if tally > needed:
                return None
        return _not_enough(tally, needed)
    except Panic as p:
        return ("panic", str(p), -1)


def verify_commit_light_trusting(vals, chain_id, commit, trust=(1, 3), mode=0):
    c_height, c_round, c_bid, sigs = commit
    num, den = trust
    try:
        if den == 0:
            return ("trust_level", "trustLevel has zero Denominator", -1)
        total = sum(v.power for v in vals)
        if total * num >= 2**63:
            return ("trust_level", "int64 overflow while calculating voting power needed. please provide smaller "
                    "trustLevel numerator", -1)
        needed = total * num // den
        by_addr = {}
        for i, v in enumerate(vals):
            by_addr.setdefault(v.address, i)  # GetByAddress: the first
        tally, seen = 0, {}
        for idx, s in enumerate(sigs):
            if s.flag != COMMIT:
                continue
            vi = by_addr.get(s.address)
            if vi is None:
                continue
            if vi in seen:
                return ("double_vote", "double vote from %s (%d and %d)" % (vals[vi].string(), seen[vi], idx), idx)
            seen[vi] = idx
            msg = sign_bytes(chain_id, c_height, c_round, c_bid, s)
            if not verify_signature(vals[vi], msg, s.signature, mode):
                return _wrong(idx, s.signature)
            tally += vals[vi].power
            if tally > needed:
                return None
        return _not_enough(tally, needed)
    except Panic as p:
        return ("panic", str(p), -1)


# ------------------------------------------------------------------ builders

def make_vals(types, power=10, start=0):
    """One validator per entry of `types`, keys from keypair(type, start + i)."""
    out = []
    for i, t in enumerate(types):
        secret, pk = keypair(t, start + i)
        out.append(Val(t, pk, power, secret))
    return out


def block_id_for(height: int) -> tuple:
    return (hashlib.sha256(b"block%d" % height).digest(), 1, hashlib.sha256(b"parts%d" % height).digest())


def timestamp_for(i: int) -> tuple:
    """Seconds and nanos that are each zero for some validators."""
    sec = 0 if i % 7 == 3 else 1672531200 + i
    nanos = 0 if i % 5 == 2 else 1000 * i + 1
    return sec, nanos


def make_commit(vals, chain_id, height, round_=0, flags=None):
    """Every present validator signs its own vote."""
    bid = block_id_for(height)
    sigs = []
    for i, v in enumerate(vals):
        f = COMMIT if flags is None else flags[i]
        if f == ABSENT:
            sigs.append(Sig(ABSENT))
            continue
        s = Sig(f, v.address, timestamp_for(i))
        s.signature = sign(v.key_type, v.secret, sign_bytes(chain_id, height, round_, bid, s))
        sigs.append(s)
    return (height, round_, bid, sigs)
