"""Python mirror of the reference's commit-verification types, backed by the
C++ replay + GPU batch in libcmtverify.so (cmtv_verify_commit).

Mirrors
  BlockID / PartSetHeader           /root/reference/types/block.go:1160-1245, part_set.go:103
  CommitSig / BlockIDFlag / Commit  /root/reference/types/block.go:575-810
  Validator / ValidatorSet          /root/reference/types/validator.go, validator_set.go
  VerifyCommit                      /root/reference/types/validator_set.go:667-714
  VerifyCommitLight                 /root/reference/types/validator_set.go:722-765
  VerifyCommitLightTrusting         /root/reference/types/validator_set.go:775-826
  ErrNotEnoughVotingPowerSigned     /root/reference/types/validator_set.go:856-863
  ErrInvalidCommitHeight/Signatures /root/reference/types/errors.go:15-41
  VoteSignBytes                     /root/reference/types/vote.go:93-101

Errors are raised as exceptions whose str() is the reference's error string;
the places where the reference panics raise ReferencePanic.
"""
from __future__ import annotations

import ctypes
import hashlib
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from . import _native as N
from . import ripemd160 as _ripemd160
from .crypto import MODE_GO_STDLIB, Context, default_context

BLOCK_ID_FLAG_ABSENT = 1
BLOCK_ID_FLAG_COMMIT = 2
BLOCK_ID_FLAG_NIL = 3
PRECOMMIT_TYPE = 2
PREVOTE_TYPE = 1
GO_ZERO_TIME_SECONDS = -62135596800  # time.Time{} as Unix seconds


class CommitError(Exception):
    code = -1


class ErrInvalidCommitSignatures(CommitError):
    code = N.COMMIT_ERR_SET_SIZE


class ErrInvalidCommitHeight(CommitError):
    code = N.COMMIT_ERR_HEIGHT


class ErrWrongBlockID(CommitError):
    code = N.COMMIT_ERR_BLOCK_ID


class ErrWrongSignature(CommitError):
    code = N.COMMIT_ERR_WRONG_SIGNATURE

    def __init__(self, msg, index):
        super().__init__(msg)
        self.index = index


class ErrNotEnoughVotingPowerSigned(CommitError):
    code = N.COMMIT_ERR_NOT_ENOUGH_POWER

    def __init__(self, msg, got, needed):
        super().__init__(msg)
        self.got = got
        self.needed = needed


class ErrDoubleVote(CommitError):
    code = N.COMMIT_ERR_DOUBLE_VOTE


class ErrTrustLevel(CommitError):
    code = N.COMMIT_ERR_TRUST_LEVEL


class ReferencePanic(Exception):
    """Raised where the reference Go code would panic."""


@dataclass
class PartSetHeader:
    total: int = 0
    hash: bytes = b""


@dataclass
class BlockID:
    hash: bytes = b""
    part_set_header: PartSetHeader = field(default_factory=PartSetHeader)

    def is_zero(self) -> bool:
        return len(self.hash) == 0 and self.part_set_header.total == 0 and len(self.part_set_header.hash) == 0

    def _c(self):
        h = (ctypes.c_uint8 * max(len(self.hash), 1)).from_buffer_copy(self.hash + b"\0")
        ph = (ctypes.c_uint8 * max(len(self.part_set_header.hash), 1)).from_buffer_copy(
            self.part_set_header.hash + b"\0")
        s = N.cmtv_block_id(hash=ctypes.cast(h, ctypes.POINTER(ctypes.c_uint8)), hash_len=len(self.hash),
                            psh_total=self.part_set_header.total,
                            psh_hash=ctypes.cast(ph, ctypes.POINTER(ctypes.c_uint8)),
                            psh_hash_len=len(self.part_set_header.hash))
        return s, (h, ph)


@dataclass
class CommitSig:
    block_id_flag: int
    validator_address: bytes = b""
    timestamp: tuple = (GO_ZERO_TIME_SECONDS, 0)  # (unix seconds, nanos)
    signature: bytes = b""

    def for_block(self) -> bool:
        return self.block_id_flag == BLOCK_ID_FLAG_COMMIT

    def absent(self) -> bool:
        return self.block_id_flag == BLOCK_ID_FLAG_ABSENT


def new_commit_sig_absent() -> CommitSig:
    return CommitSig(BLOCK_ID_FLAG_ABSENT)


@dataclass
class Commit:
    height: int
    round: int
    block_id: BlockID
    signatures: list

    def vote_sign_bytes(self, chain_id: str, val_idx: int) -> bytes:
        """Commit.VoteSignBytes (types/block.go:807)."""
        cs = self.signatures[val_idx]
        if cs.block_id_flag == BLOCK_ID_FLAG_COMMIT:
            bid = self.block_id
        elif cs.block_id_flag in (BLOCK_ID_FLAG_ABSENT, BLOCK_ID_FLAG_NIL):
            bid = BlockID()
        else:
            raise ReferencePanic(f"Unknown BlockIDFlag: {cs.block_id_flag}")
        return vote_sign_bytes(chain_id, PRECOMMIT_TYPE, self.height, self.round, bid, *cs.timestamp)

    def hash(self, ctx: Context | None = None) -> bytes:
        """Commit.Hash() (types/block.go:894) on the device (cmtv_commit_hash)."""
        ctx = ctx or default_context()
        cm, keep = _pack_commit(self)
        out = (ctypes.c_uint8 * 32)()
        N.check(N.lib().cmtv_commit_hash(ctx.handle, ctypes.byref(cm), out), "cmtv_commit_hash")
        return bytes(out)


def vote_sign_bytes(chain_id: str, vote_type: int, height: int, round_: int, block_id: Optional[BlockID],
                    ts_seconds: int, ts_nanos: int) -> bytes:
    """VoteSignBytes (types/vote.go:93) through the library's encoder."""
    cid = chain_id.encode()
    bid = block_id or BlockID()
    cb, keep = bid._c()
    buf = (ctypes.c_uint8 * 512)()
    n = N.lib().cmtv_vote_sign_bytes(cid, len(cid), vote_type, height, round_, ctypes.byref(cb), ts_seconds,
                                     ts_nanos, buf, 512)
    if n < 0:
        raise N.CmtvError(int(n), "cmtv_vote_sign_bytes")
    if n > 512:
        buf = (ctypes.c_uint8 * n)()
        n = N.lib().cmtv_vote_sign_bytes(cid, len(cid), vote_type, height, round_, ctypes.byref(cb), ts_seconds,
                                         ts_nanos, buf, n)
    return bytes(buf[:n])


@dataclass
class Validator:
    pub_key: bytes
    voting_power: int
    proposer_priority: int = 0
    key_type: str = "ed25519"  # or "secp256k1", "sr25519" (types/params.go ABCIPubKeyType*)

    @property
    def address(self) -> bytes:
        """PubKey.Address(): SHA-256(pubkey)[:20] for Ed25519 and sr25519
        (crypto/ed25519/ed25519.go:136, crypto/sr25519/pubkey.go:27),
        RIPEMD160(SHA-256(pubkey)) for secp256k1 (crypto/secp256k1/secp256k1.go:152)."""
        if self.key_type not in N.KEY_TYPES:
            raise ValueError(f"unknown key type {self.key_type!r}")
        h = hashlib.sha256(self.pub_key).digest()
        return _ripemd160.ripemd160(h) if self.key_type == "secp256k1" else h[:20]

    def bytes(self) -> bytes:
        """Validator.Bytes() (types/validator.go:117), the leaf of
        ValidatorSet.Hash(), through the library's host encoder."""
        if self.key_type not in N.KEY_TYPES:
            raise ValueError(f"unknown key type {self.key_type!r}")
        pk = (ctypes.c_uint8 * max(len(self.pub_key), 1)).from_buffer_copy(self.pub_key or b"\0")
        buf = (ctypes.c_uint8 * 96)()
        n = N.lib().cmtv_validator_bytes(N.KEY_TYPES[self.key_type], pk, len(self.pub_key), self.voting_power, buf, 96)
        if n < 0:
            raise N.CmtvError(int(n), "cmtv_validator_bytes")
        return bytes(buf[:n])


class ValidatorSet:
    def __init__(self, validators: Sequence[Validator]):
        self.validators = list(validators)
        self._packed = None

    def size(self) -> int:
        return len(self.validators)

    def total_voting_power(self) -> int:
        return sum(v.voting_power for v in self.validators)

    def _pack(self):
        if self._packed is None:
            vals = self.validators
            pks = b"".join(v.pub_key for v in vals)
            off = np.zeros(len(vals) + 1, np.uint32)
            off[1:] = np.cumsum([len(v.pub_key) for v in vals]) if vals else []
            pk = np.frombuffer(pks + b"\0", np.uint8).copy()
            vp = np.array([v.voting_power for v in vals] + [0], np.int64)
            pp = np.array([v.proposer_priority for v in vals] + [0], np.int64)
            ad = np.frombuffer(b"".join(v.address for v in vals) + b"\0", np.uint8).copy()
            kt = np.array([N.KEY_TYPES[v.key_type] for v in vals] + [0], np.uint8)
            self._packed = (pk, off, vp, pp, ad, kt)
        pk, off, vp, pp, ad, kt = self._packed
        s = N.cmtv_valset(n_vals=len(self.validators), pubkeys=_p8(pk), pk_off=_p32(off),
                          voting_power=vp.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), addrs=_p8(ad),
                          proposer_priority=pp.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
        return s, self._packed

    def hash(self, ctx: Context | None = None) -> bytes:
        """ValidatorSet.Hash() (types/validator_set.go:347) on the device (cmtv_valset_hash)."""
        ctx = ctx or default_context()
        vs, keep = self._pack()
        out = (ctypes.c_uint8 * 32)()
        N.check(N.lib().cmtv_valset_hash(ctx.handle, ctypes.byref(vs), _key_types(keep[5]), out), "cmtv_valset_hash")
        return bytes(out)

    # ----------------------------------------------------------------- verify
    def verify_commit(self, chain_id: str, block_id: BlockID, height: int, commit: Commit,
                      ctx: Context | None = None, mode: int = MODE_GO_STDLIB):
        return _verify(self, N.VERIFY_COMMIT, chain_id, block_id, height, commit, 0, 0, ctx, mode)

    def verify_commit_light(self, chain_id: str, block_id: BlockID, height: int, commit: Commit,
                            ctx: Context | None = None, mode: int = MODE_GO_STDLIB):
        return _verify(self, N.VERIFY_COMMIT_LIGHT, chain_id, block_id, height, commit, 0, 0, ctx, mode)

    def verify_commit_light_trusting(self, chain_id: str, commit: Commit, trust_level=(1, 3),
                                     ctx: Context | None = None, mode: int = MODE_GO_STDLIB):
        num, den = trust_level
        return _verify(self, N.VERIFY_COMMIT_LIGHT_TRUSTING, chain_id, None, 0, commit, num, den, ctx, mode)


def _p8(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def _p32(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


class _Arena:
    """Carves arrays out of one pinned block (a cgo shim's argument arena in
    cmtv_alloc_pinned memory), 8-byte aligned."""

    def __init__(self, block):
        self.block, self.at = block, 0

    def put(self, a: np.ndarray) -> np.ndarray:
        a = np.ascontiguousarray(a)
        out = self.block.array(a.dtype, a.size, self.at).reshape(a.shape)
        out[...] = a
        self.at += (a.nbytes + 7) // 8 * 8
        return out


def _pack_commit(commit: Commit, arena: _Arena | None = None):
    sigs = commit.signatures
    n = len(sigs)
    flags = np.array([s.block_id_flag for s in sigs] + [0], np.uint8)
    ts_s = np.array([s.timestamp[0] for s in sigs] + [0], np.int64)
    ts_n = np.array([s.timestamp[1] for s in sigs] + [0], np.int32)
    sb = np.frombuffer(b"".join(s.signature for s in sigs) + b"\0", np.uint8).copy()
    so = np.zeros(n + 1, np.uint32)
    if n:
        so[1:] = np.cumsum([len(s.signature) for s in sigs])
    if arena is not None:  # per commit flags | secs | nanos | sig_off | sigs, as INTEGRATION.md's arena
        flags, ts_s, ts_n, so, sb = (arena.put(x) for x in (flags, ts_s, ts_n, so, sb))
    addrs = b"".join((s.validator_address + bytes(20))[:20] for s in sigs)
    ad = np.frombuffer(addrs + b"\0", np.uint8).copy()
    bid, keep = commit.block_id._c()
    c = N.cmtv_commit(height=commit.height, round=commit.round, block_id=bid, n_sigs=n, flags=_p8(flags),
                      ts_seconds=ts_s.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                      ts_nanos=ts_n.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), sigs=_p8(sb), sig_off=_p32(so),
                      val_addrs=_p8(ad))
    return c, (flags, ts_s, ts_n, sb, so, ad, keep)


def _key_types(kt: np.ndarray):
    """The packed CMTV_KEY_* array of a set, or None (NULL) when every key is Ed25519."""
    return _p8(kt) if kt[:-1].any() else None


def _roots(buf, n: int) -> list:
    raw = bytes(buf)
    return [raw[32 * i: 32 * i + 32] for i in range(n)]


def merkle_roots(trees, ctx: Context | None = None) -> list:
    """HashFromByteSlices (crypto/merkle/tree.go:9) of every tree, a sequence
    of sequences of byte strings, in one cmtv_merkle_roots call."""
    ctx = ctx or default_context()
    trees = [list(t) for t in trees]
    if not trees:
        return []
    items = [it for t in trees for it in t]
    tree_off = np.zeros(len(trees) + 1, np.uint32)
    tree_off[1:] = np.cumsum([len(t) for t in trees])
    item_off = np.zeros(len(items) + 1, np.uint32)
    if items:
        item_off[1:] = np.cumsum([len(it) for it in items])
    blob = np.frombuffer(b"".join(items) + b"\0", np.uint8).copy()
    out = (ctypes.c_uint8 * (32 * len(trees)))()
    N.check(N.lib().cmtv_merkle_roots(ctx.handle, len(trees), _p32(tree_off), _p8(blob), _p32(item_off), out),
            "cmtv_merkle_roots")
    return _roots(out, len(trees))


def merkle_root(items, ctx: Context | None = None) -> bytes:
    """HashFromByteSlices of one list of byte strings (cmtv_merkle_root)."""
    ctx = ctx or default_context()
    items = list(items)
    item_off = np.zeros(len(items) + 1, np.uint32)
    if items:
        item_off[1:] = np.cumsum([len(it) for it in items])
    blob = np.frombuffer(b"".join(items) + b"\0", np.uint8).copy()
    out = (ctypes.c_uint8 * 32)()
    N.check(N.lib().cmtv_merkle_root(ctx.handle, len(items), _p8(blob), _p32(item_off), out), "cmtv_merkle_root")
    return bytes(out)


def valset_hashes(sets, ctx: Context | None = None) -> list:
    """ValidatorSet.Hash() of every set in one cmtv_valset_hashes call."""
    ctx = ctx or default_context()
    sets = list(sets)
    if not sets:
        return []
    vs_arr = (N.cmtv_valset * len(sets))()
    kt_arr = (ctypes.POINTER(ctypes.c_uint8) * len(sets))()
    keep = []
    for i, s in enumerate(sets):
        vs_arr[i], kv = s._pack()
        kt = _key_types(kv[5])
        if kt is not None:
            kt_arr[i] = kt
        keep.append(kv)
    out = (ctypes.c_uint8 * (32 * len(sets)))()
    N.check(N.lib().cmtv_valset_hashes(ctx.handle, len(sets), vs_arr, kt_arr, out), "cmtv_valset_hashes")
    return _roots(out, len(sets))


def commit_hashes(commits, ctx: Context | None = None) -> list:
    """Commit.Hash() of every commit in one cmtv_commit_hashes call."""
    ctx = ctx or default_context()
    commits = list(commits)
    if not commits:
        return []
    cm_arr = (N.cmtv_commit * len(commits))()
    keep = []
    for i, c in enumerate(commits):
        cm_arr[i], kc = _pack_commit(c)
        keep.append(kc)
    out = (ctypes.c_uint8 * (32 * len(commits)))()
    N.check(N.lib().cmtv_commit_hashes(ctx.handle, len(commits), cm_arr, out), "cmtv_commit_hashes")
    return _roots(out, len(commits))


@dataclass
class Header:
    """types/block.go Header, the fields Hash() reads, in struct order."""
    version_block: int = 0
    version_app: int = 0
    chain_id: str = ""
    height: int = 0
    time: tuple = (GO_ZERO_TIME_SECONDS, 0)  # (unix seconds, nanos)
    last_block_id: BlockID = field(default_factory=BlockID)
    last_commit_hash: bytes = b""
    data_hash: bytes = b""
    validators_hash: bytes = b""
    next_validators_hash: bytes = b""
    consensus_hash: bytes = b""
    app_hash: bytes = b""
    last_results_hash: bytes = b""
    evidence_hash: bytes = b""
    proposer_address: bytes = b""

    def _bytes_fields(self) -> tuple:
        """The nine byte fields in CMTV_HDR_* order."""
        return (self.last_commit_hash, self.data_hash, self.validators_hash, self.next_validators_hash,
                self.consensus_hash, self.app_hash, self.last_results_hash, self.evidence_hash, self.proposer_address)

    def _c(self):
        cid = self.chain_id.encode()
        bid, keep = self.last_block_id._c()
        h = N.cmtv_header(version_block=self.version_block, version_app=self.version_app, chain_id=cid,
                          chain_id_len=len(cid), height=self.height, time_seconds=self.time[0],
                          time_nanos=self.time[1], last_block_id=bid)
        bufs = []
        for i, b in enumerate(self._bytes_fields()):
            buf = (ctypes.c_uint8 * max(len(b), 1)).from_buffer_copy(b + b"\0")
            h.field[i] = ctypes.cast(buf, ctypes.POINTER(ctypes.c_uint8))
            h.field_len[i] = len(b)
            bufs.append(buf)
        return h, (cid, keep, bufs)

    def hash(self, ctx: Context | None = None) -> Optional[bytes]:
        """Header.Hash() (types/block.go:440) on the device (cmtv_header_hash);
        None where the reference returns nil."""
        return header_hashes([self], ctx)[0]


def header_hashes(headers, ctx: Context | None = None) -> list:
    """Header.Hash() of every header in one cmtv_header_hashes call; None for a
    header without a hash."""
    ctx = ctx or default_context()
    headers = list(headers)
    if not headers:
        return []
    arr = (N.cmtv_header * len(headers))()
    keep = []
    for i, h in enumerate(headers):
        arr[i], kh = h._c()
        keep.append(kh)
    out = (ctypes.c_uint8 * (32 * len(headers)))()
    has = (ctypes.c_uint8 * len(headers))()
    N.check(N.lib().cmtv_header_hashes(ctx.handle, len(headers), arr, out, has), "cmtv_header_hashes")
    return [r if ok else None for r, ok in zip(_roots(out, len(headers)), has)]


def txs_hashes(blocks, ctx: Context | None = None) -> list:
    """Txs.Hash() (types/tx.go:47) of every block's transaction list, a
    sequence of sequences of byte strings, in one cmtv_txs_hashes call."""
    ctx = ctx or default_context()
    blocks = [list(b) for b in blocks]
    if not blocks:
        return []
    txs = [tx for b in blocks for tx in b]
    block_off = np.zeros(len(blocks) + 1, np.uint32)
    block_off[1:] = np.cumsum([len(b) for b in blocks])
    tx_off = np.zeros(len(txs) + 1, np.uint32)
    if txs:
        tx_off[1:] = np.cumsum([len(tx) for tx in txs])
    blob = np.frombuffer(b"".join(txs) + b"\0", np.uint8).copy()
    out = (ctypes.c_uint8 * (32 * len(blocks)))()
    N.check(N.lib().cmtv_txs_hashes(ctx.handle, len(blocks), _p32(block_off), _p8(blob), _p32(tx_off), out),
            "cmtv_txs_hashes")
    return _roots(out, len(blocks))


def txs_hash(txs, ctx: Context | None = None) -> bytes:
    """Txs.Hash() of one list of transactions (cmtv_txs_hash)."""
    ctx = ctx or default_context()
    txs = list(txs)
    tx_off = np.zeros(len(txs) + 1, np.uint32)
    if txs:
        tx_off[1:] = np.cumsum([len(tx) for tx in txs])
    blob = np.frombuffer(b"".join(txs) + b"\0", np.uint8).copy()
    out = (ctypes.c_uint8 * 32)()
    N.check(N.lib().cmtv_txs_hash(ctx.handle, len(txs), _p8(blob), _p32(tx_off), out), "cmtv_txs_hash")
    return bytes(out)


# ---------------------------------------------------------------- merkle proofs
MAX_AUNTS = 100  # crypto/merkle/proof.go MaxAunts
HASH_SIZE = 32   # tmhash.Size


def _p64(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def _pack_items(items):
    """(blob, offsets) of a list of byte strings, as the C calls take them."""
    off = np.zeros(len(items) + 1, np.uint32)
    if items:
        off[1:] = np.cumsum([len(it) for it in items])
    return np.frombuffer(b"".join(items) + b"\0\0\0\0", np.uint8).copy(), off


def _proof_error(status: int, proof, root, out_hash: bytes):
    """Proof.Verify's error string (proof.go:52-74) for a status of cmtv_merkle_proofs_verify."""
    if status == N.PROOF_OK:
        return None
    if status == N.PROOF_ENEGTOTAL:
        return "proof total must be positive"
    if status == N.PROOF_ENEGINDEX:
        return "proof index cannot be negative"
    if status == N.PROOF_ELEAF:
        return f"invalid leaf hash: wanted {out_hash.hex().upper()} got {proof.leaf_hash.hex().upper()}"
    if status == N.PROOF_EINDEX:
        return f"compute root hash: invalid index {proof.index} and/or total {proof.total}"
    if status == N.PROOF_EEXTRA:
        return "compute root hash: unexpected inner hashes"
    if status == N.PROOF_EMISSING:
        return "compute root hash: expected at least one inner hash"
    return f"invalid root hash: wanted {root.hex().upper()} got {out_hash.hex().upper()}"


def _verify_proofs_raw(proofs, roots, leaves, leaf_kind, root_idx, ctx):
    """(status, out_hash) per proof from one cmtv_merkle_proofs_verify call.
    Any number of aunts goes to the device (more than 63 cannot verify). A
    leaf hash that is not 32 bytes cannot equal a computed one: with leaves the
    device is given zeros in its place, which fail the same check, and the
    error string quotes the proof's own. Where the reference would go on to
    hash a leaf hash (no leaf check) or an aunt of another size as it is, this
    raises ValueError with ValidateBasic's string instead."""
    ctx = ctx or default_context()
    n = len(proofs)
    if n == 0:
        return [], []
    for p in proofs:
        for i, a in enumerate(p.aunts):
            if len(a) != HASH_SIZE:
                raise ValueError(f"expected Aunts#{i} size to be {HASH_SIZE}, got {len(a)}")
        if len(p.leaf_hash) != HASH_SIZE and leaves is None:
            raise ValueError(f"expected LeafHash size to be {HASH_SIZE}, got {len(p.leaf_hash)}")
    total = np.array([p.total for p in proofs], np.int64)
    index = np.array([p.index for p in proofs], np.int64)
    lh = np.frombuffer(b"".join(p.leaf_hash if len(p.leaf_hash) == HASH_SIZE else bytes(HASH_SIZE) for p in proofs),
                       np.uint8).copy()
    aunts, aunt_off = _pack_items([b"".join(p.aunts) for p in proofs])
    aunt_off //= HASH_SIZE
    rblob = _p8(np.frombuffer(b"".join(roots), np.uint8).copy()) if roots is not None else None
    ridx = _p32(np.asarray(root_idx, np.uint32)) if root_idx is not None else None
    if leaves is not None:
        lblob, loff = _pack_items(list(leaves))
        lblob, loff = _p8(lblob), _p32(loff)
    else:
        lblob, loff = None, None
    status = (ctypes.c_uint8 * n)()
    out = (ctypes.c_uint8 * (32 * n))()
    N.check(N.lib().cmtv_merkle_proofs_verify(ctx.handle, n, _p64(total), _p64(index), _p8(lh), _p32(aunt_off),
                                              _p8(aunts), len(roots) if roots is not None else 0, rblob, ridx, lblob,
                                              loff, leaf_kind, status, out, None), "cmtv_merkle_proofs_verify")
    return list(status), _roots(out, n)


@dataclass
class Proof:
    """crypto/merkle/proof.go Proof: aunts run from the leaf's sibling up to a child of the root."""
    total: int
    index: int
    leaf_hash: bytes
    aunts: list = field(default_factory=list)

    def validate_shape(self) -> Optional[str]:
        """The size rules of ValidateBasic, which the device calls rely on."""
        if len(self.leaf_hash) != HASH_SIZE:
            return f"expected LeafHash size to be {HASH_SIZE}, got {len(self.leaf_hash)}"
        if len(self.aunts) > MAX_AUNTS:
            return f"expected no more than {MAX_AUNTS} aunts, got {len(self.aunts)}"
        for i, a in enumerate(self.aunts):
            if len(a) != HASH_SIZE:
                return f"expected Aunts#{i} size to be {HASH_SIZE}, got {len(a)}"
        return None

    def validate_basic(self) -> None:
        """ValidateBasic (proof.go:113), pure Python; raises ValueError."""
        if self.total < 0:
            raise ValueError("negative Total")
        if self.index < 0:
            raise ValueError("negative Index")
        err = self.validate_shape()
        if err is not None:
            raise ValueError(err)

    def verify(self, root, leaf: bytes, ctx: Context | None = None) -> None:
        """Proof.Verify (proof.go:52) on the device; raises ValueError with the reference's string."""
        if root is None:
            raise ValueError("invalid root hash: cannot be nil")
        err = verify_proofs([self], [bytes(root)], [leaf], ctx=ctx)[0]
        if err is not None:
            raise ValueError(err)

    def compute_root_hash(self, ctx: Context | None = None) -> bytes:
        """ComputeRootHash (proof.go:77); ReferencePanic where the reference panics."""
        st, out = _verify_proofs_raw([self], None, None, N.PROOF_LEAF_ITEM, None, ctx)
        if st[0] != N.PROOF_OK:
            # (no leaf and no root is checked: the statuses left are those of computeHashFromAunts,
            # after the two sign checks, which ComputeRootHash reports as an invalid index)
            status = N.PROOF_EINDEX if st[0] in (N.PROOF_ENEGTOTAL, N.PROOF_ENEGINDEX) else st[0]
            msg = _proof_error(status, self, b"", out[0])[len("compute root hash: "):]
            raise ReferencePanic(f"ComputeRootHash errored {msg}")
        return out[0]


def verify_proofs(proofs, roots, leaves, leaf_kind: int = N.PROOF_LEAF_ITEM, root_idx=None,
                  ctx: Context | None = None) -> list:
    """Proof.Verify of every proof in one cmtv_merkle_proofs_verify call: None,
    or the reference's error string. roots: one per proof, or any number with
    root_idx naming each proof's. leaves: the leaf bytes per proof, or None for
    no leaf check. A root that is not 32 bytes cannot match (Verify compares
    the bytes): it is compared on the host. A leaf hash of another size and
    more than 100 aunts get Verify's own strings ("invalid leaf hash ...",
    "unexpected inner hashes"), not ValidateBasic's; an aunt of another size
    raises ValueError with ValidateBasic's string (_verify_proofs_raw)."""
    proofs = list(proofs)
    roots = [bytes(r) for r in roots]
    dev_roots = [r if len(r) == HASH_SIZE else bytes(HASH_SIZE) for r in roots]
    st, out = _verify_proofs_raw(proofs, dev_roots, leaves, leaf_kind, root_idx, ctx)
    errs = []
    for i, p in enumerate(proofs):
        root = roots[root_idx[i] if root_idx is not None else i]
        status = st[i]
        if status in (N.PROOF_OK, N.PROOF_EROOT):
            status = N.PROOF_OK if out[i] == root else N.PROOF_EROOT
        errs.append(_proof_error(status, p, root, out[i]))
    return errs


@dataclass
class TxProof:
    """types/tx.go:96 TxProof."""
    root_hash: bytes
    data: bytes
    proof: Proof

    def leaf(self) -> bytes:
        return hashlib.sha256(self.data).digest()

    def validate(self, data_hash: bytes, ctx: Context | None = None) -> None:
        """TxProof.Validate (types/tx.go:109); raises ValueError with the reference's string."""
        if bytes(data_hash) != bytes(self.root_hash):
            raise ValueError("proof matches different data hash")
        if self.proof.index < 0:
            raise ValueError("proof index cannot be negative")
        if self.proof.total <= 0:
            raise ValueError("proof total must be positive")
        if any(len(a) != HASH_SIZE for a in self.proof.aunts) or \
                verify_proofs([self.proof], [self.root_hash], [self.data], N.PROOF_LEAF_TX, ctx=ctx)[0] is not None:
            raise ValueError("proof is not internally consistent")


def _proofs_call(fn, name, trees, ctx):
    ctx = ctx or default_context()
    trees = [list(t) for t in trees]
    if not trees:
        return []
    items = [it for t in trees for it in t]
    tree_off = np.zeros(len(trees) + 1, np.uint32)
    tree_off[1:] = np.cumsum([len(t) for t in trees])
    blob, item_off = _pack_items(items)
    n_aunts = ctypes.c_uint64()
    N.check(N.lib().cmtv_merkle_proofs_len(len(trees), _p32(tree_off), ctypes.byref(n_aunts)),
            "cmtv_merkle_proofs_len")
    roots = (ctypes.c_uint8 * (32 * len(trees)))()
    lh = (ctypes.c_uint8 * (32 * max(len(items), 1)))()
    aunt_off = np.zeros(len(items) + 1, np.uint32)
    aunts = (ctypes.c_uint8 * (32 * max(n_aunts.value, 1)))()
    N.check(fn(ctx.handle, len(trees), _p32(tree_off), _p8(blob), _p32(item_off), roots, lh, _p32(aunt_off), aunts,
               n_aunts.value), name)
    return _split_proofs(_roots(roots, len(trees)), [len(t) for t in trees], bytes(lh), aunt_off, bytes(aunts))


def _split_proofs(roots, sizes, lh, aunt_off, aunts):
    """[(root, [Proof])] per tree from a building call's flat outputs."""
    out, g = [], 0
    for root, n in zip(roots, sizes):
        proofs = []
        for i in range(n):
            a, b = int(aunt_off[g]), int(aunt_off[g + 1])
            proofs.append(Proof(n, i, lh[32 * g: 32 * g + 32], [aunts[32 * k: 32 * k + 32] for k in range(a, b)]))
            g += 1
        out.append((root, proofs))
    return out


def proofs_from_trees(trees, ctx: Context | None = None) -> list:
    """ProofsFromByteSlices (proof.go:35) of every tree in one
    cmtv_merkle_proofs call: [(root, [Proof])]."""
    return _proofs_call(N.lib().cmtv_merkle_proofs, "cmtv_merkle_proofs", trees, ctx)


def proofs_from_byte_slices(items, ctx: Context | None = None):
    """ProofsFromByteSlices of one list of byte strings: (root, [Proof])."""
    return proofs_from_trees([items], ctx)[0]


def txs_proofs(txs, ctx: Context | None = None):
    """Txs.Proof(i) (types/tx.go:80) for every i in one cmtv_txs_proofs call: (root, [TxProof])."""
    txs = list(txs)
    root, proofs = _proofs_call(N.lib().cmtv_txs_proofs, "cmtv_txs_proofs", [txs], ctx)[0]
    return root, [TxProof(root, tx, p) for tx, p in zip(txs, proofs)]


def part_set_from_data(data: bytes, part_size: int = 65536, ctx: Context | None = None):
    """NewPartSetFromData (types/part_set.go:166) through cmtv_part_set_proofs:
    (PartSetHeader, [Proof]), part i being data[i * part_size: (i + 1) * part_size]."""
    ctx = ctx or default_context()
    if part_size <= 0 or len(data) + part_size > 2**32:
        raise ValueError("part_size must be positive and len(data) + part_size at most 2^32")
    n = (len(data) + part_size - 1) // part_size
    n_aunts = sum(N.lib().cmtv_merkle_proof_len(n, i) for i in range(n))
    blob = np.frombuffer(bytes(data) + b"\0\0\0\0", np.uint8).copy()
    total = ctypes.c_uint32()
    root = (ctypes.c_uint8 * 32)()
    lh = (ctypes.c_uint8 * (32 * max(n, 1)))()
    aunt_off = np.zeros(n + 1, np.uint32)
    aunts = (ctypes.c_uint8 * (32 * max(n_aunts, 1)))()
    N.check(N.lib().cmtv_part_set_proofs(ctx.handle, _p8(blob), len(data), part_size, ctypes.byref(total), root, lh,
                                         _p32(aunt_off), aunts, n_aunts), "cmtv_part_set_proofs")
    (r, proofs), = _split_proofs([bytes(root)], [total.value], bytes(lh), aunt_off, bytes(aunts))
    return PartSetHeader(total.value, r), proofs


def _verify(vals: ValidatorSet, kind, chain_id, block_id, height, commit, num, den, ctx, mode):
    ctx = ctx or default_context()
    vs, keep_v = vals._pack()
    cm, keep_c = _pack_commit(commit)
    if block_id is not None:
        bid, keep_b = block_id._c()
        bidp = ctypes.byref(bid)
    else:
        bidp, keep_b = None, None
    res = N.cmtv_commit_result()
    buf = ctypes.create_string_buffer(4096)
    cid = chain_id.encode()
    kt = keep_v[5]
    if kt[:-1].any():  # a validator that is not Ed25519: the typed entry point
        rc = N.lib().cmtv_verify_commit_typed(ctx.handle, kind, mode, cid, len(cid), ctypes.byref(vs), _p8(kt), bidp,
                                              height, ctypes.byref(cm), num, den, ctypes.byref(res), buf, len(buf))
    else:
        rc = N.lib().cmtv_verify_commit(ctx.handle, kind, mode, cid, len(cid), ctypes.byref(vs), bidp, height,
                                        ctypes.byref(cm), num, den, ctypes.byref(res), buf, len(buf))
    N.check(rc, "cmtv_verify_commit")
    err = _error_for(rc, res, buf.value.decode())
    if err is not None:
        raise err
    return None


def _error_for(rc, res, msg):
    """The exception the reference's VerifyCommit* would produce (None = nil)."""
    if rc == N.CMTV_OK:
        return None
    code = res.code
    if code == N.COMMIT_ERR_SET_SIZE:
        return ErrInvalidCommitSignatures(msg)
    if code == N.COMMIT_ERR_HEIGHT:
        return ErrInvalidCommitHeight(msg)
    if code == N.COMMIT_ERR_BLOCK_ID:
        return ErrWrongBlockID(msg)
    if code == N.COMMIT_ERR_WRONG_SIGNATURE:
        return ErrWrongSignature(msg, res.sig_index)
    if code == N.COMMIT_ERR_NOT_ENOUGH_POWER:
        return ErrNotEnoughVotingPowerSigned(msg, res.got, res.needed)
    if code == N.COMMIT_ERR_DOUBLE_VOTE:
        e = ErrDoubleVote(msg)
        e.result = N.cmtv_commit_result.from_buffer_copy(res)
        return e
    if code == N.COMMIT_ERR_TRUST_LEVEL:
        return ErrTrustLevel(msg)
    if code in (N.COMMIT_PANIC_BAD_PUBKEY, N.COMMIT_PANIC_UNKNOWN_FLAG):
        return ReferencePanic(msg)
    return CommitError(msg)


def verify_commits(kind: int, chain_id: str, items, ctx: Context | None = None, mode: int = MODE_GO_STDLIB,
                   trust_level=(1, 3)):
    """Cross-height batching (cmtv_verify_commits; cmtv_verify_commits_typed
    when a validator of any item holds a secp256k1 or sr25519 key): items is a
    sequence of (ValidatorSet, BlockID | None, height, Commit). All their
    signatures go to the device in ONE batch per key type; returns, per item, None (the reference's nil) or
    the exception its VerifyCommit* would have returned -- not raised, so one
    bad height does not hide the others."""
    if len(items) == 0:
        return []
    return PackedCommits(kind, chain_id, items, mode, trust_level).verify(ctx or default_context())


class PackedCommits:
    """The C arguments of one cmtv_verify_commits call, packed once (what a
    cgo shim holds when it calls the library); verify() makes the call."""

    def __init__(self, kind: int, chain_id: str, items, mode: int = MODE_GO_STDLIB, trust_level=(1, 3),
                 pinned: Context | None = None):
        """pinned: the commits' arrays in one cmtv_alloc_pinned block of that
        context (the direct, zero-copy chunks of cmtv_verify_commits there)."""
        n = len(items)
        keep = []
        arena = None
        if pinned is not None:
            nb = 4096 + sum(80 + 24 * (len(c.signatures) + 1) + sum(len(s.signature) for s in c.signatures)
                            for _, _, _, c in items)
            self.block = pinned.alloc_pinned(nb)
            arena = _Arena(self.block)
        vs_arr = (N.cmtv_valset * n)()
        cm_arr = (N.cmtv_commit * n)()
        bid_arr = (N.cmtv_block_id * n)()
        heights = (ctypes.c_int64 * n)()
        # one CMTV_KEY_* array per set that is not all Ed25519, else NULL
        kt_arr = (ctypes.POINTER(ctypes.c_uint8) * n)()
        typed = False
        for c, (vals, block_id, height, commit) in enumerate(items):
            vs, kv = vals._pack()
            cm, kc = _pack_commit(commit, arena)
            vs_arr[c], cm_arr[c] = vs, cm
            if kv[5][:-1].any():
                kt_arr[c] = _p8(kv[5])
                typed = True
            keep += [kv, kc]
            if block_id is not None:
                bid, kb = block_id._c()
                bid_arr[c] = bid
                keep.append(kb)
            heights[c] = height
        self.n, self.kind, self.mode, self.cap = n, kind, mode, 1024
        self.cid = chain_id.encode()
        self.num, self.den = trust_level if kind == N.VERIFY_COMMIT_LIGHT_TRUSTING else (0, 0)
        self.vs_arr, self.cm_arr, self.heights, self._keep = vs_arr, cm_arr, heights, keep
        self.bid_arr = bid_arr if kind != N.VERIFY_COMMIT_LIGHT_TRUSTING else None
        self.kt_arr = kt_arr if typed else None
        self.res = (N.cmtv_commit_result * n)()
        self.rcs = (ctypes.c_int * n)()
        self.bufs = ctypes.create_string_buffer(n * self.cap)

    def call(self, ctx: Context) -> None:
        """The C call alone (results left in res / rcs / bufs): the typed
        entry point when a validator of any item is not Ed25519."""
        if self.kt_arr is not None:
            rc = N.lib().cmtv_verify_commits_typed(ctx.handle, self.kind, self.mode, self.cid, len(self.cid), self.n,
                                                   self.vs_arr, self.kt_arr, self.bid_arr, self.heights, self.cm_arr,
                                                   self.num, self.den, self.res, self.rcs, self.bufs, self.cap)
        else:
            rc = N.lib().cmtv_verify_commits(ctx.handle, self.kind, self.mode, self.cid, len(self.cid), self.n,
                                             self.vs_arr, self.bid_arr, self.heights, self.cm_arr, self.num, self.den,
                                             self.res, self.rcs, self.bufs, self.cap)
        N.check(rc, "cmtv_verify_commits")

    def verify(self, ctx: Context):
        self.call(ctx)
        raw, cap = self.bufs.raw, self.cap
        out = []
        for c in range(self.n):
            msg = raw[c * cap: (c + 1) * cap].split(b"\0", 1)[0].decode()
            out.append(_error_for(self.rcs[c], self.res[c], msg))
        return out
