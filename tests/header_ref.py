"""Reference for the header tests: Header.Hash() and Txs.Hash() restated from
the reference's sources with hashlib, on tests/merkle_ref.py. Nothing here goes
through the library.

  Header.Hash()          types/block.go:440-475
  Version.Marshal()      proto/tendermint/version/types.pb.go:238-254
  cdcEncode              types/encoding_helper.go:11-47 (gogotypes String / Int64 / Bytes values)
  StdTimeMarshal         google.protobuf.Timestamp; merkle_ref.timestamp_bytes
  BlockID.ToProto()      proto/tendermint/types/types.pb.go:1153-1171 (PartSetHeader), 1233-1256 (BlockID)
  Txs.Hash(), Tx.Hash()  types/tx.go:29-31, 47-55
"""
import hashlib
from dataclasses import dataclass, replace

import merkle_ref as R

BYTES_FIELDS = ("last_commit_hash", "data_hash", "validators_hash", "next_validators_hash", "consensus_hash",
                "app_hash", "last_results_hash", "evidence_hash", "proposer_address")


@dataclass(frozen=True)
class Hdr:
    version_block: int = 0
    version_app: int = 0
    chain_id: bytes = b""
    height: int = 0
    seconds: int = 0
    nanos: int = 0
    id_hash: bytes = b""
    id_total: int = 0
    id_part_hash: bytes = b""
    last_commit_hash: bytes = b""
    data_hash: bytes = b""
    validators_hash: bytes = b""
    next_validators_hash: bytes = b""
    consensus_hash: bytes = b""
    app_hash: bytes = b""
    last_results_hash: bytes = b""
    evidence_hash: bytes = b""
    proposer_address: bytes = b""

    def with_(self, **kw):
        return replace(self, **kw)


def tagged_varint(tag: int, v: int) -> bytes:
    return bytes([tag]) + R.uvarint(v) if v != 0 else b""


def tagged_bytes(tag: int, b: bytes) -> bytes:
    return bytes([tag]) + R.uvarint(len(b)) + b if b else b""


def block_id_bytes(id_hash: bytes, total: int, part_hash: bytes) -> bytes:
    psh = tagged_varint(0x08, total) + tagged_bytes(0x12, part_hash)
    return tagged_bytes(0x0A, id_hash) + b"\x12" + R.uvarint(len(psh)) + psh  # the part-set header is not nullable


def time_ok(seconds: int, nanos: int) -> bool:
    return R.GO_ZERO_TIME_SECONDS <= seconds <= R.LAST_VALID_SECOND and 0 <= nanos < 10**9


def leaves(h: Hdr) -> list:
    out = [tagged_varint(0x08, h.version_block) + tagged_varint(0x10, h.version_app),
           tagged_bytes(0x0A, h.chain_id),
           tagged_varint(0x08, h.height),
           R.timestamp_bytes(h.seconds, h.nanos),
           block_id_bytes(h.id_hash, h.id_total, h.id_part_hash)]
    return out + [tagged_bytes(0x0A, getattr(h, f)) for f in BYTES_FIELDS]


def header_hash(h: Hdr):
    """None where the reference returns nil."""
    if not h.validators_hash or not time_ok(h.seconds, h.nanos):
        return None
    return R.root(leaves(h))


def tx_leaf(tx: bytes) -> bytes:
    return R.leaf_hash(hashlib.sha256(tx).digest())


def txs_hash(txs) -> bytes:
    return R.root([hashlib.sha256(tx).digest() for tx in txs])


def kat_header() -> Hdr:
    """types/block_test.go:305-326 TestHeaderHash's header."""
    s = lambda b: hashlib.sha256(b).digest()  # noqa: E731 (tmhash.Sum)
    return Hdr(version_block=1, version_app=2, chain_id=b"chainId", height=3, seconds=1570983284, nanos=0,
               id_hash=bytes(32), id_total=6, id_part_hash=bytes(32), last_commit_hash=s(b"last_commit_hash"),
               data_hash=s(b"data_hash"), validators_hash=s(b"validators_hash"),
               next_validators_hash=s(b"next_validators_hash"), consensus_hash=s(b"consensus_hash"),
               app_hash=s(b"app_hash"), last_results_hash=s(b"last_results_hash"),
               evidence_hash=s(b"evidence_hash"), proposer_address=s(b"proposer_address")[:20])
