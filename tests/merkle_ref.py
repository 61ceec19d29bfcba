"""Reference for the merkle tests: hashlib, the recursive HashFromByteSlices
and the two leaf encodings, restated from the reference's sources. Nothing
here goes through the library.

  HashFromByteSlices        crypto/merkle/tree.go:9-21, hash.go:14-26
  Validator.Bytes()         types/validator.go:117-133,
                            proto/tendermint/types/validator.pb.go:361-384 (SimpleValidator),
                            proto/tendermint/crypto/keys.pb.go:376-402 (PublicKey),
                            crypto/encoding/codec.go:20-38
  CommitSig.ToProto()       types/block.go, proto/tendermint/types/types.pb.go:1563-1596
"""
import hashlib

GO_ZERO_TIME_SECONDS = -62135596800  # time.Time{}
LAST_VALID_SECOND = 253402300799     # 9999-12-31T23:59:59Z (gogo/protobuf StdTimeMarshal's bound)
FLAG_ABSENT, FLAG_COMMIT, FLAG_NIL = 1, 2, 3
KEY_ED25519, KEY_SECP256K1, KEY_SR25519 = 0, 1, 2
EMPTY_ROOT = hashlib.sha256(b"").digest()


def sha256(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


def leaf_hash(item: bytes) -> bytes:
    return sha256(b"\x00" + item)


def inner_hash(left: bytes, right: bytes) -> bytes:
    return sha256(b"\x01" + left + right)


def split_point(n: int) -> int:
    """The largest power of two strictly below n (tree.go getSplitPoint)."""
    k = 1
    while k * 2 < n:
        k *= 2
    return k


def root(items) -> bytes:
    n = len(items)
    if n == 0:
        return EMPTY_ROOT
    if n == 1:
        return leaf_hash(items[0])
    k = split_point(n)
    return inner_hash(root(items[:k]), root(items[k:]))


def uvarint(v: int) -> bytes:
    v &= (1 << 64) - 1  # a negative int64 as uint64: ten bytes
    out = bytearray()
    while v >= 0x80:
        out.append(v & 0x7F | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def validator_bytes(key_type: int, key: bytes, power: int) -> bytes:
    tag = {KEY_ED25519: b"\x0a", KEY_SECP256K1: b"\x12"}[key_type]
    pk = tag + uvarint(len(key)) + key
    out = b"\x0a" + uvarint(len(pk)) + pk
    if power != 0:
        out += b"\x10" + uvarint(power)
    return out


def timestamp_bytes(seconds: int, nanos: int) -> bytes:
    out = b""
    if seconds != 0:
        out += b"\x08" + uvarint(seconds)
    if nanos != 0:
        out += b"\x10" + uvarint(nanos)
    return out


def commit_sig_bytes(flag: int, addr, seconds: int, nanos: int, sig: bytes) -> bytes:
    """addr: the address bytes, or None / b"" for no address field."""
    out = b""
    if flag != 0:
        out += b"\x08" + uvarint(flag)
    if addr:
        out += b"\x12" + uvarint(len(addr)) + addr
    t = timestamp_bytes(seconds, nanos)
    out += b"\x1a" + uvarint(len(t)) + t
    if sig:
        out += b"\x22" + uvarint(len(sig)) + sig
    return out


def commit_sig_leaf(flag: int, addr20: bytes, seconds: int, nanos: int, sig: bytes) -> bytes:
    """The struct-of-arrays form's leaf: an Absent signature contributes no
    address field, every other flag its 20 bytes."""
    return commit_sig_bytes(flag, None if flag == FLAG_ABSENT else addr20, seconds, nanos, sig)


def valset_hash(vals) -> bytes:
    """vals: (key_type, key, power) per validator."""
    return root([validator_bytes(*v) for v in vals])


def commit_hash(sigs) -> bytes:
    """sigs: (flag, addr20, seconds, nanos, sig) per signature."""
    return root([commit_sig_leaf(*s) for s in sigs])
