"""Shared by the header tests: seeded headers in tests/header_ref.py's form, and
that form packed into the C struct."""
import ctypes

import numpy as np

import header_ref as H
from cometbft_amd import _native as N

U64 = (1 << 64) - 1
_p8 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))  # noqa: E731


def gen_header(rng, **kw):
    """A header as a chain produces them (32-byte hashes, a 20-byte address, a
    16-character chain id), fields random; kw replaces fields."""
    h = H.Hdr(version_block=11, version_app=rng.randrange(3), chain_id=b"test-chain-%05d" % rng.randrange(10**5),
              height=rng.randrange(1, 2**40), seconds=1_700_000_000 + rng.randrange(10**7), nanos=rng.randrange(10**9),
              id_hash=rng.randbytes(32), id_total=rng.randrange(1, 100), id_part_hash=rng.randbytes(32),
              **{f: rng.randbytes(20 if f == "proposer_address" else 32) for f in H.BYTES_FIELDS})
    return h.with_(**kw)


def as_int64(v):
    """The int64 with v's low 64 bits."""
    return ((v + 2**63) % 2**64) - 2**63


class CHeader:
    """A header_ref.Hdr in the C struct, every byte field `align` bytes into an
    array of its own that ends within four bytes of the field."""

    def __init__(self, h: H.Hdr, align=0):
        self.h, self.keep = h, []

        def put(b):
            a = np.frombuffer(bytes(align) + b + b"\0", np.uint8).copy()
            self.keep.append(a)
            return a.ctypes.data + align

        bid = N.cmtv_block_id(hash=ctypes.cast(put(h.id_hash), N._u8p), hash_len=len(h.id_hash), psh_total=h.id_total,
                              psh_hash=ctypes.cast(put(h.id_part_hash), N._u8p), psh_hash_len=len(h.id_part_hash))
        self.c = N.cmtv_header(version_block=h.version_block & U64, version_app=h.version_app & U64,
                               chain_id=ctypes.c_char_p(put(h.chain_id)), chain_id_len=len(h.chain_id),
                               height=h.height, time_seconds=h.seconds, time_nanos=h.nanos, last_block_id=bid)
        for i, f in enumerate(H.BYTES_FIELDS):
            self.c.field[i] = ctypes.cast(put(getattr(h, f)), N._u8p)
            self.c.field_len[i] = len(getattr(h, f))
