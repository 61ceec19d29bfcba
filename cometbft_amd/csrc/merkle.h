// merkle.h -- RFC 6962 merkle roots (crypto/merkle/tree.go:9 HashFromByteSlices,
// hash.go:14-26) with the leaves of ValidatorSet.Hash() and Commit.Hash()
// built on the device, for gfx950 and the host checkers
// (tests/host/merklecheck.cpp compiles this file with CMTV_HD = inline).
//
//   empty tree   SHA-256("")
//   leaf         SHA-256(0x00 || item)
//   inner node   SHA-256(0x01 || left || right)
//
// The reference splits at the largest power of two below n; reducing level by
// level in pairs and promoting an unpaired last node unchanged gives the same
// root (its own HashFromByteSlicesIterative, tree.go:62): node j of level l
// covers leaves [j 2^l, min((j + 1) 2^l, n)), so an aligned block of
// CMTV_MERKLE_BLOCK_LEAVES leaves reduces to one node on its own.
//
// A message is held as big-endian words in registers, every index static: a
// field whose position depends on the lane (a varint before it) is built at
// position 0 of a small array and moved into place by msg_place, a funnel
// shift plus a five-stage word shifter, never by an indexed store (which
// would put the array in scratch).
#pragma once
#include <stdint.h>

#include "sha256.h"

#define CMTV_MERKLE_BLOCK_LEAVES 256

namespace cmtv {

constexpr uint32_t kMerkleB = CMTV_MERKLE_BLOCK_LEAVES;
static_assert((kMerkleB & (kMerkleB - 1)) == 0 && kMerkleB >= 64, "a power of two of whole waves");

// key types of a validator leaf (include/cmtverify.h CMTV_KEY_*)
constexpr uint32_t kMerkleKeyEd25519 = 0, kMerkleKeySecp256k1 = 1;
constexpr uint32_t kMerkleFlagAbsent = 1;  // types/block.go BlockIDFlagAbsent

CMTV_HD void sha256_init(uint32_t st[8]) {
  st[0] = 0x6a09e667u; st[1] = 0xbb67ae85u; st[2] = 0x3c6ef372u; st[3] = 0xa54ff53au;
  st[4] = 0x510e527fu; st[5] = 0x9b05688cu; st[6] = 0x1f83d9abu; st[7] = 0x5be0cd19u;
}

// SHA-256("") as digest words: the root of an empty tree
CMTV_HD void merkle_empty(uint32_t out[8]) {
  out[0] = 0xe3b0c442u; out[1] = 0x98fc1c14u; out[2] = 0x9afbf4c8u; out[3] = 0x996fb924u;
  out[4] = 0x27ae41e4u; out[5] = 0x649b934cu; out[6] = 0xa495991bu; out[7] = 0x7852b855u;
}

// SHA-256 of a padded message of nb (1 or 2) blocks in w[0 .. 16 nb); w is consumed
CMTV_HD void sha256_blocks(uint32_t out[8], uint32_t w[32], uint32_t nb) {
  sha256_init(out);
  sha256_compress(out, w);
  if (nb > 1) sha256_compress(out, w + 16);
}

// ORs the byte stream of c (N big-endian words) into w at byte position pos.
// The stream's non-zero bytes must end by byte 128.
template <int N>
CMTV_HD void msg_place(uint32_t w[32], const uint32_t c[N], uint32_t pos) {
  const uint32_t sh = pos & 3, q = pos >> 2;
  uint32_t t[32];
#pragma unroll
  for (int k = 0; k < 32; k++) {
    const uint32_t hi = (k >= 1 && k <= N) ? c[k - 1] : 0u;
    const uint32_t lo = k < N ? c[k] : 0u;
    t[k] = k <= N ? funnel_bytes(hi, lo, sh) : 0u;
  }
#pragma unroll
  for (int s = 16; s >= 1; s >>= 1) {
    const bool on = (q & (uint32_t)s) != 0;
#pragma unroll
    for (int k = 31; k >= 0; k--) {
      const uint32_t from = k >= s ? t[k - s] : 0u;
      t[k] = on ? from : t[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 32; k++) w[k] |= t[k];
}

// A field of at most 4 N bytes built byte by byte at position 0
template <int N>
struct MsgBytes {
  uint32_t c[N];
  uint32_t n;
  CMTV_HD void clear() {
#pragma unroll
    for (int k = 0; k < N; k++) c[k] = 0u;
    n = 0;
  }
  CMTV_HD void put(uint32_t b) {
    const uint32_t at = n >> 2, v = (b & 0xffu) << (24 - 8 * (n & 3));
#pragma unroll
    for (int k = 0; k < N; k++) c[k] |= at == (uint32_t)k ? v : 0u;
    n++;
  }
  CMTV_HD void put_uvarint(uint64_t v) {
    while (v >= 0x80) {
      put((uint32_t)(v & 0x7f) | 0x80u);
      v >>= 7;
    }
    put((uint32_t)v);
  }
};

CMTV_HD uint32_t merkle_uvlen(uint64_t v) {
  uint32_t n = 1;
  while (v >= 0x80) {
    v >>= 7;
    n++;
  }
  return n;
}

// The first len (at most 4 NW) bytes at p, any alignment, as big-endian words,
// zero past len: 4-byte aligned loads re-aligned in registers, only words that
// hold one of the bytes (sha256_msg's reads)
template <int NW>
CMTV_HD void load_be_words(uint32_t out[NW], const uint8_t* p, uint32_t len) {
  const uint32_t sh = (uint32_t)((uintptr_t)p & 3);
  const uint32_t* mw = reinterpret_cast<const uint32_t*>(p - sh);
  const uint32_t nwords = len ? (sh + len + 3) / 4 : 0u;
  const uint32_t jmax = nwords ? nwords - 1 : 0u;
  const uint32_t* mb = nwords ? mw : &g_sha512_no_word;
  uint32_t mv[NW + 1];
#pragma unroll
  for (int k = 0; k < NW + 1; k++) mv[k] = mb[(uint32_t)k < nwords ? (uint32_t)k : jmax];
#pragma unroll
  for (int k = 0; k < NW + 1; k++) mv[k] = (uint32_t)k < nwords ? mv[k] : 0u;
#pragma unroll
  for (int t = 0; t < NW; t++) {
    const uint32_t v = funnel_bytes(mv[t + 1], mv[t], sh);
    const int r = (int)len - 4 * t;
    const uint32_t rr = r < 0 ? 0u : (r > 4 ? 4u : (uint32_t)r);
    out[t] = __builtin_bswap32(v & (uint32_t)((1ull << (8 * rr)) - 1u));
  }
}

// the message length (bytes) into the last block's length word; returns the block count
CMTV_HD uint32_t msg_finish(uint32_t w[32], uint32_t len) {
  const uint32_t nb = len + 9 > 64 ? 2u : 1u;
  if (nb == 1)
    w[15] = 8 * len;
  else
    w[31] = 8 * len;
  return nb;
}

// 0x00 || Validator.Bytes() (types/validator.go:117-133, SimpleValidator
// proto/tendermint/types/validator.pb.go:361-384, PublicKey
// proto/tendermint/crypto/keys.pb.go:376-402) as a padded message:
//   0x0a uvarint(len P) P  [0x10 uvarint(power) when power != 0]
//   P = 0x0a (Ed25519) or 0x12 (secp256k1), uvarint(len key), key
// kw: the key's bytes as big-endian words, zero past klen; klen 1..64, so
// both lengths are one byte and the key starts at byte 5. Returns the block
// count (1 or 2).
CMTV_HD uint32_t merkle_validator_leaf(uint32_t w[32], const uint32_t kw[16], uint32_t klen, uint32_t ktype,
                                       int64_t power) {
  const uint32_t tag = ktype == kMerkleKeySecp256k1 ? 0x12u : 0x0au;
  w[0] = 0x000a0000u | ((klen + 2) << 8) | tag;
#pragma unroll
  for (int k = 0; k < 17; k++) {
    const uint32_t prev = k == 0 ? klen : kw[k - 1];
    const uint32_t cur = k < 16 ? kw[k] : 0u;
    w[1 + k] = funnel_bytes(prev, cur, 1);
  }
#pragma unroll
  for (int k = 18; k < 32; k++) w[k] = 0u;
  MsgBytes<3> tail;
  tail.clear();
  if (power != 0) {
    tail.put(0x10);
    tail.put_uvarint((uint64_t)power);
  }
  tail.put(0x80);
  msg_place<3>(w, tail.c, 5 + klen);
  return msg_finish(w, 5 + klen + tail.n - 1);
}

// 0x00 || CommitSig.ToProto().Marshal() (types/block.go CommitSig.ToProto,
// proto/tendermint/types/types.pb.go:1563-1596) as a padded message:
//   [0x08 uvarint(flag) when flag != 0]  [0x12 0x14 address unless Absent]
//   0x1a uvarint(len T) T  [0x22 uvarint(len sig) sig when non-empty]
//   T = [0x08 uvarint(seconds) when != 0] [0x10 uvarint(nanos) when != 0]
// addr: the 20 address bytes as big-endian words; sw: the signature's bytes as
// big-endian words, zero past slen; slen at most 64, nanos in [0, 10^9).
// Returns the block count (1 or 2).
CMTV_HD uint32_t merkle_commit_sig_leaf(uint32_t w[32], uint32_t flag, const uint32_t addr[5], int64_t sec,
                                        int32_t nanos, const uint32_t sw[16], uint32_t slen) {
#pragma unroll
  for (int k = 0; k < 32; k++) w[k] = 0u;
  uint32_t pos = 1;
  if (flag != 0) {
    MsgBytes<1> f;
    f.clear();
    f.put(0x08);
    f.put_uvarint(flag & 0xffu);
    msg_place<1>(w, f.c, pos);
    pos += f.n;
  }
  if (flag != kMerkleFlagAbsent) {
    uint32_t a[6];
    a[0] = 0x12140000u | (addr[0] >> 16);
#pragma unroll
    for (int k = 1; k < 5; k++) a[k] = (addr[k - 1] << 16) | (addr[k] >> 16);
    a[5] = addr[4] << 16;
    msg_place<6>(w, a, pos);
    pos += 22;
  }
  {
    MsgBytes<5> t;
    t.clear();
    uint32_t tl = 0;
    if (sec != 0) tl += 1 + merkle_uvlen((uint64_t)sec);
    if (nanos != 0) tl += 1 + merkle_uvlen((uint64_t)(int64_t)nanos);
    t.put(0x1a);
    t.put(tl);
    if (sec != 0) {
      t.put(0x08);
      t.put_uvarint((uint64_t)sec);
    }
    if (nanos != 0) {
      t.put(0x10);
      t.put_uvarint((uint64_t)(int64_t)nanos);
    }
    msg_place<5>(w, t.c, pos);
    pos += t.n;
  }
  if (slen != 0) {
    uint32_t s[17];
    s[0] = 0x22000000u | (slen << 16) | (sw[0] >> 16);
#pragma unroll
    for (int k = 1; k < 16; k++) s[k] = (sw[k - 1] << 16) | (sw[k] >> 16);
    s[16] = sw[15] << 16;
    msg_place<17>(w, s, pos);
    pos += 2 + slen;
  }
  const uint32_t pad[1] = {0x80000000u};
  msg_place<1>(w, pad, pos);
  return msg_finish(w, pos);
}

// SHA-256(0x00 || item[0 .. len)), the item anywhere in global memory:
// sha256_msg's aligned loads, the stream moved one byte up for the prefix
CMTV_HD void merkle_leaf_hash(uint32_t out[8], const uint8_t* item, uint32_t len) {
  sha256_init(out);
  const uint32_t total = len + 1;
  const uint32_t nblocks = (total + 9 + 63) / 64;
  const uint32_t sh = (uint32_t)((uintptr_t)item & 3);
  const uint32_t* mw = reinterpret_cast<const uint32_t*>(item - sh);
  const uint32_t nwords = len ? (sh + len + 3) / 4 : 0u;
  const uint32_t jmax = nwords ? nwords - 1 : 0u;
  const uint32_t* mb = nwords ? mw : &g_sha512_no_word;
  uint32_t prev = 0;  // the item's little-endian stream word before this block's first
#pragma unroll 1
  for (uint32_t b = 0; b < nblocks; b++) {
    uint32_t mv[17];
#pragma unroll
    for (int k = 0; k < 17; k++) {
      const uint32_t j = b * 16 + k;
      mv[k] = mb[j < nwords ? j : jmax];
    }
#pragma unroll
    for (int k = 0; k < 17; k++) mv[k] = b * 16 + k < nwords ? mv[k] : 0u;
    uint32_t w[16];
#pragma unroll
    for (int t = 0; t < 16; t++) {
      const uint32_t pos = b * 64 + 4 * t;
      const uint32_t cur = funnel_bytes(mv[t + 1], mv[t], sh);  // item bytes 4 (16 b + t) ...
      const uint32_t v = funnel_bytes(cur, prev, 3);            // ... and the hashed stream's, one byte later
      prev = cur;
      const int r = (int)total - (int)pos;
      const uint32_t rr = r < 0 ? 0u : (r > 4 ? 4u : (uint32_t)r);
      const uint32_t keep = (uint32_t)((1ull << (8 * rr)) - 1u);
      const uint32_t pad = (r >= 0 && r < 4) ? (0x80u << (8 * rr)) : 0u;
      // byte 0 of the stream is the 0x00 prefix: prev starts as zero
      w[t] = __builtin_bswap32((v & keep) | pad);
    }
    if (b == nblocks - 1) {
      w[14] = total >> 29;
      w[15] = total << 3;
    }
    sha256_compress(out, w);
  }
}

// The leaf of a transaction in Txs.Hash() (types/tx.go:29-31, 47-55):
// SHA-256(0x00 || SHA-256(tx)), the transaction anywhere in global memory and
// of any length (sha256_msg's block loop), then the 33-byte leaf in one block
CMTV_HD void merkle_tx_leaf_hash(uint32_t out[8], const uint8_t* tx, uint32_t len) {
  uint32_t d[8], w[16];
  sha256_msg(d, tx, len);
  w[0] = d[0] >> 8;
#pragma unroll
  for (int k = 1; k < 8; k++) w[k] = funnel_bytes(d[k - 1], d[k], 1);
  w[8] = (d[7] << 24) | 0x00800000u;
#pragma unroll
  for (int k = 9; k < 15; k++) w[k] = 0u;
  w[15] = 8 * 33;
  sha256_init(out);
  sha256_compress(out, w);
}

// SHA-256(0x01 || left || right), n = the two nodes' sixteen digest words. The
// 65-byte message sits one byte off the words: block 1 is sixteen funnel
// shifts, block 2 the last byte, the padding and the length 520.
CMTV_HD void merkle_inner_hash(uint32_t out[8], const uint32_t n[16]) {
  uint32_t w[16];
  w[0] = funnel_bytes(0x01u, n[0], 1);
#pragma unroll
  for (int k = 1; k < 16; k++) w[k] = funnel_bytes(n[k - 1], n[k], 1);
  sha256_init(out);
  sha256_compress(out, w);
  w[0] = (n[15] << 24) | 0x00800000u;
#pragma unroll
  for (int k = 1; k < 15; k++) w[k] = 0u;
  w[15] = 520u;
  sha256_compress(out, w);
}

// ---------------------------------------------------------------- passes
// A launch reduces every tree's aligned blocks of kMerkleB leaves to one node
// each; the next takes those nodes as leaves, until every tree has one.
// A tree of n leaves has merkle_blocks(n) workgroups (one for an empty tree:
// it writes the constant). wg_off (n_trees + 1 words) is their prefix sum,
// leaf_off (n_trees + 1) the leaves'; workgroup g writes node g, so a pass's
// wg_off is the next one's leaf_off.
CMTV_HD uint32_t merkle_blocks(uint32_t n) { return n <= kMerkleB ? 1u : (n + kMerkleB - 1) / kMerkleB; }

struct MerkleBlock {
  uint32_t first;  // its first leaf
  uint32_t m;      // its leaves, 0 (an empty tree) .. kMerkleB
};

CMTV_HD MerkleBlock merkle_block_of(uint32_t g, const uint32_t* wg_off, const uint32_t* leaf_off, uint32_t n_trees) {
  uint32_t lo = 0, hi = n_trees;  // wg_off[lo] <= g < wg_off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (wg_off[mid] <= g)
      lo = mid;
    else
      hi = mid;
  }
  const uint32_t j = g - wg_off[lo], n = leaf_off[lo + 1] - leaf_off[lo];
  MerkleBlock b;
  b.first = leaf_off[lo] + j * kMerkleB;
  b.m = n - j * kMerkleB < kMerkleB ? n - j * kMerkleB : kMerkleB;
  return b;
}

// A level is stored word-planar, word k of node i at [k * kMerkleB + i]: a
// lane's two children are eight 8-byte reads at unit stride across the wave.
struct alignas(8) MerklePair {
  uint32_t l, r;
};

// One lane's share of one level: the c nodes of src become (c + 1) / 2 in
// dst, the unpaired last one promoted unchanged. src and dst are different
// buffers, so a level costs one barrier.
CMTV_HD void merkle_level_lane(uint32_t lane, uint32_t c, const uint32_t* src, uint32_t* dst) {
  const uint32_t pairs = c >> 1;
  if (lane < pairs) {
    uint32_t n[16], h[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const MerklePair p = *reinterpret_cast<const MerklePair*>(src + k * kMerkleB + 2 * lane);
      n[k] = p.l;
      n[8 + k] = p.r;
    }
    merkle_inner_hash(h, n);
#pragma unroll
    for (int k = 0; k < 8; k++) dst[k * kMerkleB + lane] = h[k];
  } else if (lane == pairs && (c & 1)) {
#pragma unroll
    for (int k = 0; k < 8; k++) dst[k * kMerkleB + lane] = src[k * kMerkleB + c - 1];
  }
}

}  // namespace cmtv
