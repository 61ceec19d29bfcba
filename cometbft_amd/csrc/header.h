// header.h -- Header.Hash() (types/block.go:440-475) for many headers: the
// fourteen leaves built in registers and the in-wave reduction of one header's
// tree, for gfx950 (header.hip) and the host checker
// (tests/host/headercheck.cpp compiles this file with CMTV_HD = inline).
//
// The root is RFC 6962 (merkle.h) over 14 items in struct order:
//    0  Version.Marshal()        [0x08 uvarint(block)] [0x10 uvarint(app)]
//    1  cdcEncode(ChainID)       0x0a uvarint(len) bytes, or the empty item
//    2  cdcEncode(Height)        [0x08 uvarint(height)]
//    3  StdTimeMarshal(Time)     [0x08 uvarint(seconds)] [0x10 uvarint(nanos)]
//    4  LastBlockID              [0x0a len hash] 0x12 len(P) P,
//                                P = [0x08 uvarint(total)] [0x12 len hash]
//    5..13 cdcEncode(HexBytes)   as leaf 1
// (a bracketed part is left out when its value is zero or empty;
// proto/tendermint/version/types.pb.go:238-254, types/encoding_helper.go:11-47,
// proto/tendermint/types/types.pb.go:1153-1171, 1233-1256). So three builders:
// "bytes" (ten leaves), "two tagged varints" (leaves 0, 2, 3) and "block id".
// Each writes 0x00 || item as a padded message of one or two blocks, in the
// style of merkle.h: every array index static, a piece whose position depends
// on the lane moved into place by msg_place.
//
// A header is owned by kHeaderGroup = 16 lanes, one DPP row: lanes 0..13 hash
// one leaf each, and four levels (14 -> 7 -> 4 -> 2 -> 1) reduce in place at
// stride 2^l, a lane reading its right neighbour's node through the group
// policy's row move. The lane whose right neighbour does not exist keeps its
// node. No LDS, no barrier; lane 0 ends with the root.
#pragma once
#include <stdint.h>

#include "merkle.h"

// headers per workgroup of k_header_hash: 256 threads, 16 lanes a header
#define CMTV_HEADERS_PER_WG 16

namespace cmtv {

constexpr uint32_t kHeaderLeaves = 14;
constexpr uint32_t kHeaderGroup = 16;       // lanes per header: one DPP row
constexpr uint32_t kHeadersPerWg = CMTV_HEADERS_PER_WG;
constexpr uint32_t kHeaderFieldMax = 64;    // chain id and the nine byte fields
constexpr uint32_t kHeaderIdHashMax = 32;   // the two hashes of LastBlockID
// the byte fields as staged, twelve per header: offsets off[12 h + f]
constexpr uint32_t kHeaderVarFields = 12;
constexpr uint32_t kHeaderVarChainId = 0, kHeaderVarIdHash = 1, kHeaderVarIdPartHash = 2, kHeaderVarBytes0 = 3;
// the 64-bit fields, planar: u64[k n + h]
constexpr uint32_t kHeaderU64Fields = 4;
constexpr uint32_t kHeaderVersionBlock = 0, kHeaderVersionApp = 1, kHeaderHeight = 2, kHeaderSeconds = 3;
// the 32-bit ones
constexpr uint32_t kHeaderU32Fields = 2;
constexpr uint32_t kHeaderNanos = 0, kHeaderIdTotal = 1;

// 0x00 || [0x0a len bytes] of a field of at most 64 bytes. fw: its bytes as
// big-endian words, zero past len. Returns the block count: two from 53 bytes.
CMTV_HD uint32_t header_bytes_leaf(uint32_t w[32], const uint32_t fw[16], uint32_t len) {
#pragma unroll
  for (int k = 0; k < 32; k++) w[k] = 0u;
  if (len == 0) {
    w[0] = 0x00800000u;
    return msg_finish(w, 1);
  }
  w[0] = 0x000a0000u | (len << 8) | (fw[0] >> 24);
#pragma unroll
  for (int k = 1; k < 17; k++) w[k] = funnel_bytes(fw[k - 1], k < 16 ? fw[k] : 0u, 3);
  const uint32_t pad[1] = {0x80000000u};
  msg_place<1>(w, pad, 3 + len);
  return msg_finish(w, 3 + len);
}

// 0x00 || [0x08 uvarint(a) when a != 0] [0x10 uvarint(b) when b != 0]: at most
// 23 bytes, one block
CMTV_HD uint32_t header_varints_leaf(uint32_t w[32], uint64_t a, uint64_t b) {
  MsgBytes<6> m;
  m.clear();
  m.put(0x00);
  if (a != 0) {
    m.put(0x08);
    m.put_uvarint(a);
  }
  if (b != 0) {
    m.put(0x10);
    m.put_uvarint(b);
  }
  const uint32_t len = m.n;
  m.put(0x80);
#pragma unroll
  for (int k = 0; k < 32; k++) w[k] = k < 6 ? m.c[k] : 0u;
  return msg_finish(w, len);
}

// one of a block id's hashes as a tagged field, tag len bytes, at position 0
CMTV_HD void header_tagged_hash(uint32_t p[9], uint32_t tag, const uint32_t hw[8], uint32_t len) {
  p[0] = (tag << 24) | (len << 16) | (hw[0] >> 16);
#pragma unroll
  for (int k = 1; k < 9; k++) p[k] = (hw[k - 1] << 16) | (k < 8 ? hw[k] >> 16 : 0u);
}

// 0x00 || BlockID.ToProto().Marshal(); both hashes at most 32 bytes, as
// big-endian words, zero past their lengths. At most 77 bytes.
CMTV_HD uint32_t header_block_id_leaf(uint32_t w[32], const uint32_t hw[8], uint32_t hlen, uint32_t total,
                                      const uint32_t pw[8], uint32_t plen) {
#pragma unroll
  for (int k = 0; k < 32; k++) w[k] = 0u;
  uint32_t pos = 1;
  uint32_t p[9];
  if (hlen != 0) {
    header_tagged_hash(p, 0x0a, hw, hlen);
    msg_place<9>(w, p, pos);
    pos += 2 + hlen;
  }
  {
    MsgBytes<2> m;
    m.clear();
    m.put(0x12);
    m.put((total ? 1 + merkle_uvlen(total) : 0u) + (plen ? 2 + plen : 0u));
    if (total != 0) {
      m.put(0x08);
      m.put_uvarint(total);
    }
    msg_place<2>(w, m.c, pos);
    pos += m.n;
  }
  if (plen != 0) {
    header_tagged_hash(p, 0x12, pw, plen);
    msg_place<9>(w, p, pos);
    pos += 2 + plen;
  }
  const uint32_t pad[1] = {0x80000000u};
  msg_place<1>(w, pad, pos);
  return msg_finish(w, pos);
}

// A header's fields as a run stages them (kernels.h MerkleLeaves: var, off,
// i64 and i32 hold the arrays named above), n headers
struct HeaderFields {
  const uint8_t* var;
  const uint32_t* off;
  const uint64_t* u64;
  const uint32_t* u32;
  uint32_t n;
};

// leaf `leaf` (0..13) of header h as a padded message; returns the block count
CMTV_HD uint32_t header_leaf(uint32_t w[32], const HeaderFields& F, uint32_t h, uint32_t leaf) {
  const uint32_t* off = F.off + kHeaderVarFields * (size_t)h;
  if (leaf == 0 || leaf == 2 || leaf == 3) {
    const uint32_t ka = leaf == 0 ? kHeaderVersionBlock : leaf == 2 ? kHeaderHeight : kHeaderSeconds;
    const uint64_t a = F.u64[ka * (size_t)F.n + h];
    uint64_t b = 0;
    if (leaf == 0) b = F.u64[kHeaderVersionApp * (size_t)F.n + h];
    if (leaf == 3) b = F.u32[kHeaderNanos * (size_t)F.n + h];
    return header_varints_leaf(w, a, b);
  }
  if (leaf == 4) {
    uint32_t hw[8], pw[8];
    const uint32_t o0 = off[kHeaderVarIdHash], o1 = off[kHeaderVarIdPartHash], o2 = off[kHeaderVarIdPartHash + 1];
    load_be_words<8>(hw, F.var + o0, o1 - o0);
    load_be_words<8>(pw, F.var + o1, o2 - o1);
    return header_block_id_leaf(w, hw, o1 - o0, F.u32[kHeaderIdTotal * (size_t)F.n + h], pw, o2 - o1);
  }
  const uint32_t f = leaf == 1 ? kHeaderVarChainId : kHeaderVarBytes0 + (leaf - 5);
  const uint32_t o = off[f], len = off[f + 1] - o;
  uint32_t fw[16];
  load_be_words<16>(fw, F.var + o, len);
  return header_bytes_leaf(w, fw, len);
}

// One level of a group's reduction: the c nodes held at stride S (by the lanes
// whose index in the group is a multiple of S) become (c + 1) / 2 at stride
// 2 S. G::down<S>(out, in): every lane's `in`, eight words, as held by the
// lane S above it in the same row of 16 (DevGroup: DPP row_shl; the host
// checker's policy reads a snapshot of the wave). Every lane hashes, so the
// compressions are uniform across the wave; only a left child with a right
// neighbour keeps the result.
template <int S, class G>
CMTV_HD void header_level(const G& g, uint32_t lane, uint32_t c, uint32_t h[8]) {
  uint32_t n[16], r[8];
#pragma unroll
  for (int k = 0; k < 8; k++) n[k] = h[k];
  g.template down<S>(n + 8, h);
  merkle_inner_hash(r, n);
  const bool pair = (lane & (2 * S - 1)) == 0 && lane / S + 1 < c;
#pragma unroll
  for (int k = 0; k < 8; k++) h[k] = pair ? r[k] : h[k];
}

// 14 -> 7 -> 4 -> 2 -> 1: lane 0 of the group ends with the root. (The host
// checker runs the same four levels, each over a whole wave at a time.)
template <class G>
CMTV_HD void header_reduce(const G& g, uint32_t lane, uint32_t h[8]) {
  header_level<1>(g, lane, 14, h);
  header_level<2>(g, lane, 7, h);
  header_level<4>(g, lane, 4, h);
  header_level<8>(g, lane, 2, h);
}

}  // namespace cmtv
