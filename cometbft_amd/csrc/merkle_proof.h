// merkle_proof.h -- merkle inclusion proofs (crypto/merkle/proof.go): the
// lane code of the proof-building passes and of Proof.Verify, for gfx950 and
// the host checker (tests/host/merkleproofcheck.cpp compiles this file with
// CMTV_HD = inline).
//
// In merkle.h's level form (node j of level l covers leaves [j 2^l,
// min((j + 1) 2^l, n)), an unpaired last node promoted) leaf i's aunts are,
// for l = 0, 1, ... while level l has more than one node, node (i >> l) ^ 1 of
// level l whenever that index is below the level's node count: a promoted
// node contributes none. The count is a function of (n, i) alone
// (merkle_proof_len), at most 63 for an int64 total, and it splits over the
// passes: a leaf's first merkle_proof_len(m, i mod B) aunts are nodes of its
// own aligned block of m leaves, the others are the aunts of its block node
// in the tree of block nodes.
//
// computeHashFromAunts (proof.go:166) is recursive from the root. Here the
// lane walks down from (index, total) first, splitting at the largest power
// of two below total and keeping left / right in a 64-bit mask, then hashes
// upward from the leaf with aunt 0 first and the directions in reverse.
#pragma once
#include "merkle.h"

namespace cmtv {

// include/cmtverify.h CMTV_PROOF_*, in Proof.Verify's own order of checks
constexpr uint32_t kProofOk = 0, kProofNegTotal = 1, kProofNegIndex = 2, kProofLeaf = 3, kProofIndex = 4,
                   kProofExtra = 5, kProofMissing = 6, kProofRoot = 7;
constexpr uint32_t kProofLeafItem = 0, kProofLeafTx = 1;
// a tree of 2^63 - 1 leaves is 63 levels deep: no int64 total takes more aunts
constexpr uint32_t kProofMaxAunts = 63;

// aunts of leaf i in a tree of n leaves, n >= 1 and i < n
template <class U>
CMTV_HD uint32_t merkle_proof_len(U n, U i) {
  uint32_t k = 0;
  for (uint32_t l = 0; l < 8 * sizeof(U); l++) {
    const U c = ((n - 1) >> l) + 1;  // level l's nodes
    if (c <= 1) break;
    k += ((i >> l) ^ 1) < c ? 1u : 0u;
  }
  return k;
}

struct alignas(16) MerkleQuad {
  uint32_t x, y, z, w;
};

// a node's eight digest words to / from 16-byte aligned memory, two 16-byte accesses
CMTV_HD void merkle_store_node(uint32_t* dst, const uint32_t h[8]) {
  MerkleQuad* q = reinterpret_cast<MerkleQuad*>(dst);
  q[0] = MerkleQuad{h[0], h[1], h[2], h[3]};
  q[1] = MerkleQuad{h[4], h[5], h[6], h[7]};
}

CMTV_HD void merkle_load_node(uint32_t h[8], const uint32_t* src) {
  const MerkleQuad* q = reinterpret_cast<const MerkleQuad*>(src);
  const MerkleQuad a = q[0], b = q[1];
  h[0] = a.x; h[1] = a.y; h[2] = a.z; h[3] = a.w;
  h[4] = b.x; h[5] = b.y; h[6] = b.z; h[7] = b.w;
}

// 32 hash bytes at a 16-byte aligned address as digest words
CMTV_HD void merkle_load_hash(uint32_t h[8], const uint8_t* p) {
  merkle_load_node(h, reinterpret_cast<const uint32_t*>(p));
#pragma unroll
  for (int k = 0; k < 8; k++) h[k] = __builtin_bswap32(h[k]);
}

// The lane's aunt at level l of its block: its sibling there among the c nodes
// of src (word-planar, merkle_level_lane's layout), when it has one
CMTV_HD bool merkle_aunt_lane(uint32_t lane, uint32_t l, uint32_t c, const uint32_t* src, uint32_t a[8]) {
  const uint32_t s = (lane >> l) ^ 1u;
  if (s >= c) return false;
#pragma unroll
  for (int k = 0; k < 8; k++) a[k] = src[k * kMerkleB + s];
  return true;
}

// ---------------------------------------------------------------- spreading
// A tree of more than kMerkleB leaves: pass p >= 1 wrote the aunts of its
// leaves (pass p - 1's block nodes) once per node into `up`; they belong to
// every leaf below the node. One lane per leaf appends them to its proof.
constexpr uint32_t kProofMaxPasses = 5;  // kMerkleB >= 64: 2^32 leaves reduce in at most 6 passes, 5 above the first

struct ProofSpread {
  const uint32_t* pref;      // n_pass arrays of n_trees + 1: pass p's leaves' prefix sums
  const uint32_t* aunt_off;  // per leaf of pass 0, in nodes of `aunts`
  const uint32_t* up_off;    // per leaf of the passes >= 1, concatenated, in nodes of `up`
  const uint32_t* up;
  uint32_t* aunts;
  uint32_t n_trees, n_pass, n_leaves;
  uint32_t up_base[kProofMaxPasses + 1];  // where pass p's leaves start in up_off
};

CMTV_HD void merkle_proof_spread_lane(const ProofSpread& S, uint32_t g) {
  uint32_t lo = 0, hi = S.n_trees;  // pref[0][lo] <= g < pref[0][hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (S.pref[mid] <= g)
      lo = mid;
    else
      hi = mid;
  }
  const uint32_t n = S.pref[lo + 1] - S.pref[lo];
  if (n <= kMerkleB) return;  // its proofs are whole after the first pass
  uint32_t j = g - S.pref[lo];
  const uint32_t left0 = n - (j & ~(kMerkleB - 1));
  uint32_t* dst = S.aunts + 8 * ((size_t)S.aunt_off[g] +
                                 merkle_proof_len<uint32_t>(left0 < kMerkleB ? left0 : kMerkleB, j & (kMerkleB - 1)));
  for (uint32_t p = 1; p < S.n_pass; p++) {
    const uint32_t* pf = S.pref + (size_t)(S.n_trees + 1) * p;
    const uint32_t np = pf[lo + 1] - pf[lo];
    j /= kMerkleB;
    const uint32_t left = np - (j & ~(kMerkleB - 1));
    const uint32_t cnt = merkle_proof_len<uint32_t>(left < kMerkleB ? left : kMerkleB, j & (kMerkleB - 1));
    const uint32_t* src = S.up + 8 * (size_t)S.up_off[S.up_base[p] + pf[lo] + j];
    for (uint32_t k = 0; k < cnt; k++) {
      uint32_t h[8];
      merkle_load_node(h, src + 8 * k);
      merkle_store_node(dst, h);
      dst += 8;
    }
  }
}

// ---------------------------------------------------------------- verifying
// The walk down from (index, total) with k aunts: kProofOk and the directions
// (bit d set: the node at depth d below the root is a right child; the depth
// is k), or the error computeHashFromAunts reports first.
CMTV_HD uint32_t merkle_proof_walk(int64_t total, int64_t index, uint32_t k, uint64_t* mask) {
  *mask = 0;
  if (index >= total || index < 0 || total <= 0) return kProofIndex;
  if (k > kProofMaxAunts) return kProofExtra;  // no tree is that deep
  uint64_t t = (uint64_t)total, i = (uint64_t)index, m = 0;
  uint32_t d = 0;
  while (t > 1) {
    if (k == 0) return kProofMissing;
    const uint64_t sp = 1ull << (63 - __builtin_clzll(t - 1));  // getSplitPoint
    if (i < sp) {
      t = sp;
    } else {
      i -= sp;
      t -= sp;
      m |= 1ull << d;
    }
    d++;
    k--;
  }
  if (k != 0) return kProofExtra;
  *mask = m;
  return kProofOk;
}

// A batch of proofs as the verify kernel reads it. Hashes are bytes at
// 16-byte aligned addresses (the aunts' staging 32-byte aligned).
struct ProofBatch {
  const int64_t* total;
  const int64_t* index;
  const uint8_t* leaf_hash;  // n x 32
  const uint32_t* aunt_at;   // proof i's aunts start at aunts + 32 aunt_at[i] ...
  const uint32_t* aunt_cnt;  // ... and are this many (above kProofMaxAunts: none is staged)
  const uint8_t* aunts;
  const uint8_t* roots;      // null: no root check
  const uint32_t* root_idx;  // proof i is checked against root root_idx[i]
  const uint8_t* leaves;     // leaf i = leaves[leaf_off[i] .. leaf_off[i + 1]) ...
  const uint32_t* leaf_off;  // ... null: no leaf check (ComputeRootHash)
  uint32_t leaf_kind;        // kProofLeafItem, or kProofLeafTx: the leaf is SHA-256(tx)
  uint8_t* status;           // n bytes
  uint32_t* out_hash;        // n x 8 digest words: the computed leaf hash on kProofLeaf,
                             // the computed root on kProofOk and kProofRoot, zeros otherwise
};

CMTV_HD bool merkle_node_eq(const uint32_t a[8], const uint32_t b[8]) {
  uint32_t d = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) d |= a[k] ^ b[k];
  return d == 0;
}

// Proof.Verify (proof.go:52) of proof i
CMTV_HD void merkle_proof_verify_lane(const ProofBatch& P, uint32_t i) {
  uint32_t out[8], h[8];
#pragma unroll
  for (int k = 0; k < 8; k++) out[k] = 0u;
  const int64_t total = P.total[i], index = P.index[i];
  uint32_t st = total < 0 ? kProofNegTotal : (index < 0 ? kProofNegIndex : kProofOk);
  merkle_load_hash(h, P.leaf_hash + 32 * (size_t)i);
  if (st == kProofOk && P.leaf_off) {
    const uint32_t o = P.leaf_off[i], len = P.leaf_off[i + 1] - o;
    uint32_t lh[8];
    if (P.leaf_kind == kProofLeafTx)
      merkle_tx_leaf_hash(lh, P.leaves + o, len);
    else
      merkle_leaf_hash(lh, P.leaves + o, len);
    if (!merkle_node_eq(lh, h)) {
      st = kProofLeaf;
#pragma unroll
      for (int k = 0; k < 8; k++) out[k] = lh[k];
    }
  }
  if (st == kProofOk) {
    const uint32_t cnt = P.aunt_cnt[i];
    uint64_t mask;
    st = merkle_proof_walk(total, index, cnt, &mask);
    if (st == kProofOk) {
      const uint8_t* a = P.aunts + 32 * (size_t)P.aunt_at[i];
      for (uint32_t j = 0; j < cnt; j++) {
        uint32_t au[8], n[16];
        merkle_load_hash(au, a + 32 * (size_t)j);
        const bool right = ((mask >> (cnt - 1 - j)) & 1) != 0;  // this node is the right child
#pragma unroll
        for (int k = 0; k < 8; k++) {
          n[k] = right ? au[k] : h[k];
          n[8 + k] = right ? h[k] : au[k];
        }
        merkle_inner_hash(h, n);
      }
#pragma unroll
      for (int k = 0; k < 8; k++) out[k] = h[k];
      if (P.roots) {
        uint32_t r[8];
        merkle_load_hash(r, P.roots + 32 * (size_t)P.root_idx[i]);
        if (!merkle_node_eq(r, h)) st = kProofRoot;
      }
    }
  }
  P.status[i] = (uint8_t)st;
  merkle_store_node(P.out_hash + 8 * (size_t)i, out);
}

}  // namespace cmtv
