// merkle_internal.h -- what the merkle engine (merkle.cpp) shares with the
// other host files that hash through it (header.cpp): a call's trees as a
// TreeSource, the staging of a run, and the call itself.
#pragma once
#include "runtime_state.h"

namespace cmtv {

// google.protobuf.Timestamp as gogo/protobuf's StdTimeMarshal accepts it
bool merkle_timestamp_ok(int64_t sec, int32_t nanos);
size_t merkle_put_uvarint(uint8_t* p, uint64_t v);
// off[0 .. n] does not decrease
bool merkle_offsets_ok(const uint32_t* off, size_t n);

// Where a run's arrays sit in its staging block (each 16-byte aligned) and,
// while it is packed, the host pointers to them. A kind's arrays are planar
// where it has more than one of a type: array k of the run's n leaves at
// [k n ..).
struct MerkleStage {
  size_t o_pref = 0, o_i64 = 0, o_off = 0, o_i32 = 0, o_u8 = 0, o_addr = 0, o_var = 0, bytes = 0;
  size_t n = 0;  // the run's leaves
  uint32_t* off = nullptr;
  int64_t* i64 = nullptr;
  int32_t* i32 = nullptr;
  uint8_t* u8 = nullptr;
  uint8_t* addr = nullptr;
  uint8_t* var = nullptr;
};

// The trees of one call and leaf kind
struct TreeSource {
  MerkleLeafKind kind;
  size_t n_trees = 0;
  explicit TreeSource(MerkleLeafKind k) : kind(k) {}
  virtual ~TreeSource() = default;
  virtual uint32_t leaves(size_t t) const = 0;
  virtual uint64_t var_bytes(size_t t) const = 0;  // its items, keys, signatures or byte fields
  // tree t's leaves into the staging, from leaf leaf0 and byte var0 of var
  // (the kind's offsets of each of them; the engine writes the run's last offset)
  virtual void pack(size_t t, uint32_t leaf0, uint32_t var0, const MerkleStage& S) const = 0;
};

// Trees of items (kMerkleItems) or of transactions (kMerkleTxs), as
// cmtv_merkle_roots takes them
struct ItemTrees : TreeSource {
  const uint32_t* tree_off;
  const uint8_t* items;
  const uint32_t* item_off;
  ItemTrees(MerkleLeafKind k, size_t n, const uint32_t* to, const uint8_t* it, const uint32_t* io)
      : TreeSource(k), tree_off(to), items(it), item_off(io) {
    n_trees = n;
  }
  uint32_t leaves(size_t t) const override { return tree_off[t + 1] - tree_off[t]; }
  uint64_t var_bytes(size_t t) const override {
    return leaves(t) ? item_off[tree_off[t + 1]] - item_off[tree_off[t]] : 0u;
  }
  void pack(size_t t, uint32_t leaf0, uint32_t var0, const MerkleStage& S) const override;
};

// cmtv_merkle_roots' argument rules (ctx and n_trees apart)
bool merkle_item_trees_ok(size_t n_trees, const uint32_t* tree_off, const uint8_t* items, const uint32_t* item_off,
                          const uint8_t* out);

// A call: the context lock, the first device, the roots into a buffer of the
// call's own and into out only when all of them are there.
int merkle_call(cmtv_ctx* ctx, const TreeSource& S, uint8_t* out);

}  // namespace cmtv
