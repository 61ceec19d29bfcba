// header.cpp -- the host layer of Header.Hash() (header.h, header.hip): the C
// ABI's cmtv_header_hash[es] and cmtv_header_leaf_bytes. The headers of a call
// go through the merkle engine (merkle_internal.h) as one more leaf kind: a
// run stages the headers' fields, never an encoded leaf, and one launch turns
// them into roots. A header with a field too long for the device builders has
// its fourteen leaves encoded here and is hashed as a tree of items; a header
// for which the reference returns nil costs no device work.
#include "merkle_internal.h"
// (after hip_runtime.h, which defines CMTV_HD's attributes for a host compile)
#include "header.h"

namespace cmtv {
namespace {

// a NULL pointer with a length
bool header_args_ok(const cmtv_header& h) {
  if (!h.chain_id && h.chain_id_len) return false;
  if (!h.last_block_id.hash && h.last_block_id.hash_len) return false;
  if (!h.last_block_id.psh_hash && h.last_block_id.psh_hash_len) return false;
  for (int f = 0; f < CMTV_HDR_N_BYTES_FIELDS; f++)
    if (!h.field[f] && h.field_len[f]) return false;
  return true;
}

// types/block.go:441 (a nil header apart): no ValidatorsHash, or a time that
// StdTimeMarshal refuses, and Hash() is nil
bool header_has_hash(const cmtv_header& h) {
  return h.field_len[CMTV_HDR_VALIDATORS_HASH] != 0 && merkle_timestamp_ok(h.time_seconds, h.time_nanos);
}

// every leaf fits the register builders (two SHA-256 blocks)
bool header_device_form(const cmtv_header& h) {
  if (h.chain_id_len > kHeaderFieldMax) return false;
  if (h.last_block_id.hash_len > kHeaderIdHashMax || h.last_block_id.psh_hash_len > kHeaderIdHashMax) return false;
  for (int f = 0; f < CMTV_HDR_N_BYTES_FIELDS; f++)
    if (h.field_len[f] > kHeaderFieldMax) return false;
  return true;
}

void put_tagged_varint(std::vector<uint8_t>& out, uint8_t tag, uint64_t v) {
  if (v == 0) return;
  uint8_t b[11];
  b[0] = tag;
  const size_t n = 1 + merkle_put_uvarint(b + 1, v);
  out.insert(out.end(), b, b + n);
}

void put_tagged_bytes(std::vector<uint8_t>& out, uint8_t tag, const void* p, uint32_t len) {
  if (len == 0) return;
  uint8_t b[6];
  b[0] = tag;
  const size_t n = 1 + merkle_put_uvarint(b + 1, len);
  out.insert(out.end(), b, b + n);
  const auto* q = static_cast<const uint8_t*>(p);
  out.insert(out.end(), q, q + len);
}

// leaf 0..13 as Header.Hash() encodes it (header.h lists them), appended to out
void encode_header_leaf(std::vector<uint8_t>& out, const cmtv_header& h, uint32_t leaf) {
  switch (leaf) {
    case 0:
      put_tagged_varint(out, 0x08, h.version_block);
      put_tagged_varint(out, 0x10, h.version_app);
      break;
    case 1:
      put_tagged_bytes(out, 0x0a, h.chain_id, h.chain_id_len);
      break;
    case 2:
      put_tagged_varint(out, 0x08, (uint64_t)h.height);
      break;
    case 3:
      put_tagged_varint(out, 0x08, (uint64_t)h.time_seconds);
      put_tagged_varint(out, 0x10, (uint64_t)(int64_t)h.time_nanos);
      break;
    case 4: {
      const cmtv_block_id& id = h.last_block_id;
      put_tagged_bytes(out, 0x0a, id.hash, id.hash_len);
      std::vector<uint8_t> p;
      put_tagged_varint(p, 0x08, id.psh_total);
      put_tagged_bytes(p, 0x12, id.psh_hash, id.psh_hash_len);
      uint8_t b[6];
      b[0] = 0x12;
      const size_t n = 1 + merkle_put_uvarint(b + 1, p.size());
      out.insert(out.end(), b, b + n);
      out.insert(out.end(), p.begin(), p.end());
      break;
    }
    default:
      put_tagged_bytes(out, 0x0a, h.field[leaf - 5], h.field_len[leaf - 5]);
  }
}

// The device-form headers of a call: a tree is a header and has one "leaf",
// the header itself (kernels.h launch_header_hash names the arrays)
struct HeaderTrees : TreeSource {
  std::vector<const cmtv_header*> hs;
  HeaderTrees() : TreeSource(kMerkleHeaders) {}
  uint32_t leaves(size_t) const override { return 1; }
  uint64_t var_bytes(size_t t) const override {
    const cmtv_header& h = *hs[t];
    uint64_t n = (uint64_t)h.chain_id_len + h.last_block_id.hash_len + h.last_block_id.psh_hash_len;
    for (int f = 0; f < CMTV_HDR_N_BYTES_FIELDS; f++) n += h.field_len[f];
    return n;
  }
  void pack(size_t t, uint32_t leaf0, uint32_t var0, const MerkleStage& S) const override {
    const cmtv_header& h = *hs[t];
    uint32_t* off = S.off + kHeaderVarFields * (size_t)leaf0;
    uint32_t at = var0;
    auto put = [&](uint32_t f, const void* p, uint32_t len) {
      off[f] = at;
      if (len) std::memcpy(S.var + at, p, len);
      at += len;
    };
    put(kHeaderVarChainId, h.chain_id, h.chain_id_len);
    put(kHeaderVarIdHash, h.last_block_id.hash, h.last_block_id.hash_len);
    put(kHeaderVarIdPartHash, h.last_block_id.psh_hash, h.last_block_id.psh_hash_len);
    for (uint32_t f = 0; f < CMTV_HDR_N_BYTES_FIELDS; f++) put(kHeaderVarBytes0 + f, h.field[f], h.field_len[f]);
    S.i64[kHeaderVersionBlock * S.n + leaf0] = (int64_t)h.version_block;
    S.i64[kHeaderVersionApp * S.n + leaf0] = (int64_t)h.version_app;
    S.i64[kHeaderHeight * S.n + leaf0] = h.height;
    S.i64[kHeaderSeconds * S.n + leaf0] = h.time_seconds;
    S.i32[kHeaderNanos * S.n + leaf0] = h.time_nanos;
    S.i32[kHeaderIdTotal * S.n + leaf0] = (int32_t)h.last_block_id.psh_total;
  }
};
static_assert(kHeaderVarFields == 3 + CMTV_HDR_N_BYTES_FIELDS, "the staged byte fields");

}  // namespace
}  // namespace cmtv

using namespace cmtv;

extern "C" {

int cmtv_header_hashes(cmtv_ctx* ctx, size_t n, const cmtv_header* hs, uint8_t* out, uint8_t* has_hash) {
  if (!ctx || n > (1ull << 31)) return CMTV_EINVAL;
  if (n == 0) return CMTV_OK;
  if (!hs || !out) return CMTV_EINVAL;
  // headers that take the device builders, headers encoded here, and headers without a hash
  HeaderTrees dev;
  std::vector<size_t> dev_at, wide_at;
  std::vector<uint8_t> has(n, 0);
  for (size_t t = 0; t < n; t++) {
    if (!header_args_ok(hs[t])) return CMTV_EINVAL;
    if (!header_has_hash(hs[t])) {
      if (!has_hash) return CMTV_EINVAL;
      continue;
    }
    has[t] = 1;
    if (header_device_form(hs[t])) {
      dev_at.push_back(t);
      dev.hs.push_back(&hs[t]);
    } else {
      wide_at.push_back(t);
    }
  }
  dev.n_trees = dev.hs.size();
  std::vector<uint8_t> roots(32 * n, 0), part(32 * std::max(dev_at.size(), wide_at.size()));
  int rc;
  if (!dev_at.empty()) {
    if ((rc = merkle_call(ctx, dev, part.data())) != CMTV_OK) return rc;
    for (size_t k = 0; k < dev_at.size(); k++) std::memcpy(&roots[32 * dev_at[k]], &part[32 * k], 32);
  }
  if (!wide_at.empty()) {
    std::vector<uint8_t> items;
    std::vector<uint32_t> item_off(1, 0u), tree_off(1, 0u);
    for (size_t t : wide_at) {
      for (uint32_t leaf = 0; leaf < kHeaderLeaves; leaf++) {
        encode_header_leaf(items, hs[t], leaf);
        if (items.size() > 0xFFFFFFF0ull) return CMTV_EINVAL;
        item_off.push_back((uint32_t)items.size());
      }
      tree_off.push_back((uint32_t)(item_off.size() - 1));
    }
    rc = merkle_call(ctx, ItemTrees(kMerkleItems, wide_at.size(), tree_off.data(), items.data(), item_off.data()),
                     part.data());
    if (rc != CMTV_OK) return rc;
    for (size_t k = 0; k < wide_at.size(); k++) std::memcpy(&roots[32 * wide_at[k]], &part[32 * k], 32);
  }
  std::memcpy(out, roots.data(), roots.size());
  if (has_hash) std::memcpy(has_hash, has.data(), n);
  return CMTV_OK;
}

int cmtv_header_hash(cmtv_ctx* ctx, const cmtv_header* h, uint8_t out[32], uint8_t* has_hash) {
  return cmtv_header_hashes(ctx, 1, h, out, has_hash);
}

int64_t cmtv_header_leaf_bytes(const cmtv_header* h, uint32_t leaf, uint8_t* out, size_t cap) {
  if (!h || leaf >= kHeaderLeaves || (!out && cap) || !header_args_ok(*h)) return CMTV_EINVAL;
  if (leaf == 3 && !merkle_timestamp_ok(h->time_seconds, h->time_nanos)) return CMTV_EINVAL;
  std::vector<uint8_t> b;
  encode_header_leaf(b, *h, leaf);
  if (b.size() <= cap && !b.empty()) std::memcpy(out, b.data(), b.size());
  return (int64_t)b.size();
}

}  // extern "C"
