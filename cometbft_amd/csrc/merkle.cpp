// merkle.cpp -- the host layer of the merkle engine (merkle.h, merkle.hip):
// the C ABI's cmtv_merkle_root[s], cmtv_valset_hash[es], cmtv_commit_hash[es]
// and the two host leaf encoders (header.cpp's calls run through the same
// engine: merkle_internal.h). A call's trees are cut into runs of about
// kRunBytes staged bytes; a run is one pinned staging block (the pass prefix
// arrays and the leaves' struct-of-arrays fields, no encoded leaf), one copy
// to the context's first device, one launch per pass on its stream and the
// run's roots back. Two staging slots: the host packs a run while the device
// hashes the one before.
#include "merkle_internal.h"
// (after hip_runtime.h, which defines CMTV_HD's attributes for a host compile)
#include "header.h"

namespace cmtv {

// google.protobuf.Timestamp as gogo/protobuf's StdTimeMarshal accepts it
// (types/timestamp.go validateTimestamp; that library is not part of the
// reference tree, the bounds are from its public source): seconds from
// 0001-01-01T00:00:00Z up to, not including, 10000-01-01T00:00:00Z
constexpr int64_t kMinSeconds = -62135596800ll, kMaxSeconds = 253402300800ll;

bool merkle_timestamp_ok(int64_t sec, int32_t nanos) {
  return sec >= kMinSeconds && sec < kMaxSeconds && nanos >= 0 && nanos < 1000000000;
}

size_t merkle_put_uvarint(uint8_t* p, uint64_t v) {
  size_t n = 0;
  while (v >= 0x80) {
    p[n++] = (uint8_t)(v | 0x80);
    v >>= 7;
  }
  p[n++] = (uint8_t)v;
  return n;
}

bool merkle_offsets_ok(const uint32_t* off, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (off[i + 1] < off[i]) return false;
  return true;
}

namespace {

// staged bytes of a run (a tree is never split: a larger one is a run of its own)
constexpr uint64_t kRunBytes = 32ull << 20;
constexpr size_t kRunTrees = 1u << 20;

// crypto/encoding/codec.go:20-38 PubKeyToProto knows Ed25519 and secp256k1
// only (an sr25519 key makes Validator.Bytes() panic); no codec
// yields a key of 0 or of more than 64 bytes
bool validator_ok(uint32_t key_type, size_t pk_len) {
  return key_type <= CMTV_KEY_SECP256K1 && pk_len >= 1 && pk_len <= 64;
}

constexpr size_t kValidatorBytesMax = 2 + 2 + 64 + 11;

// Validator.Bytes() (types/validator.go:117-133); validator_ok holds
size_t encode_validator(uint8_t* p, uint32_t key_type, const uint8_t* pk, size_t pk_len, int64_t power) {
  size_t n = 0;
  p[n++] = 0x0a;
  p[n++] = (uint8_t)(pk_len + 2);
  p[n++] = key_type == CMTV_KEY_SECP256K1 ? 0x12 : 0x0a;
  p[n++] = (uint8_t)pk_len;
  std::memcpy(p + n, pk, pk_len);
  n += pk_len;
  if (power != 0) {
    p[n++] = 0x10;
    n += merkle_put_uvarint(p + n, (uint64_t)power);
  }
  return n;
}

// CommitSig.ToProto().Marshal() (proto/tendermint/types/types.pb.go:1563-1596), appended to out
void encode_commit_sig(std::vector<uint8_t>& out, uint32_t flag, const uint8_t* addr20, int64_t sec, int32_t nanos,
                       const uint8_t* sig, size_t sig_len) {
  uint8_t b[64];
  size_t n = 0;
  if (flag != 0) {
    b[n++] = 0x08;
    n += merkle_put_uvarint(b + n, flag);
  }
  if (addr20) {
    b[n++] = 0x12;
    b[n++] = 0x14;
    std::memcpy(b + n, addr20, 20);
    n += 20;
  }
  uint8_t t[20];
  size_t tl = 0;
  if (sec != 0) {
    t[tl++] = 0x08;
    tl += merkle_put_uvarint(t + tl, (uint64_t)sec);
  }
  if (nanos != 0) {
    t[tl++] = 0x10;
    tl += merkle_put_uvarint(t + tl, (uint64_t)(int64_t)nanos);
  }
  b[n++] = 0x1a;
  b[n++] = (uint8_t)tl;
  std::memcpy(b + n, t, tl);
  n += tl;
  if (sig_len) {
    b[n++] = 0x22;
    n += merkle_put_uvarint(b + n, sig_len);
  }
  out.insert(out.end(), b, b + n);
  if (sig_len) out.insert(out.end(), sig, sig + sig_len);
}

void pack_offsets(uint32_t* dst, const uint32_t* src, uint32_t n, uint32_t var0) {
  for (uint32_t i = 0; i < n; i++) dst[i] = var0 + (src[i] - src[0]);
}

struct ValidatorTrees : TreeSource {
  const cmtv_valset* vals;
  const uint8_t* const* key_types;
  ValidatorTrees(size_t n, const cmtv_valset* v, const uint8_t* const* kt)
      : TreeSource(kMerkleValidators), vals(v), key_types(kt) {
    n_trees = n;
  }
  uint32_t leaves(size_t t) const override { return vals[t].n_vals; }
  uint64_t var_bytes(size_t t) const override {
    return vals[t].n_vals ? vals[t].pk_off[vals[t].n_vals] - vals[t].pk_off[0] : 0u;
  }
  void pack(size_t t, uint32_t leaf0, uint32_t var0, const MerkleStage& S) const override {
    const cmtv_valset& v = vals[t];
    const uint32_t n = v.n_vals;
    if (!n) return;
    pack_offsets(S.off + leaf0, v.pk_off, n, var0);
    std::memcpy(S.var + var0, v.pubkeys + v.pk_off[0], v.pk_off[n] - v.pk_off[0]);
    std::memcpy(S.i64 + leaf0, v.voting_power, 8 * (size_t)n);
    const uint8_t* kt = key_types ? key_types[t] : nullptr;
    if (kt)
      std::memcpy(S.u8 + leaf0, kt, n);
    else
      std::memset(S.u8 + leaf0, CMTV_KEY_ED25519, n);
  }
};

struct CommitTrees : TreeSource {
  std::vector<const cmtv_commit*> commits;
  CommitTrees() : TreeSource(kMerkleCommitSigs) {}
  uint32_t leaves(size_t t) const override { return commits[t]->n_sigs; }
  uint64_t var_bytes(size_t t) const override {
    const cmtv_commit& c = *commits[t];
    return c.n_sigs ? c.sig_off[c.n_sigs] - c.sig_off[0] : 0u;
  }
  void pack(size_t t, uint32_t leaf0, uint32_t var0, const MerkleStage& S) const override {
    const cmtv_commit& c = *commits[t];
    const uint32_t n = c.n_sigs;
    if (!n) return;
    pack_offsets(S.off + leaf0, c.sig_off, n, var0);
    if (c.sig_off[n] != c.sig_off[0]) std::memcpy(S.var + var0, c.sigs + c.sig_off[0], c.sig_off[n] - c.sig_off[0]);
    std::memcpy(S.i64 + leaf0, c.ts_seconds, 8 * (size_t)n);
    std::memcpy(S.i32 + leaf0, c.ts_nanos, 4 * (size_t)n);
    std::memcpy(S.u8 + leaf0, c.flags, n);
    if (c.val_addrs)
      std::memcpy(S.addr + 20 * (size_t)leaf0, c.val_addrs, 20 * (size_t)n);
    else  // every signature is absent: the addresses are not read into a leaf
      std::memset(S.addr + 20 * (size_t)leaf0, 0, 20 * (size_t)n);
  }
};

// How many arrays of each type a leaf kind stages per leaf, besides the
// variable bytes: items and transactions their offset; a validator its power,
// key offset and key type; a CommitSig its seconds, signature offset, nanos,
// flag and address; a header (one "leaf" a header: header.h) four 64-bit
// fields, twelve offsets and two 32-bit fields
struct LeafArrays {
  uint32_t i64, off, i32, u8, addr;
  uint64_t bytes() const { return 8 * i64 + 4 * off + 4 * i32 + u8 + 20 * addr; }
};

LeafArrays leaf_arrays(MerkleLeafKind k) {
  switch (k) {
    case kMerkleValidators: return {1, 1, 0, 1, 0};
    case kMerkleCommitSigs: return {1, 1, 1, 1, 1};
    case kMerkleHeaders: return {kHeaderU64Fields, kHeaderVarFields, kHeaderU32Fields, 0, 0};
    default: return {0, 1, 0, 0, 0};
  }
}

// One run, trees [a, b) of S, enqueued on D.stream through staging slot M;
// its roots arrive in M.h_out (digest words) when M.done has passed.
int enqueue_run(cmtv_ctx* ctx, CmtvDev& D, MerkleSlot& M, const TreeSource& S, size_t a, size_t b) {
  const size_t nt = b - a;
  // the passes' prefix arrays: pref[0] the leaves', pref[p + 1] pass p's
  // workgroups' (and pass p + 1's leaves'), until every tree has one node
  std::vector<std::vector<uint32_t>> pref(1, std::vector<uint32_t>(nt + 1, 0u));
  uint64_t nl = 0, vb = 0;
  for (size_t t = 0; t < nt; t++) {
    nl += S.leaves(a + t);
    vb += S.var_bytes(a + t);
    pref[0][t + 1] = (uint32_t)nl;
  }
  // (one tree may bring up to 2^32 - 1 leaves and as many bytes: u32 all the same)
  if (nl > 0xFFFFFFFFull || vb + 4 > 0xFFFFFFFFull) return CMTV_EINVAL;
  do {
    const std::vector<uint32_t>& p = pref.back();
    std::vector<uint32_t> q(nt + 1, 0u);
    for (size_t t = 0; t < nt; t++) q[t + 1] = q[t] + merkle_blocks(p[t + 1] - p[t]);
    pref.push_back(std::move(q));
  } while (pref.back()[nt] != nt);
  // (a header is reduced to its root by the one launch: no prefix arrays staged)
  const bool headers = S.kind == kMerkleHeaders;
  const size_t n_pass = pref.size() - 1, n_pref = headers ? 0 : pref.size();
  const LeafArrays A = leaf_arrays(S.kind);
  MerkleStage L;
  L.n = nl;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o = align_up(o + bytes, 16);
    return at;
  };
  L.o_pref = take(4 * (nt + 1) * n_pref);
  L.o_i64 = take(8 * nl * A.i64);
  L.o_off = take(4 * (nl * A.off + 1));
  L.o_i32 = take(4 * nl * A.i32);
  L.o_u8 = take(nl * A.u8);
  L.o_addr = take(20 * nl * A.addr);
  // + 4: the aligned reads of the last item end inside its last byte's word
  L.o_var = take(vb + 4);
  L.bytes = o;
  const size_t w0 = pref[1][nt], w1 = n_pass > 1 ? pref[2][nt] : 0;
  hipError_t e;
  if ((e = M.h_in.ensure(L.bytes)) != hipSuccess) return hip_fail(e);
  if ((e = M.d_in.ensure(L.bytes)) != hipSuccess) return hip_fail(e);
  if ((e = M.d_nodes.ensure(32 * (w0 + w1))) != hipSuccess) return hip_fail(e);
  if ((e = M.h_out.ensure(32 * nt)) != hipSuccess) return hip_fail(e);
  if (!M.done && (e = hipEventCreateWithFlags(&M.done, hipEventDisableTiming)) != hipSuccess) return hip_fail(e);
  auto* h = static_cast<uint8_t*>(M.h_in.p);
  for (size_t p = 0; p < n_pref; p++) std::memcpy(h + L.o_pref + 4 * (nt + 1) * p, pref[p].data(), 4 * (nt + 1));
  L.i64 = reinterpret_cast<int64_t*>(h + L.o_i64);
  L.off = reinterpret_cast<uint32_t*>(h + L.o_off);
  L.i32 = reinterpret_cast<int32_t*>(h + L.o_i32);
  L.u8 = h + L.o_u8;
  L.addr = h + L.o_addr;
  L.var = h + L.o_var;
  uint32_t var0 = 0;
  for (size_t t = 0; t < nt; t++) {
    S.pack(a + t, pref[0][t], var0, L);
    var0 += (uint32_t)S.var_bytes(a + t);
  }
  L.off[nl * A.off] = var0;
  std::memset(L.var + vb, 0, 4);
  auto* d = static_cast<uint8_t*>(M.d_in.p);
  hipStream_t s = D.stream;
  if ((e = hipMemcpyAsync(d, h, L.bytes, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e);
  MerkleLeaves leaves;
  leaves.var = d + L.o_var;
  leaves.off = reinterpret_cast<const uint32_t*>(d + L.o_off);
  leaves.i64 = reinterpret_cast<const int64_t*>(d + L.o_i64);
  leaves.i32 = reinterpret_cast<const int32_t*>(d + L.o_i32);
  leaves.u8 = d + L.o_u8;
  leaves.addr = d + L.o_addr;
  auto* nodes = static_cast<uint32_t*>(M.d_nodes.p);
  uint32_t* out = nodes;
  // one run in timing_every has its passes between an event pair (cmtv_stats device_ms)
  Timing::Pair tp{};
  const bool timed = ctx->timing_every && D.timing_seq++ % ctx->timing_every == 0;
  if (timed && (e = D.timing.begin(tp, s)) != hipSuccess) return hip_fail(e);
  for (size_t p = 0; p < n_pass; p++) {
    // pass p writes pref[p + 1][nt] nodes: the two halves of d_nodes in turn
    // (the passes' node counts never grow, so both fit)
    out = (p & 1) ? nodes + 8 * w0 : nodes;
    const auto* d_pref = reinterpret_cast<const uint32_t*>(d + L.o_pref);
    if (fault_hit(ctx) || D.inject_fault)
      e = hipErrorLaunchFailure;
    else if (headers)
      e = launch_header_hash(leaves, (uint32_t)nt, out, s);
    else
      e = launch_merkle_pass(p ? kMerkleNodes : S.kind, leaves, d_pref + (nt + 1) * (p + 1), d_pref + (nt + 1) * p,
                             (uint32_t)nt, pref[p + 1][nt], out, s);
    if (e != hipSuccess) {
      D.timing.abandon(tp);
      return hip_fail(e);
    }
    ctx->stats.kernel_launches++;
    D.launches++;
    leaves.nodes = out;
  }
  if (timed && (e = D.timing.end(tp, s)) != hipSuccess) return hip_fail(e);
  if ((e = hipMemcpyAsync(M.h_out.p, out, 32 * nt, hipMemcpyDeviceToHost, s)) != hipSuccess) return hip_fail(e);
  if ((e = hipEventRecord(M.done, s)) != hipSuccess) return hip_fail(e);
  return CMTV_OK;
}

// The roots of S's trees (32 bytes each) into roots. Caller holds the
// context lock; devs[0] is current.
int merkle_roots_locked(cmtv_ctx* ctx, const TreeSource& S, uint8_t* roots) {
  CmtvDev& D = ctx->devs[0];
  D.timing.harvest(ctx->stats, D.device_ms, D.timed_calls, false);
  struct Span {
    size_t a = 0, b = 0;
    bool pending = false;
  } span[2];
  auto finish = [&](int k) -> int {
    if (!span[k].pending) return CMTV_OK;
    span[k].pending = false;
    const hipError_t e = hipEventSynchronize(D.merkle[k].done);
    if (e != hipSuccess) return hip_fail(e);
    const auto* w = static_cast<const uint32_t*>(D.merkle[k].h_out.p);
    uint8_t* r = roots + 32 * span[k].a;
    for (size_t i = 0; i < 8 * (span[k].b - span[k].a); i++) {
      const uint32_t be = __builtin_bswap32(w[i]);
      std::memcpy(r + 4 * i, &be, 4);
    }
    return CMTV_OK;
  };
  const uint64_t per_leaf = leaf_arrays(S.kind).bytes();
  int rc = CMTV_OK;
  size_t t = 0;
  for (int k = 0; t < S.n_trees && rc == CMTV_OK; k ^= 1) {
    size_t b = t;
    uint64_t bytes = 0;
    do {
      bytes += 16 + per_leaf * S.leaves(b) + S.var_bytes(b);
      b++;
    } while (b < S.n_trees && b - t < kRunTrees &&
             bytes + 16 + per_leaf * S.leaves(b) + S.var_bytes(b) <= kRunBytes);
    if ((rc = finish(k)) != CMTV_OK) break;  // the slot's previous run
    if ((rc = enqueue_run(ctx, D, D.merkle[k], S, t, b)) != CMTV_OK) break;
    span[k].a = t;
    span[k].b = b;
    span[k].pending = true;
    t = b;
  }
  for (int k = 0; k < 2 && rc == CMTV_OK; k++) rc = finish(k);
  // after an error the copies and launches already enqueued still use the staging
  if (rc != CMTV_OK) (void)hipStreamSynchronize(D.stream);
  return rc;
}

}  // namespace

void ItemTrees::pack(size_t t, uint32_t leaf0, uint32_t var0, const MerkleStage& S) const {
  const uint32_t n = leaves(t);
  if (!n) return;
  const uint32_t* io = item_off + tree_off[t];
  pack_offsets(S.off + leaf0, io, n, var0);
  if (io[n] != io[0]) std::memcpy(S.var + var0, items + io[0], io[n] - io[0]);
}

bool merkle_item_trees_ok(size_t n_trees, const uint32_t* tree_off, const uint8_t* items, const uint32_t* item_off,
                          const uint8_t* out) {
  if (!tree_off || !out || !merkle_offsets_ok(tree_off, n_trees)) return false;
  const uint32_t first = tree_off[0], last = tree_off[n_trees];
  if (last != first) {
    if (!item_off || !merkle_offsets_ok(item_off + first, last - first)) return false;
    if (!items && item_off[last] != item_off[first]) return false;
  }
  return true;
}

// A call: the context lock, the first device, the roots into a buffer of the
// call's own and into out only when all of them are there.
int merkle_call(cmtv_ctx* ctx, const TreeSource& S, uint8_t* out) {
  std::unique_lock<std::mutex> lk;
  if (ctx_lock(ctx, lk) != CMTV_OK) return CMTV_ENODEV;
  if (ctx->devs.empty() || ctx->devs[0].failed) return CMTV_ENODEV;
  std::vector<uint8_t> roots(32 * S.n_trees);
  const int rc = merkle_roots_locked(ctx, S, roots.data());
  ctx->fault_pending = false;  // CMTV_FAULT_AT's failure belongs to this call
  if (rc != CMTV_OK) return rc;
  ctx->stats.calls++;
  std::memcpy(out, roots.data(), roots.size());
  return CMTV_OK;
}

namespace {

bool valset_ok(const cmtv_valset& v, const uint8_t* kt) {
  if (v.n_vals == 0) return true;
  if (!v.pubkeys || !v.pk_off || !v.voting_power) return false;
  for (uint32_t i = 0; i < v.n_vals; i++) {
    if (v.pk_off[i + 1] < v.pk_off[i]) return false;
    if (!validator_ok(kt ? kt[i] : CMTV_KEY_ED25519, v.pk_off[i + 1] - v.pk_off[i])) return false;
  }
  return true;
}

// *wide: a signature of more than 64 bytes (the host-encoded route)
bool commit_ok(const cmtv_commit& c, bool* wide) {
  *wide = false;
  if (c.n_sigs == 0) return true;
  if (!c.flags || !c.ts_seconds || !c.ts_nanos || !c.sig_off) return false;
  if (!merkle_offsets_ok(c.sig_off, c.n_sigs)) return false;
  if (!c.sigs && c.sig_off[c.n_sigs] != c.sig_off[0]) return false;
  for (uint32_t i = 0; i < c.n_sigs; i++) {
    if (!merkle_timestamp_ok(c.ts_seconds[i], c.ts_nanos[i])) return false;
    if (!c.val_addrs && c.flags[i] != kMerkleFlagAbsent) return false;
    if (c.sig_off[i + 1] - c.sig_off[i] > 64) *wide = true;
  }
  return true;
}

}  // namespace
}  // namespace cmtv

using namespace cmtv;

extern "C" {

int cmtv_merkle_roots(cmtv_ctx* ctx, size_t n_trees, const uint32_t* tree_off, const uint8_t* items,
                      const uint32_t* item_off, uint8_t* out) {
  if (!ctx || n_trees > (1ull << 31)) return CMTV_EINVAL;
  if (n_trees == 0) return CMTV_OK;
  if (!merkle_item_trees_ok(n_trees, tree_off, items, item_off, out)) return CMTV_EINVAL;
  return merkle_call(ctx, ItemTrees(kMerkleItems, n_trees, tree_off, items, item_off), out);
}

int cmtv_merkle_root(cmtv_ctx* ctx, size_t n, const uint8_t* items, const uint32_t* item_off, uint8_t out[32]) {
  if (n > 0xFFFFFFFFull) return CMTV_EINVAL;
  const uint32_t tree_off[2] = {0u, (uint32_t)n};
  return cmtv_merkle_roots(ctx, 1, tree_off, items, item_off, out);
}

int cmtv_txs_hashes(cmtv_ctx* ctx, size_t n_blocks, const uint32_t* block_off, const uint8_t* txs,
                    const uint32_t* tx_off, uint8_t* out) {
  if (!ctx || n_blocks > (1ull << 31)) return CMTV_EINVAL;
  if (n_blocks == 0) return CMTV_OK;
  if (!merkle_item_trees_ok(n_blocks, block_off, txs, tx_off, out)) return CMTV_EINVAL;
  return merkle_call(ctx, ItemTrees(kMerkleTxs, n_blocks, block_off, txs, tx_off), out);
}

int cmtv_txs_hash(cmtv_ctx* ctx, size_t n, const uint8_t* txs, const uint32_t* tx_off, uint8_t out[32]) {
  if (n > 0xFFFFFFFFull) return CMTV_EINVAL;
  const uint32_t block_off[2] = {0u, (uint32_t)n};
  return cmtv_txs_hashes(ctx, 1, block_off, txs, tx_off, out);
}

int cmtv_valset_hashes(cmtv_ctx* ctx, size_t n, const cmtv_valset* vals, const uint8_t* const* key_types,
                       uint8_t* out) {
  if (!ctx || n > (1ull << 31)) return CMTV_EINVAL;
  if (n == 0) return CMTV_OK;
  if (!vals || !out) return CMTV_EINVAL;
  for (size_t t = 0; t < n; t++)
    if (!valset_ok(vals[t], key_types ? key_types[t] : nullptr)) return CMTV_EINVAL;
  return merkle_call(ctx, ValidatorTrees(n, vals, key_types), out);
}

int cmtv_valset_hash(cmtv_ctx* ctx, const cmtv_valset* vals, const uint8_t* key_types, uint8_t out[32]) {
  return cmtv_valset_hashes(ctx, 1, vals, key_types ? &key_types : nullptr, out);
}

int cmtv_commit_hashes(cmtv_ctx* ctx, size_t n, const cmtv_commit* commits, uint8_t* out) {
  if (!ctx || n > (1ull << 31)) return CMTV_EINVAL;
  if (n == 0) return CMTV_OK;
  if (!commits || !out) return CMTV_EINVAL;
  // commits whose signatures all fit the device leaf builder, and the others
  CommitTrees dev;
  std::vector<size_t> dev_at, wide_at;
  for (size_t t = 0; t < n; t++) {
    bool wide;
    if (!commit_ok(commits[t], &wide)) return CMTV_EINVAL;
    (wide ? wide_at : dev_at).push_back(t);
    if (!wide) dev.commits.push_back(&commits[t]);
  }
  dev.n_trees = dev.commits.size();
  if (wide_at.empty()) return merkle_call(ctx, dev, out);
  // a signature of more than 64 bytes: that commit's leaves are encoded here
  // (encode_commit_sig) and hashed as items
  std::vector<uint8_t> items;
  std::vector<uint32_t> item_off(1, 0u), tree_off(1, 0u);
  for (size_t t : wide_at) {
    const cmtv_commit& c = commits[t];
    for (uint32_t i = 0; i < c.n_sigs; i++) {
      encode_commit_sig(items, c.flags[i], c.flags[i] != kMerkleFlagAbsent ? c.val_addrs + 20 * (size_t)i : nullptr,
                        c.ts_seconds[i], c.ts_nanos[i], c.sigs + c.sig_off[i], c.sig_off[i + 1] - c.sig_off[i]);
      if (items.size() > 0xFFFFFFF0ull) return CMTV_EINVAL;
      item_off.push_back((uint32_t)items.size());
    }
    tree_off.push_back((uint32_t)(item_off.size() - 1));
  }
  std::vector<uint8_t> roots(32 * n);
  int rc = CMTV_OK;
  std::vector<uint8_t> part(32 * std::max(dev_at.size(), wide_at.size()));
  if (!dev_at.empty()) {
    if ((rc = merkle_call(ctx, dev, part.data())) != CMTV_OK) return rc;
    for (size_t k = 0; k < dev_at.size(); k++) std::memcpy(&roots[32 * dev_at[k]], &part[32 * k], 32);
  }
  rc = merkle_call(ctx, ItemTrees(kMerkleItems, wide_at.size(), tree_off.data(), items.data(), item_off.data()), part.data());
  if (rc != CMTV_OK) return rc;
  for (size_t k = 0; k < wide_at.size(); k++) std::memcpy(&roots[32 * wide_at[k]], &part[32 * k], 32);
  std::memcpy(out, roots.data(), roots.size());
  return CMTV_OK;
}

int cmtv_commit_hash(cmtv_ctx* ctx, const cmtv_commit* commit, uint8_t out[32]) {
  return cmtv_commit_hashes(ctx, 1, commit, out);
}

int cmtv_validator_bytes(uint32_t key_type, const uint8_t* pk, size_t pk_len, int64_t power, uint8_t* out,
                         size_t cap) {
  if (!pk || (!out && cap) || !validator_ok(key_type, pk_len)) return CMTV_EINVAL;
  uint8_t b[kValidatorBytesMax];
  const size_t n = encode_validator(b, key_type, pk, pk_len, power);
  if (n <= cap) std::memcpy(out, b, n);
  return (int)n;
}

int cmtv_commit_sig_bytes(uint32_t flag, const uint8_t* addr20_or_null, int64_t ts_seconds, int32_t ts_nanos,
                          const uint8_t* sig, size_t sig_len, uint8_t* out, size_t cap) {
  if ((!sig && sig_len) || (!out && cap) || sig_len > (1u << 30) || !merkle_timestamp_ok(ts_seconds, ts_nanos))
    return CMTV_EINVAL;
  std::vector<uint8_t> b;
  encode_commit_sig(b, flag, addr20_or_null, ts_seconds, ts_nanos, sig, sig_len);
  if (b.size() <= cap && !b.empty()) std::memcpy(out, b.data(), b.size());
  return (int)b.size();
}

}  // extern "C"
