// merkle_proof.cpp -- the host layer of the merkle proofs (merkle_proof.h,
// merkle_proof.hip): the C ABI's cmtv_merkle_proof[s]_len, cmtv_merkle_proofs,
// cmtv_txs_proofs, cmtv_part_set_proofs and cmtv_merkle_proofs_verify. The
// calls run as the merkle root calls do (merkle.cpp): cut into runs, a run
// one pinned staging block, one copy to the context's first device, its
// launches on that device's stream and its results back, through the same two
// staging slots, so the host packs a run while the device works on the one
// before. A run is bounded by its output bytes as well as its staged bytes.
// Results reach the caller's buffers only when every run is in: a call of one
// run converts them there from the pinned block, a longer one collects them
// in buffers of its own first.
#include "merkle_internal.h"
// (after hip_runtime.h, which defines CMTV_HD's attributes for a host compile)
#include "merkle_proof.h"

#include <new>
#include <unordered_map>

namespace cmtv {
namespace {

constexpr uint64_t kRunBytes = 32ull << 20;  // of a run's staging, and of its results
constexpr size_t kRunTrees = 1u << 20;
constexpr size_t kRunProofs = 1u << 24;

// n hashes of digest words as bytes
void put_hashes(uint8_t* dst, const uint32_t* w, size_t n) {
  for (size_t i = 0; i < 8 * n; i++) {
    const uint32_t be = __builtin_bswap32(w[i]);
    std::memcpy(dst + 4 * i, &be, 4);
  }
}

// Both staging slots in turn over the call's pieces: cut(t) is where the run
// that starts at piece t ends, enqueue(M, a, b) puts it on the stream through
// slot M, collect(M, a, b) takes its results once M.done has passed.
template <class Cut, class Enqueue, class Collect>
int run_slots(CmtvDev& D, size_t n, Cut cut, Enqueue enqueue, Collect collect) {
  struct Span {
    size_t a = 0, b = 0;
    bool pending = false;
  } span[2];
  auto finish = [&](int k) -> int {
    if (!span[k].pending) return CMTV_OK;
    span[k].pending = false;
    const hipError_t e = hipEventSynchronize(D.merkle[k].done);
    if (e != hipSuccess) return hip_fail(e);
    collect(D.merkle[k], span[k].a, span[k].b);
    return CMTV_OK;
  };
  int rc = CMTV_OK;
  size_t t = 0;
  try {
    for (int k = 0; t < n && rc == CMTV_OK; k ^= 1) {
      const size_t b = cut(t);
      if ((rc = finish(k)) != CMTV_OK) break;  // the slot's previous run
      if ((rc = enqueue(D.merkle[k], t, b)) != CMTV_OK) break;
      span[k].a = t;
      span[k].b = b;
      span[k].pending = true;
      t = b;
    }
    for (int k = 0; k < 2 && rc == CMTV_OK; k++) rc = finish(k);
  } catch (const std::bad_alloc&) {  // a run's plan could not be allocated
    rc = CMTV_ENOMEM;
  }
  // after an error the copies and launches already enqueued still use the staging
  if (rc != CMTV_OK) (void)hipStreamSynchronize(D.stream);
  return rc;
}

struct Taker {
  size_t o = 0;
  size_t operator()(size_t bytes) {
    const size_t at = o;
    o = align_up(o + bytes, 32);
    return at;
  }
};

// ------------------------------------------------------------------ building
// Where a call's results go: the caller's buffers or the call's own, from
// the call's first tree and item on
struct ProofDst {
  uint8_t* roots;
  uint8_t* leaf_hashes;
  uint8_t* aunts;
};

// What a run left in its slot's h_out: roots | leaf hashes | aunts
struct ProofRunOut {
  size_t o_lh = 0, o_aunts = 0;
};

struct ProofBuild {
  cmtv_ctx* ctx;
  const ItemTrees& S;
  std::vector<uint32_t> item0;     // tree t's first item, counted from the call's first
  std::vector<uint32_t> aunt_off;  // per item of the call, the result
  ProofRunOut out[2];

  uint64_t tree_out_bytes(size_t t) const {
    return 32ull * (1 + S.leaves(t) + (aunt_off[item0[t + 1]] - aunt_off[item0[t]]));
  }

  // One run, trees [a, b), through slot M (merkle.cpp enqueue_run with the nodes kept)
  int enqueue(CmtvDev& D, MerkleSlot& M, size_t a, size_t b) {
    const size_t nt = b - a;
    std::vector<std::vector<uint32_t>> pref(1, std::vector<uint32_t>(nt + 1, 0u));
    uint64_t nl = 0, vb = 0;
    for (size_t t = 0; t < nt; t++) {
      nl += S.leaves(a + t);
      vb += S.var_bytes(a + t);
      pref[0][t + 1] = (uint32_t)nl;
    }
    if (nl > 0xFFFFFFFFull || vb + 4 > 0xFFFFFFFFull) return CMTV_EINVAL;
    do {
      const std::vector<uint32_t>& p = pref.back();
      std::vector<uint32_t> q(nt + 1, 0u);
      for (size_t t = 0; t < nt; t++) q[t + 1] = q[t] + merkle_blocks(p[t + 1] - p[t]);
      pref.push_back(std::move(q));
    } while (pref.back()[nt] != nt);
    const size_t n_pass = pref.size() - 1, n_pref = pref.size();
    if (n_pass > kProofMaxPasses + 1) return CMTV_EINVAL;
    // the aunts that the passes after the first collect, once per block node:
    // up_off over those passes' leaves, concatenated
    ProofSpread sp{};
    std::vector<uint32_t> up_off(1, 0u);
    for (size_t p = 1; p < n_pass; p++) {
      sp.up_base[p] = (uint32_t)(up_off.size() - 1);
      for (size_t t = 0; t < nt; t++) {
        const uint32_t n = pref[p][t + 1] - pref[p][t];
        for (uint32_t j = 0; j < n; j++) {
          const uint32_t left = n - (j & ~(kMerkleB - 1));
          up_off.push_back(up_off.back() +
                           merkle_proof_len<uint32_t>(std::min(left, kMerkleB), j & (kMerkleB - 1)));
        }
      }
    }
    const size_t n_up = up_off.back();
    const uint32_t a0 = aunt_off[item0[a]];
    const size_t na = aunt_off[item0[b]] - a0;

    MerkleStage L;
    L.n = nl;
    Taker take;
    L.o_pref = take(4 * (nt + 1) * n_pref);
    L.o_off = take(4 * (nl + 1));
    const size_t o_aoff = take(4 * (nl + 1)), o_uoff = take(4 * up_off.size());
    // + 4: the aligned reads of the last item end inside its last byte's word
    L.o_var = take(vb + 4);
    L.bytes = take.o;
    Taker take_out;
    const size_t d_lh = take_out(32 * nl), d_aunts = take_out(32 * na), d_up = take_out(32 * n_up);
    const size_t w0 = pref[1][nt], w1 = n_pass > 1 ? pref[2][nt] : 0;
    ProofRunOut& R = out[&M - D.merkle];
    R.o_lh = 32 * nt;
    R.o_aunts = R.o_lh + 32 * nl;
    hipError_t e;
    if ((e = M.h_in.ensure(L.bytes)) != hipSuccess) return hip_fail(e);
    if ((e = M.d_in.ensure(L.bytes)) != hipSuccess) return hip_fail(e);
    if ((e = M.d_nodes.ensure(32 * (w0 + w1))) != hipSuccess) return hip_fail(e);
    if ((e = M.d_out.ensure(std::max<size_t>(take_out.o, 32))) != hipSuccess) return hip_fail(e);
    if ((e = M.h_out.ensure(R.o_aunts + 32 * na)) != hipSuccess) return hip_fail(e);
    if (!M.done && (e = hipEventCreateWithFlags(&M.done, hipEventDisableTiming)) != hipSuccess) return hip_fail(e);
    auto* h = static_cast<uint8_t*>(M.h_in.p);
    for (size_t p = 0; p < n_pref; p++) std::memcpy(h + L.o_pref + 4 * (nt + 1) * p, pref[p].data(), 4 * (nt + 1));
    L.off = reinterpret_cast<uint32_t*>(h + L.o_off);
    L.var = h + L.o_var;
    uint32_t var0 = 0;
    for (size_t t = 0; t < nt; t++) {
      S.pack(a + t, pref[0][t], var0, L);
      var0 += (uint32_t)S.var_bytes(a + t);
    }
    L.off[nl] = var0;
    std::memset(L.var + vb, 0, 4);
    auto* h_aoff = reinterpret_cast<uint32_t*>(h + o_aoff);
    for (size_t i = 0; i <= nl; i++) h_aoff[i] = aunt_off[item0[a] + i] - a0;
    std::memcpy(h + o_uoff, up_off.data(), 4 * up_off.size());

    auto* d = static_cast<uint8_t*>(M.d_in.p);
    auto* dout = static_cast<uint8_t*>(M.d_out.p);
    hipStream_t s = D.stream;
    if ((e = hipMemcpyAsync(d, h, L.bytes, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e);
    MerkleLeaves leaves;
    leaves.var = d + L.o_var;
    leaves.off = reinterpret_cast<const uint32_t*>(d + L.o_off);
    const auto* d_pref = reinterpret_cast<const uint32_t*>(d + L.o_pref);
    const auto* d_aoff = reinterpret_cast<const uint32_t*>(d + o_aoff);
    const auto* d_uoff = reinterpret_cast<const uint32_t*>(d + o_uoff);
    auto* nodes = static_cast<uint32_t*>(M.d_nodes.p);
    uint32_t* root_nodes = nodes;
    Timing::Pair tp{};
    const bool timed = ctx->timing_every && D.timing_seq++ % ctx->timing_every == 0;
    if (timed && (e = D.timing.begin(tp, s)) != hipSuccess) return hip_fail(e);
    auto launched = [&](hipError_t le) -> int {
      if (le != hipSuccess) {
        D.timing.abandon(tp);
        return hip_fail(le);
      }
      ctx->stats.kernel_launches++;
      D.launches++;
      return CMTV_OK;
    };
    for (size_t p = 0; p < n_pass; p++) {
      root_nodes = (p & 1) ? nodes + 8 * w0 : nodes;
      if (fault_hit(ctx) || D.inject_fault)
        e = hipErrorLaunchFailure;
      else
        e = launch_merkle_proof_pass(p ? kMerkleNodes : S.kind, leaves, d_pref + (nt + 1) * (p + 1),
                                     d_pref + (nt + 1) * p, (uint32_t)nt, pref[p + 1][nt], root_nodes,
                                     p ? nullptr : reinterpret_cast<uint32_t*>(dout + d_lh),
                                     p ? d_uoff + sp.up_base[p] : d_aoff,
                                     reinterpret_cast<uint32_t*>(dout + (p ? d_up : d_aunts)), s);
      if (const int rc = launched(e)) return rc;
      leaves.nodes = root_nodes;
    }
    if (n_pass > 1 && n_up > 0) {
      sp.pref = d_pref;
      sp.aunt_off = d_aoff;
      sp.up_off = d_uoff;
      sp.up = reinterpret_cast<const uint32_t*>(dout + d_up);
      sp.aunts = reinterpret_cast<uint32_t*>(dout + d_aunts);
      sp.n_trees = (uint32_t)nt;
      sp.n_pass = (uint32_t)n_pass;
      sp.n_leaves = (uint32_t)nl;
      e = (fault_hit(ctx) || D.inject_fault) ? hipErrorLaunchFailure : launch_merkle_proof_spread(sp, s);
      if (const int rc = launched(e)) return rc;
    }
    if (timed && (e = D.timing.end(tp, s)) != hipSuccess) return hip_fail(e);
    auto* ho = static_cast<uint8_t*>(M.h_out.p);
    if ((e = hipMemcpyAsync(ho, root_nodes, 32 * nt, hipMemcpyDeviceToHost, s)) != hipSuccess) return hip_fail(e);
    // (the leaf hashes and the aunts are neighbours on the device only up to d_aunts' alignment, which is 32)
    if (nl && (e = hipMemcpyAsync(ho + R.o_lh, dout + d_lh, 32 * (nl + na), hipMemcpyDeviceToHost, s)) != hipSuccess)
      return hip_fail(e);
    if ((e = hipEventRecord(M.done, s)) != hipSuccess) return hip_fail(e);
    return CMTV_OK;
  }

  void collect(CmtvDev& D, MerkleSlot& M, size_t a, size_t b, const ProofDst& dst) const {
    const ProofRunOut& R = out[&M - D.merkle];
    const auto* ho = static_cast<const uint8_t*>(M.h_out.p);
    const size_t i0 = item0[a], nl = item0[b] - i0, a0 = aunt_off[i0], na = aunt_off[item0[b]] - a0;
    put_hashes(dst.roots + 32 * a, reinterpret_cast<const uint32_t*>(ho), b - a);
    if (nl) put_hashes(dst.leaf_hashes + 32 * i0, reinterpret_cast<const uint32_t*>(ho + R.o_lh), nl);
    if (na) put_hashes(dst.aunts + 32 * a0, reinterpret_cast<const uint32_t*>(ho + R.o_aunts), na);
  }
};

// per item of the trees, its proof's first aunt; false when they pass 2^32 - 1
bool proof_offsets(size_t n_trees, const uint32_t* tree_off, std::vector<uint32_t>* off, uint64_t* total) {
  uint64_t sum = 0;
  if (off) {
    off->clear();
    off->reserve((size_t)(tree_off[n_trees] - tree_off[0]) + 1);
    off->push_back(0u);
  }
  for (size_t t = 0; t < n_trees; t++) {
    const uint32_t n = tree_off[t + 1] - tree_off[t];
    for (uint32_t i = 0; i < n; i++) {
      sum += merkle_proof_len<uint32_t>(n, i);
      if (off) {
        if (sum > 0xFFFFFFFFull) return false;
        off->push_back((uint32_t)sum);
      }
    }
  }
  *total = sum;
  return true;
}

int proofs_call(cmtv_ctx* ctx, MerkleLeafKind kind, size_t n_trees, const uint32_t* tree_off, const uint8_t* items,
                const uint32_t* item_off, uint8_t* roots, uint8_t* leaf_hashes, uint32_t* aunt_off, uint8_t* aunts,
                size_t cap_aunts) {
  if (!ctx || n_trees > (1ull << 31)) return CMTV_EINVAL;
  if (n_trees == 0) return CMTV_OK;
  if (!merkle_item_trees_ok(n_trees, tree_off, items, item_off, roots)) return CMTV_EINVAL;
  const size_t n_items = tree_off[n_trees] - tree_off[0];
  if (n_items && (!leaf_hashes || !aunt_off)) return CMTV_EINVAL;
  const ItemTrees S(kind, n_trees, tree_off, items, item_off);
  ProofBuild B{ctx, S, {}, {}, {}};
  uint64_t n_aunts = 0;
  if (!proof_offsets(n_trees, tree_off, &B.aunt_off, &n_aunts)) return CMTV_EINVAL;
  if (n_aunts > cap_aunts || (n_aunts && !aunts)) return CMTV_EINVAL;
  B.item0.resize(n_trees + 1);
  for (size_t t = 0; t <= n_trees; t++) B.item0[t] = tree_off[t] - tree_off[0];

  auto cut = [&](size_t t) {
    size_t b = t;
    uint64_t in = 0, out = 0;
    do {
      in += 16 + 8ull * S.leaves(b) + S.var_bytes(b);
      out += B.tree_out_bytes(b);
      b++;
    } while (b < n_trees && b - t < kRunTrees && in + 16 + 8ull * S.leaves(b) + S.var_bytes(b) <= kRunBytes &&
             out + B.tree_out_bytes(b) <= kRunBytes);
    return b;
  };
  std::unique_lock<std::mutex> lk;
  if (ctx_lock(ctx, lk) != CMTV_OK) return CMTV_ENODEV;
  if (ctx->devs.empty() || ctx->devs[0].failed) return CMTV_ENODEV;
  CmtvDev& D = ctx->devs[0];
  D.timing.harvest(ctx->stats, D.device_ms, D.timed_calls, false);
  // a call of one run converts its results straight into the caller's buffers
  // (nothing can fail after its event); a longer one collects them first
  const bool one_run = cut(0) == n_trees;
  std::vector<uint8_t> own_roots, own_lh, own_aunts;
  ProofDst dst{roots, leaf_hashes, aunts};
  if (!one_run) {
    own_roots.resize(32 * n_trees);
    own_lh.resize(32 * n_items);
    own_aunts.resize(32 * n_aunts);
    dst = ProofDst{own_roots.data(), own_lh.data(), own_aunts.data()};
  }
  const int rc = run_slots(
      D, n_trees, cut, [&](MerkleSlot& M, size_t a, size_t b) { return B.enqueue(D, M, a, b); },
      [&](MerkleSlot& M, size_t a, size_t b) { B.collect(D, M, a, b, dst); });
  ctx->fault_pending = false;  // CMTV_FAULT_AT's failure belongs to this call
  if (rc != CMTV_OK) return rc;
  ctx->stats.calls++;
  if (!one_run) {
    std::memcpy(roots, own_roots.data(), own_roots.size());
    if (n_items) std::memcpy(leaf_hashes, own_lh.data(), own_lh.size());
    if (n_aunts) std::memcpy(aunts, own_aunts.data(), own_aunts.size());
  }
  if (aunt_off) std::memcpy(aunt_off, B.aunt_off.data(), 4 * B.aunt_off.size());
  return CMTV_OK;
}

// ------------------------------------------------------------------ verifying
struct ProofVerify {
  cmtv_ctx* ctx;
  size_t n;
  const int64_t* total;
  const int64_t* index;
  const uint8_t* leaf_hashes;
  const uint32_t* aunt_off;
  const uint8_t* aunts;
  size_t n_roots;
  const uint8_t* roots;
  const uint32_t* root_idx;
  const uint8_t* leaves;
  const uint32_t* leaf_off;
  uint32_t leaf_kind;
  size_t o_hash[2] = {0, 0};  // where a run's hashes start in its slot's h_out, after the status bytes

  // the aunts proof i stages: none of a count no tree can have
  uint32_t staged(size_t i) const {
    const uint32_t c = aunt_off[i + 1] - aunt_off[i];
    return c > kProofMaxAunts ? 0u : c;
  }
  // (with root_idx a run stages the roots its proofs name, each once: at most one a proof)
  uint64_t proof_bytes(size_t i) const {
    return 72 + 32ull * staged(i) + (leaf_off ? leaf_off[i + 1] - leaf_off[i] : 0u) + (roots ? 32 : 0);
  }
  size_t cut(size_t t) const {
    size_t b = t;
    uint64_t in = 0;
    do {
      in += proof_bytes(b);
      b++;
    } while (b < n && b - t < kRunProofs && in + proof_bytes(b) <= kRunBytes);
    return b;
  }

  int enqueue(CmtvDev& D, MerkleSlot& M, size_t a, size_t b) {
    const size_t m = b - a;
    uint64_t na = 0;
    for (size_t i = a; i < b; i++) na += staged(i);
    const uint64_t lb = leaf_off ? leaf_off[b] - leaf_off[a] : 0;
    // the roots of the run: one a proof, or with root_idx those its proofs name, in order of first use
    std::vector<uint32_t> run_roots;
    std::unordered_map<uint32_t, uint32_t> root_at;
    if (roots && root_idx)
      for (size_t i = a; i < b; i++)
        if (root_at.emplace(root_idx[i], (uint32_t)run_roots.size()).second) run_roots.push_back(root_idx[i]);
    const size_t nr = !roots ? 0 : (root_idx ? run_roots.size() : m);
    if (na > 0xFFFFFFFFull) return CMTV_EINVAL;
    Taker take;
    const size_t o_total = take(8 * m), o_index = take(8 * m), o_lh = take(32 * m), o_at = take(4 * m),
                 o_cnt = take(4 * m), o_ridx = take(4 * m), o_loff = take(4 * (m + 1)), o_roots = take(32 * nr),
                 o_aunts = take(32 * na), o_leaves = take(lb + 4);
    Taker take_out;
    const size_t o_status = take_out(m), o_out = take_out(32 * m);
    o_hash[&M - D.merkle] = o_out;
    hipError_t e;
    if ((e = M.h_in.ensure(take.o)) != hipSuccess) return hip_fail(e);
    if ((e = M.d_in.ensure(take.o)) != hipSuccess) return hip_fail(e);
    if ((e = M.d_out.ensure(take_out.o)) != hipSuccess) return hip_fail(e);
    if ((e = M.h_out.ensure(take_out.o)) != hipSuccess) return hip_fail(e);
    if (!M.done && (e = hipEventCreateWithFlags(&M.done, hipEventDisableTiming)) != hipSuccess) return hip_fail(e);
    auto* h = static_cast<uint8_t*>(M.h_in.p);
    std::memcpy(h + o_total, total + a, 8 * m);
    std::memcpy(h + o_index, index + a, 8 * m);
    std::memcpy(h + o_lh, leaf_hashes + 32 * a, 32 * m);
    auto* at = reinterpret_cast<uint32_t*>(h + o_at);
    auto* cnt = reinterpret_cast<uint32_t*>(h + o_cnt);
    auto* ridx = reinterpret_cast<uint32_t*>(h + o_ridx);
    auto* loff = reinterpret_cast<uint32_t*>(h + o_loff);
    uint32_t pos = 0;
    for (size_t i = 0; i < m; i++) {
      const uint32_t k = staged(a + i);
      at[i] = pos;
      cnt[i] = aunt_off[a + i + 1] - aunt_off[a + i];
      if (k) std::memcpy(h + o_aunts + 32 * (size_t)pos, aunts + 32 * (size_t)aunt_off[a + i], 32 * (size_t)k);
      pos += k;
      ridx[i] = roots && root_idx ? root_at[root_idx[a + i]] : (uint32_t)i;
      loff[i] = leaf_off ? leaf_off[a + i] - leaf_off[a] : 0u;
    }
    loff[m] = (uint32_t)lb;
    if (nr && !root_idx) std::memcpy(h + o_roots, roots + 32 * a, 32 * nr);
    for (size_t k = 0; root_idx && k < nr; k++)
      std::memcpy(h + o_roots + 32 * k, roots + 32 * (size_t)run_roots[k], 32);
    if (lb) std::memcpy(h + o_leaves, leaves + leaf_off[a], lb);
    std::memset(h + o_leaves + lb, 0, 4);

    auto* d = static_cast<uint8_t*>(M.d_in.p);
    auto* dout = static_cast<uint8_t*>(M.d_out.p);
    hipStream_t s = D.stream;
    if ((e = hipMemcpyAsync(d, h, take.o, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e);
    ProofBatch P{};
    P.total = reinterpret_cast<const int64_t*>(d + o_total);
    P.index = reinterpret_cast<const int64_t*>(d + o_index);
    P.leaf_hash = d + o_lh;
    P.aunt_at = reinterpret_cast<const uint32_t*>(d + o_at);
    P.aunt_cnt = reinterpret_cast<const uint32_t*>(d + o_cnt);
    P.aunts = d + o_aunts;
    P.roots = roots ? d + o_roots : nullptr;
    P.root_idx = reinterpret_cast<const uint32_t*>(d + o_ridx);
    P.leaves = d + o_leaves;
    P.leaf_off = leaf_off ? reinterpret_cast<const uint32_t*>(d + o_loff) : nullptr;
    P.leaf_kind = leaf_kind;
    P.status = dout + o_status;
    P.out_hash = reinterpret_cast<uint32_t*>(dout + o_out);
    Timing::Pair tp{};
    const bool timed = ctx->timing_every && D.timing_seq++ % ctx->timing_every == 0;
    if (timed && (e = D.timing.begin(tp, s)) != hipSuccess) return hip_fail(e);
    e = (fault_hit(ctx) || D.inject_fault) ? hipErrorLaunchFailure : launch_merkle_proofs_verify(P, (uint32_t)m, s);
    if (e != hipSuccess) {
      D.timing.abandon(tp);
      return hip_fail(e);
    }
    ctx->stats.kernel_launches++;
    D.launches++;
    if (timed && (e = D.timing.end(tp, s)) != hipSuccess) return hip_fail(e);
    if ((e = hipMemcpyAsync(M.h_out.p, dout, take_out.o, hipMemcpyDeviceToHost, s)) != hipSuccess) return hip_fail(e);
    if ((e = hipEventRecord(M.done, s)) != hipSuccess) return hip_fail(e);
    return CMTV_OK;
  }
};

// (no exception crosses the C ABI: a call whose host buffers cannot be had is CMTV_ENOMEM)
template <class F>
int no_throw(F f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return CMTV_ENOMEM;
  }
}

}  // namespace
}  // namespace cmtv

using namespace cmtv;

extern "C" {

int cmtv_merkle_proof_len(uint64_t total, uint64_t index) {
  if (index >= total) return -1;
  return (int)merkle_proof_len<uint64_t>(total, index);
}

int cmtv_merkle_proofs_len(size_t n_trees, const uint32_t* tree_off, uint64_t* n_aunts) {
  if (!n_aunts || n_trees > (1ull << 31)) return CMTV_EINVAL;
  if (n_trees && (!tree_off || !merkle_offsets_ok(tree_off, n_trees))) return CMTV_EINVAL;
  uint64_t sum = 0;
  if (n_trees) proof_offsets(n_trees, tree_off, nullptr, &sum);
  *n_aunts = sum;
  return CMTV_OK;
}

int cmtv_merkle_proofs(cmtv_ctx* ctx, size_t n_trees, const uint32_t* tree_off, const uint8_t* items,
                       const uint32_t* item_off, uint8_t* roots, uint8_t* leaf_hashes, uint32_t* aunt_off,
                       uint8_t* aunts, size_t cap_aunts) {
  return no_throw([&] {
    return proofs_call(ctx, kMerkleItems, n_trees, tree_off, items, item_off, roots, leaf_hashes, aunt_off, aunts,
                       cap_aunts);
  });
}

int cmtv_txs_proofs(cmtv_ctx* ctx, size_t n_blocks, const uint32_t* block_off, const uint8_t* txs,
                    const uint32_t* tx_off, uint8_t* roots, uint8_t* leaf_hashes, uint32_t* aunt_off, uint8_t* aunts,
                    size_t cap_aunts) {
  return no_throw([&] {
    return proofs_call(ctx, kMerkleTxs, n_blocks, block_off, txs, tx_off, roots, leaf_hashes, aunt_off, aunts,
                       cap_aunts);
  });
}

int cmtv_part_set_proofs(cmtv_ctx* ctx, const uint8_t* data, size_t len, uint32_t part_size, uint32_t* total,
                         uint8_t root[32], uint8_t* leaf_hashes, uint32_t* aunt_off, uint8_t* aunts,
                         size_t cap_aunts) {
  if (!ctx || !total || !root || part_size == 0 || (uint64_t)len + part_size > (1ull << 32) || (!data && len))
    return CMTV_EINVAL;
  const uint32_t n = (uint32_t)(((uint64_t)len + part_size - 1) / part_size);
  // 2^28 parts have 28 aunts each or more: past what aunt_off can count, and refused before any allocation
  if (n >= (1u << 28)) return CMTV_EINVAL;
  return no_throw([&] {
    std::vector<uint32_t> item_off((size_t)n + 1);
    for (uint32_t i = 0; i <= n; i++) item_off[i] = (uint32_t)std::min<uint64_t>((uint64_t)i * part_size, len);
    const uint32_t tree_off[2] = {0u, n};
    const int rc = proofs_call(ctx, kMerkleItems, 1, tree_off, data, item_off.data(), root, leaf_hashes, aunt_off,
                               aunts, cap_aunts);
    if (rc == CMTV_OK) *total = n;
    return rc;
  });
}

int cmtv_merkle_proofs_verify(cmtv_ctx* ctx, size_t n, const int64_t* total, const int64_t* index,
                              const uint8_t* leaf_hashes, const uint32_t* aunt_off, const uint8_t* aunts,
                              size_t n_roots, const uint8_t* roots, const uint32_t* root_idx, const uint8_t* leaves,
                              const uint32_t* leaf_off, uint32_t leaf_kind, uint8_t* status, uint8_t* out_hash,
                              int* all_ok) {
  if (!ctx || n > (1ull << 31) || leaf_kind > kProofLeafTx) return CMTV_EINVAL;
  if (n == 0) {
    if (all_ok) *all_ok = 1;
    return CMTV_OK;
  }
  if (!total || !index || !leaf_hashes || !aunt_off || !status || !merkle_offsets_ok(aunt_off, n)) return CMTV_EINVAL;
  return no_throw([&]() -> int {
    ProofVerify V{ctx,  n,        total,  index,    leaf_hashes, aunt_off, aunts,
                  n_roots, roots, root_idx, leaves, leaf_off,    leaf_kind};
    if (!aunts)
      for (size_t i = 0; i < n; i++)
        if (V.staged(i)) return CMTV_EINVAL;
    if (!roots) {
      if (!out_hash) return CMTV_EINVAL;
    } else if (!root_idx) {
      if (n_roots != n) return CMTV_EINVAL;
    } else {
      if (n_roots > (1ull << 31)) return CMTV_EINVAL;
      for (size_t i = 0; i < n; i++)
        if (root_idx[i] >= n_roots) return CMTV_EINVAL;
    }
    if (leaf_off) {
      if (!merkle_offsets_ok(leaf_off, n) || (!leaves && leaf_off[n] != leaf_off[0])) return CMTV_EINVAL;
    } else if (leaves) {
      return CMTV_EINVAL;
    }
    std::unique_lock<std::mutex> lk;
    if (ctx_lock(ctx, lk) != CMTV_OK) return CMTV_ENODEV;
    if (ctx->devs.empty() || ctx->devs[0].failed) return CMTV_ENODEV;
    CmtvDev& D = ctx->devs[0];
    D.timing.harvest(ctx->stats, D.device_ms, D.timed_calls, false);
    const bool one_run = V.cut(0) == n;
    std::vector<uint8_t> own_status, own_hash;
    uint8_t* st = status;
    uint8_t* oh = out_hash;
    if (!one_run) {
      own_status.resize(n);
      st = own_status.data();
      if (out_hash) {
        own_hash.resize(32 * n);
        oh = own_hash.data();
      }
    }
    const int rc = run_slots(
        D, n, [&](size_t t) { return V.cut(t); },
        [&](MerkleSlot& M, size_t a, size_t b) { return V.enqueue(D, M, a, b); },
        [&](MerkleSlot& M, size_t a, size_t b) {
          const auto* ho = static_cast<const uint8_t*>(M.h_out.p);
          std::memcpy(st + a, ho, b - a);
          if (oh) put_hashes(oh + 32 * a, reinterpret_cast<const uint32_t*>(ho + V.o_hash[&M - D.merkle]), b - a);
        });
    ctx->fault_pending = false;  // CMTV_FAULT_AT's failure belongs to this call
    if (rc != CMTV_OK) return rc;
    ctx->stats.calls++;
    if (!one_run) {
      std::memcpy(status, own_status.data(), n);
      if (out_hash) std::memcpy(out_hash, own_hash.data(), 32 * n);
    }
    if (all_ok) {
      int ok = 1;
      for (size_t i = 0; i < n; i++) ok &= status[i] == kProofOk;
      *all_ok = ok;
    }
    return CMTV_OK;
  });
}

}  // extern "C"
