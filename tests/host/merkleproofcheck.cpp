// Host-side build of the merkle proof device code (cometbft_amd/csrc/
// merkle_proof.h, merkle.h, sha256.h). Test infrastructure only: checks the
// kernel source without a GPU (tests/test_merkle_proof_host.py, with
// -fsanitize=address,undefined), and times it on one CPU thread
// (tools/bench_merkle_proofs.py, -O2 without sanitizers).
//
// Default mode
//   input  (stdin):  u32 count, then records { u32 op, operands }
//     1 build   u32 kind (0 items, 1 transactions), u32 n_trees,
//               per tree { u32 n, per item { u32 len, item } }
//               -> per tree its root, then per item { leaf hash, u32 aunts, the aunts }:
//               the proof passes emulated lane by lane (merkle_block_of, the
//               leaf hash, merkle_aunt_lane, merkle_level_lane), then
//               merkle_proof_spread_lane per leaf; every buffer has the exact
//               size the host layer gives it
//     2 verify  u32 n, u32 has_leaves, u32 leaf_kind, u32 has_roots, per proof
//               { i64 total, i64 index, u8 leaf_hash[32], u32 aunts, the aunts,
//                 [u8 root[32]], [u32 len, leaf] }
//               -> per proof { u8 status, u8 out_hash[32] }: merkle_proof_verify_lane
//               over the staging the host layer builds (no aunt staged for a
//               count above 63)
// argv[1] == "bench":
//   bench build <kind> <n_trees> <n_leaves> <item_len> <reps>
//   bench verify <leaf_kind> <n> <total> <leaf_len> <reps>
//   -> one JSON line, the p50 wall time of one thread doing the call's hashing once
#define CMTV_HD inline
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../cometbft_amd/csrc/merkle_proof.h"

using namespace cmtv;

static bool rd(void* p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }

template <class T>
static T get() {
  T v{};
  if (!rd(&v, sizeof v)) {
    fprintf(stderr, "short input\n");
    exit(2);
  }
  return v;
}

static void emit(const uint32_t h[8]) {
  uint8_t out[32];
  for (int i = 0; i < 8; i++) {
    const uint32_t be = __builtin_bswap32(h[i]);
    memcpy(out + 4 * i, &be, 4);
  }
  fwrite(out, 1, 32, stdout);
}

// n nodes of 16-byte aligned words, exactly
struct Nodes {
  std::vector<MerkleQuad> q;
  explicit Nodes(size_t n) : q(2 * n) {}
  uint32_t* w() { return reinterpret_cast<uint32_t*>(q.data()); }
};

typedef std::vector<std::vector<std::vector<uint8_t>>> Trees;

struct Built {
  std::vector<uint32_t> roots, leaf_hashes, aunts, aunt_off;
};

// ProofsFromByteSlices of the trees, the way the kernels and the host layer compute it
static Built build(const Trees& T, uint32_t kind) {
  const uint32_t nt = (uint32_t)T.size();
  std::vector<const std::vector<uint8_t>*> items;
  std::vector<std::vector<uint32_t>> pref(1, std::vector<uint32_t>(nt + 1, 0));
  for (uint32_t t = 0; t < nt; t++) {
    for (const auto& it : T[t]) items.push_back(&it);
    pref[0][t + 1] = (uint32_t)items.size();
  }
  const uint32_t nl = (uint32_t)items.size();
  do {
    const std::vector<uint32_t>& p = pref.back();
    std::vector<uint32_t> q(nt + 1, 0);
    for (uint32_t t = 0; t < nt; t++) q[t + 1] = q[t] + merkle_blocks(p[t + 1] - p[t]);
    pref.push_back(std::move(q));
  } while (pref.back()[nt] != nt);
  const uint32_t n_pass = (uint32_t)pref.size() - 1;
  std::vector<uint32_t> flat;  // the prefix arrays as the run stages them
  for (const auto& p : pref) flat.insert(flat.end(), p.begin(), p.end());
  // a proof's place: the prefix sum of the count function
  Built R;
  R.aunt_off.assign(1, 0);
  for (uint32_t t = 0; t < nt; t++) {
    const uint32_t n = (uint32_t)T[t].size();
    for (uint32_t i = 0; i < n; i++) R.aunt_off.push_back(R.aunt_off.back() + merkle_proof_len<uint32_t>(n, i));
  }
  ProofSpread sp{};
  std::vector<uint32_t> up_off(1, 0);
  for (uint32_t p = 1; p < n_pass; p++) {
    sp.up_base[p] = (uint32_t)up_off.size() - 1;
    for (uint32_t t = 0; t < nt; t++) {
      const uint32_t n = pref[p][t + 1] - pref[p][t];
      for (uint32_t j = 0; j < n; j++) {
        const uint32_t left = n - (j & ~(kMerkleB - 1));
        up_off.push_back(up_off.back() + merkle_proof_len<uint32_t>(std::min(left, kMerkleB), j & (kMerkleB - 1)));
      }
    }
  }
  Nodes lh(nl), aunts(R.aunt_off.back()), up(up_off.back());
  std::vector<uint32_t> nodes;  // the previous pass's output
  for (uint32_t p = 0; p < n_pass; p++) {
    const uint32_t* leaf_off = &flat[(size_t)(nt + 1) * p];
    const uint32_t* wg_off = &flat[(size_t)(nt + 1) * (p + 1)];
    const uint32_t* aoff = p ? up_off.data() + sp.up_base[p] : R.aunt_off.data();
    uint32_t* adst = p ? up.w() : aunts.w();
    Nodes out(wg_off[nt]);
    alignas(16) static uint32_t lv[2][8 * kMerkleB];
    for (uint32_t g = 0; g < wg_off[nt]; g++) {
      const MerkleBlock b = merkle_block_of(g, wg_off, leaf_off, nt);
      uint32_t h[8];
      if (b.m == 0) {
        merkle_empty(h);
        merkle_store_node(out.w() + 8 * (size_t)g, h);
        continue;
      }
      std::vector<uint32_t*> dst(b.m);
      for (uint32_t lane = 0; lane < b.m; lane++) {
        if (p == 0) {
          const auto& it = *items[b.first + lane];
          // a copy that ends at the item's last word, at a varying alignment
          const uint32_t al = (b.first + lane) & 3, len = (uint32_t)it.size();
          std::vector<uint32_t> buf((al + len + 3) / 4 + (al + len == 0));
          uint8_t* q = reinterpret_cast<uint8_t*>(buf.data()) + al;
          if (len) memcpy(q, it.data(), len);
          if (kind == 1)
            merkle_tx_leaf_hash(h, q, len);
          else
            merkle_leaf_hash(h, q, len);
          merkle_store_node(lh.w() + 8 * (size_t)(b.first + lane), h);
        } else {
          merkle_load_node(h, &nodes[8 * (size_t)(b.first + lane)]);
        }
        for (int k = 0; k < 8; k++) lv[0][k * kMerkleB + lane] = h[k];
        dst[lane] = adst + 8 * (size_t)aoff[b.first + lane];
      }
      uint32_t cur = 0, l = 0;
      for (uint32_t c = b.m; c > 1; c = (c + 1) >> 1, l++) {
        for (uint32_t lane = 0; lane < b.m; lane++)
          if (merkle_aunt_lane(lane, l, c, lv[cur], h)) {
            merkle_store_node(dst[lane], h);
            dst[lane] += 8;
          }
        for (uint32_t lane = 0; lane < kMerkleB; lane++) merkle_level_lane(lane, c, lv[cur], lv[cur ^ 1]);
        cur ^= 1;
      }
      for (int k = 0; k < 8; k++) h[k] = lv[cur][k * kMerkleB];
      merkle_store_node(out.w() + 8 * (size_t)g, h);
    }
    nodes.assign(out.w(), out.w() + 8 * (size_t)wg_off[nt]);
  }
  if (n_pass > 1 && up_off.back() > 0) {
    sp.pref = flat.data();
    sp.aunt_off = R.aunt_off.data();
    sp.up_off = up_off.data();
    sp.up = up.w();
    sp.aunts = aunts.w();
    sp.n_trees = nt;
    sp.n_pass = n_pass;
    sp.n_leaves = nl;
    for (uint32_t g = 0; g < nl; g++) merkle_proof_spread_lane(sp, g);
  }
  R.roots = nodes;
  R.leaf_hashes.assign(lh.w(), lh.w() + 8 * (size_t)nl);
  R.aunts.assign(aunts.w(), aunts.w() + 8 * (size_t)R.aunt_off.back());
  return R;
}

struct ProofIn {
  int64_t total, index;
  uint8_t leaf_hash[32], root[32];
  std::vector<uint8_t> aunts, leaf;
};

struct Verdicts {
  std::vector<uint8_t> status;
  std::vector<uint32_t> out;
};

static Verdicts verify(const std::vector<ProofIn>& V, bool has_leaves, uint32_t leaf_kind, bool has_roots) {
  const uint32_t n = (uint32_t)V.size();
  std::vector<int64_t> total(n), index(n);
  std::vector<uint32_t> at(n), cnt(n), ridx(n), loff(n + 1, 0);
  size_t na = 0, lb = 0;
  for (uint32_t i = 0; i < n; i++) {
    total[i] = V[i].total;
    index[i] = V[i].index;
    cnt[i] = (uint32_t)(V[i].aunts.size() / 32);
    at[i] = (uint32_t)na;
    na += cnt[i] > kProofMaxAunts ? 0 : cnt[i];
    ridx[i] = i;
    lb += V[i].leaf.size();
    loff[i + 1] = (uint32_t)lb;
  }
  Nodes lh(n), aunts(na), roots(has_roots ? n : 0), out(n);
  std::vector<uint32_t> leaves((lb + 3) / 4 + (lb == 0));
  auto* lp = reinterpret_cast<uint8_t*>(leaves.data());
  for (uint32_t i = 0; i < n; i++) {
    memcpy(reinterpret_cast<uint8_t*>(lh.w()) + 32 * (size_t)i, V[i].leaf_hash, 32);
    if (cnt[i] && cnt[i] <= kProofMaxAunts)
      memcpy(reinterpret_cast<uint8_t*>(aunts.w()) + 32 * (size_t)at[i], V[i].aunts.data(), V[i].aunts.size());
    if (has_roots) memcpy(reinterpret_cast<uint8_t*>(roots.w()) + 32 * (size_t)i, V[i].root, 32);
    if (!V[i].leaf.empty()) memcpy(lp + loff[i], V[i].leaf.data(), V[i].leaf.size());
  }
  Verdicts R;
  R.status.assign(n, 0xEE);
  ProofBatch P{};
  P.total = total.data();
  P.index = index.data();
  P.leaf_hash = reinterpret_cast<const uint8_t*>(lh.w());
  P.aunt_at = at.data();
  P.aunt_cnt = cnt.data();
  P.aunts = reinterpret_cast<const uint8_t*>(aunts.w());
  P.roots = has_roots ? reinterpret_cast<const uint8_t*>(roots.w()) : nullptr;
  P.root_idx = ridx.data();
  P.leaves = lp;
  P.leaf_off = has_leaves ? loff.data() : nullptr;
  P.leaf_kind = leaf_kind;
  P.status = R.status.data();
  P.out_hash = out.w();
  for (uint32_t i = 0; i < n; i++) merkle_proof_verify_lane(P, i);
  R.out.assign(out.w(), out.w() + 8 * (size_t)n);
  return R;
}

// ------------------------------------------------------------------ bench
template <class F>
static int timed(const char* what, int reps, F f) {
  std::vector<double> ms;
  uint32_t acc = 0;
  for (int r = 0; r < reps; r++) {
    const auto t0 = std::chrono::steady_clock::now();
    acc ^= f();
    ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  std::sort(ms.begin(), ms.end());
  printf("{\"what\": \"%s\", \"reps\": %d, \"p50_ms\": %.6f, \"min_ms\": %.6f, \"check\": %u}\n", what, reps,
         ms[ms.size() / 2], ms[0], acc);
  return 0;
}

static int bench(int argc, char** argv) {
  if (argc != 8) return 2;
  const uint32_t kind = (uint32_t)atoi(argv[3]);
  const int reps = atoi(argv[7]);
  uint32_t x = 12345;
  auto fill = [&](std::vector<uint8_t>& v) {
    for (auto& b : v) b = (uint8_t)((x = x * 1664525u + 1013904223u) >> 24);
  };
  if (!strcmp(argv[2], "build")) {
    const uint32_t nt = (uint32_t)atoi(argv[4]), n = (uint32_t)atoi(argv[5]), len = (uint32_t)atoi(argv[6]);
    Trees T(nt, std::vector<std::vector<uint8_t>>(n, std::vector<uint8_t>(len)));
    for (auto& t : T)
      for (auto& it : t) fill(it);
    return timed("build", reps, [&] {
      const Built b = build(T, kind);
      return b.roots[0] ^ (b.aunts.empty() ? 0u : b.aunts.back());
    });
  }
  if (!strcmp(argv[2], "verify")) {
    const uint32_t n = (uint32_t)atoi(argv[4]), total = (uint32_t)atoi(argv[5]), len = (uint32_t)atoi(argv[6]);
    // one tree of `total` leaves; proof i is that of leaf i mod total
    Trees T(1, std::vector<std::vector<uint8_t>>(total, std::vector<uint8_t>(len)));
    for (auto& it : T[0]) fill(it);
    const Built b = build(T, kind);
    std::vector<ProofIn> V(n);
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t j = i % total;
      V[i].total = total;
      V[i].index = j;
      V[i].leaf = T[0][j];
      for (int k = 0; k < 8; k++) {
        const uint32_t lw = __builtin_bswap32(b.leaf_hashes[8 * (size_t)j + k]), rw = __builtin_bswap32(b.roots[k]);
        memcpy(V[i].leaf_hash + 4 * k, &lw, 4);
        memcpy(V[i].root + 4 * k, &rw, 4);
      }
      for (uint32_t a = b.aunt_off[j]; a < b.aunt_off[j + 1]; a++)
        for (int k = 0; k < 8; k++) {
          const uint32_t w = __builtin_bswap32(b.aunts[8 * (size_t)a + k]);
          V[i].aunts.insert(V[i].aunts.end(), reinterpret_cast<const uint8_t*>(&w),
                            reinterpret_cast<const uint8_t*>(&w) + 4);
        }
    }
    return timed("verify", reps, [&] {
      const Verdicts r = verify(V, true, kind, true);
      uint32_t bad = 0;
      for (uint8_t s : r.status) bad += s;
      return bad;
    });
  }
  return 2;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "bench")) return bench(argc, argv);
  const uint32_t count = get<uint32_t>();
  for (uint32_t r = 0; r < count; r++) {
    const uint32_t op = get<uint32_t>();
    if (op == 1) {
      const uint32_t kind = get<uint32_t>(), nt = get<uint32_t>();
      Trees T(nt);
      for (auto& t : T) {
        t.resize(get<uint32_t>());
        for (auto& it : t) {
          it.resize(get<uint32_t>());
          if (!rd(it.data(), it.size())) return 2;
        }
      }
      const Built b = build(T, kind);
      size_t g = 0;
      for (uint32_t t = 0; t < nt; t++) {
        emit(&b.roots[8 * (size_t)t]);
        for (size_t i = 0; i < T[t].size(); i++, g++) {
          emit(&b.leaf_hashes[8 * g]);
          const uint32_t k = b.aunt_off[g + 1] - b.aunt_off[g];
          fwrite(&k, 4, 1, stdout);
          for (uint32_t a = b.aunt_off[g]; a < b.aunt_off[g + 1]; a++) emit(&b.aunts[8 * (size_t)a]);
        }
      }
    } else if (op == 2) {
      const uint32_t n = get<uint32_t>(), has_leaves = get<uint32_t>(), leaf_kind = get<uint32_t>(),
                     has_roots = get<uint32_t>();
      std::vector<ProofIn> V(n);
      for (auto& p : V) {
        p.total = get<int64_t>();
        p.index = get<int64_t>();
        if (!rd(p.leaf_hash, 32)) return 2;
        p.aunts.resize(32 * (size_t)get<uint32_t>());
        if (!rd(p.aunts.data(), p.aunts.size())) return 2;
        if (has_roots && !rd(p.root, 32)) return 2;
        if (has_leaves) {
          p.leaf.resize(get<uint32_t>());
          if (!rd(p.leaf.data(), p.leaf.size())) return 2;
        }
      }
      const Verdicts v = verify(V, has_leaves != 0, leaf_kind, has_roots != 0);
      for (uint32_t i = 0; i < n; i++) {
        fwrite(&v.status[i], 1, 1, stdout);
        emit(&v.out[8 * (size_t)i]);
      }
    } else {
      fprintf(stderr, "unknown op %u\n", op);
      return 2;
    }
  }
  return 0;
}
