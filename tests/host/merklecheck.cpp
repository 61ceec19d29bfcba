// Host-side build of the merkle device code (cometbft_amd/csrc/merkle.h,
// sha256.h). Test infrastructure only: checks the kernel source without a GPU
// (tests/test_merkle_host.py, with -fsanitize=address,undefined), and times
// it on one CPU thread (tools/bench_merkle.py, -O2 without sanitizers).
//
// Default mode
//   input  (stdin):  u32 count, then records { u32 op, operands }
//   output (stdout): per record its digests, 32 bytes each
//     1 validator leaf   u32 key_type, u32 align, u32 klen, key, i64 power
//     2 CommitSig leaf   u32 flag, u8 addr[20], i64 seconds, i32 nanos, u32 align, u32 slen, sig
//     3 generic leaf     u32 align, u32 len, item
//     4 inner node       u8 left[32], u8 right[32]
//     5 trees            u32 n_trees, per tree { u32 n, per item { u32 len, item } }
//                        -> n_trees roots, by the kernel's pass structure
//                        emulated lane by lane (merkle_block_of, merkle_level_lane)
//   Every key, signature and item is read from a heap block of its own that
//   ends at the word holding its last byte, `align` bytes into it.
// argv[1] == "bench": bench <valset|commit> <n_trees> <n_leaves> <reps>
//   -> one JSON line, the p50 wall time of hashing the trees once
#define CMTV_HD inline
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../cometbft_amd/csrc/merkle.h"

using namespace cmtv;

static bool rd(void* p, size_t n) { return fread(p, 1, n, stdin) == n; }

template <class T>
static T get() {
  T v{};
  if (!rd(&v, sizeof v)) {
    fprintf(stderr, "short input\n");
    exit(2);
  }
  return v;
}

// len bytes from stdin in a block of their own, `align` bytes in
struct Bytes {
  uint8_t* base;
  uint8_t* p;
  Bytes(uint32_t align, uint32_t len) {
    base = static_cast<uint8_t*>(malloc((align + len + 3) / 4 * 4 + 4 * (align + len == 0)));
    p = base + align;
    if (len && !rd(p, len)) exit(2);
  }
  ~Bytes() { free(base); }
};

static void emit(const uint32_t h[8]) {
  uint8_t out[32];
  for (int i = 0; i < 8; i++) {
    const uint32_t be = __builtin_bswap32(h[i]);
    memcpy(out + 4 * i, &be, 4);
  }
  fwrite(out, 1, 32, stdout);
}

// The roots of n_trees trees of items, the way the kernels compute them
static void trees(const std::vector<std::vector<std::vector<uint8_t>>>& T) {
  const uint32_t nt = (uint32_t)T.size();
  std::vector<const std::vector<uint8_t>*> items;
  std::vector<uint32_t> leaf_off(nt + 1, 0);
  for (uint32_t t = 0; t < nt; t++) {
    for (const auto& it : T[t]) items.push_back(&it);
    leaf_off[t + 1] = (uint32_t)items.size();
  }
  std::vector<uint32_t> nodes;  // the previous pass's output
  for (bool first = true;; first = false) {
    std::vector<uint32_t> wg_off(nt + 1, 0);
    for (uint32_t t = 0; t < nt; t++) wg_off[t + 1] = wg_off[t] + merkle_blocks(leaf_off[t + 1] - leaf_off[t]);
    std::vector<uint32_t> out(8 * (size_t)wg_off[nt]);
    alignas(16) static uint32_t lv[2][8 * kMerkleB];
    for (uint32_t g = 0; g < wg_off[nt]; g++) {
      const MerkleBlock b = merkle_block_of(g, wg_off.data(), leaf_off.data(), nt);
      uint32_t h[8];
      if (b.m == 0) {
        merkle_empty(h);
        memcpy(&out[8 * (size_t)g], h, 32);
        continue;
      }
      for (uint32_t lane = 0; lane < b.m; lane++) {
        if (first) {
          const auto& it = *items[b.first + lane];
          // a copy that ends at the item's last word, at a varying alignment
          const uint32_t al = (b.first + lane) & 3, len = (uint32_t)it.size();
          std::vector<uint32_t> buf((al + len + 3) / 4 + 1);
          uint8_t* p = reinterpret_cast<uint8_t*>(buf.data()) + al;
          if (len) memcpy(p, it.data(), len);
          merkle_leaf_hash(h, p, len);
        } else {
          memcpy(h, &nodes[8 * (size_t)(b.first + lane)], 32);
        }
        for (int k = 0; k < 8; k++) lv[0][k * kMerkleB + lane] = h[k];
      }
      uint32_t cur = 0;
      for (uint32_t c = b.m; c > 1; c = (c + 1) >> 1) {
        for (uint32_t lane = 0; lane < kMerkleB; lane++) merkle_level_lane(lane, c, lv[cur], lv[cur ^ 1]);
        cur ^= 1;
      }
      for (int k = 0; k < 8; k++) out[8 * (size_t)g + k] = lv[cur][k * kMerkleB];
    }
    nodes.swap(out);
    if (wg_off[nt] == nt) break;
    leaf_off = wg_off;
  }
  for (uint32_t t = 0; t < nt; t++) emit(&nodes[8 * (size_t)t]);
}

// ------------------------------------------------------------------ bench
// n nodes (8 words each) reduced in place, level by level
static void reduce(std::vector<uint32_t>& v, uint32_t n, uint32_t out[8]) {
  if (n == 0) {
    merkle_empty(out);
    return;
  }
  for (uint32_t c = n; c > 1; c = (c + 1) >> 1) {
    for (uint32_t i = 0; i < c / 2; i++) {
      uint32_t h[8];
      merkle_inner_hash(h, &v[16 * (size_t)i]);
      memcpy(&v[8 * (size_t)i], h, 32);
    }
    if (c & 1) memmove(&v[8 * (size_t)(c / 2)], &v[8 * (size_t)(c - 1)], 32);
  }
  memcpy(out, v.data(), 32);
}

static int bench(int argc, char** argv) {
  if (argc != 6) return 2;
  const bool commit = !strcmp(argv[2], "commit");
  const uint32_t nt = (uint32_t)atoi(argv[3]), n = (uint32_t)atoi(argv[4]);
  const int reps = atoi(argv[5]);
  // one tree's fields, shared by every tree of the call (the time is the hashing's)
  std::vector<uint32_t> key(16 * (size_t)n), sig(16 * (size_t)n), addr(5 * (size_t)n);
  uint32_t x = 12345;
  for (auto* a : {&key, &sig, &addr})
    for (auto& w : *a) w = x = x * 1664525u + 1013904223u;
  std::vector<uint32_t> v(8 * (size_t)std::max(n, 1u));
  std::vector<double> ms;
  uint32_t acc = 0;
  for (int r = 0; r < reps; r++) {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t t = 0; t < nt; t++) {
      for (uint32_t i = 0; i < n; i++) {
        uint32_t w[32], nb;
        if (commit)
          nb = merkle_commit_sig_leaf(w, 2, &addr[5 * (size_t)i], 1700000000 + i + t, 123456789, &sig[16 * (size_t)i], 64);
        else
          nb = merkle_validator_leaf(w, &key[16 * (size_t)i], 32, kMerkleKeyEd25519, 1000 + i + t);
        sha256_blocks(&v[8 * (size_t)i], w, nb);
      }
      uint32_t h[8];
      reduce(v, n, h);
      acc ^= h[0];
    }
    ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  std::sort(ms.begin(), ms.end());
  printf("{\"kind\": \"%s\", \"n_trees\": %u, \"n_leaves\": %u, \"reps\": %d, \"p50_ms\": %.6f, \"min_ms\": %.6f, \"check\": %u}\n",
         argv[2], nt, n, reps, ms[ms.size() / 2], ms[0], acc);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "bench")) return bench(argc, argv);
  const uint32_t count = get<uint32_t>();
  for (uint32_t r = 0; r < count; r++) {
    const uint32_t op = get<uint32_t>();
    uint32_t h[8], w[32];
    if (op == 1) {
      const uint32_t kt = get<uint32_t>(), al = get<uint32_t>(), klen = get<uint32_t>();
      Bytes key(al, klen);
      const int64_t power = get<int64_t>();
      uint32_t kw[16];
      load_be_words<16>(kw, key.p, klen);
      const uint32_t nb = merkle_validator_leaf(w, kw, klen, kt, power);
      sha256_blocks(h, w, nb);
      emit(h);
    } else if (op == 2) {
      const uint32_t flag = get<uint32_t>();
      uint8_t a[20];
      if (!rd(a, 20)) return 2;
      const int64_t sec = get<int64_t>();
      const int32_t nanos = get<int32_t>();
      const uint32_t al = get<uint32_t>(), slen = get<uint32_t>();
      Bytes sig(al, slen);
      uint32_t addr[5], sw[16];
      for (int k = 0; k < 5; k++) {
        memcpy(&addr[k], a + 4 * k, 4);
        addr[k] = __builtin_bswap32(addr[k]);
      }
      load_be_words<16>(sw, sig.p, slen);
      const uint32_t nb = merkle_commit_sig_leaf(w, flag, addr, sec, nanos, sw, slen);
      sha256_blocks(h, w, nb);
      emit(h);
    } else if (op == 3) {
      const uint32_t al = get<uint32_t>(), len = get<uint32_t>();
      Bytes item(al, len);
      merkle_leaf_hash(h, item.p, len);
      emit(h);
    } else if (op == 4) {
      uint8_t b[64];
      if (!rd(b, 64)) return 2;
      uint32_t n[16];
      for (int k = 0; k < 16; k++) {
        memcpy(&n[k], b + 4 * k, 4);
        n[k] = __builtin_bswap32(n[k]);
      }
      merkle_inner_hash(h, n);
      emit(h);
    } else if (op == 5) {
      const uint32_t nt = get<uint32_t>();
      std::vector<std::vector<std::vector<uint8_t>>> T(nt);
      for (auto& t : T) {
        t.resize(get<uint32_t>());
        for (auto& it : t) {
          it.resize(get<uint32_t>());
          if (!it.empty() && !rd(it.data(), it.size())) return 2;
        }
      }
      trees(T);
    } else {
      fprintf(stderr, "unknown op %u\n", op);
      return 2;
    }
  }
  return 0;
}
