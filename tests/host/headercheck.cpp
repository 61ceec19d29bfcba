// Host-side build of the header device code (cometbft_amd/csrc/header.h,
// merkle.h, sha256.h). Test infrastructure only: checks the kernel source
// without a GPU (tests/test_header_host.py, with -fsanitize=address,undefined),
// and times it on one CPU thread (tools/bench_header.py, -O2 without
// sanitizers).
//
// Default mode
//   input  (stdin):  u32 count, then records { u32 op, operands }
//   output (stdout): per record its digests, 32 bytes each
//     1 bytes leaf       u32 align, u32 len, bytes
//     2 varints leaf     u64 a, u64 b
//     3 block id leaf    u32 align, u32 hlen, hash, u32 total, u32 align, u32 plen, part hash
//     4 headers          u32 n, per header { u64 version.block, u64 version.app, u32 len, chain id,
//                        i64 height, i64 seconds, i32 nanos, u32 len, id hash, u32 total,
//                        u32 len, id part hash, 9 x { u32 len, bytes } }
//                        -> n roots, by k_header_hash's structure: the fields staged
//                        as struct-of-arrays, waves of 64 lanes, 16 lanes a header,
//                        the reduction emulated lane by lane with the host form of
//                        the row move
//     5 transaction leaf u32 align, u32 len, tx
//   Every byte string of ops 1, 3 and 5 is read from a heap block of its own
//   that ends at the word holding its last byte, `align` bytes into it.
// argv[1] == "bench": bench header <n> <reps> | bench txs <n_blocks> <n_txs> <tx_len> <reps>
//   -> one JSON line, the p50 wall time of hashing them once
#define CMTV_HD inline
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../cometbft_amd/csrc/header.h"

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

// The group policy of header.h on the host: a snapshot of the wave's 64 nodes
// before the level; lane i reads lane i + S of its row of 16, zero when there
// is none (DPP row_shl with bound_ctrl)
struct HostGroup {
  const uint32_t (*snap)[8];
  uint32_t lane;  // in the wave
  template <int S>
  void down(uint32_t out[8], const uint32_t in[8]) const {
    if (memcmp(in, snap[lane], 32)) {
      fprintf(stderr, "lane %u moves a value that is not its node\n", lane);
      exit(3);
    }
    const uint32_t row = lane & ~15u, src = (lane & 15u) + S;
    for (int k = 0; k < 8; k++) out[k] = src < 16 ? snap[row + src][k] : 0u;
  }
};

template <int S>
static void wave_level(uint32_t d[64][8], uint32_t c) {
  uint32_t snap[64][8];
  memcpy(snap, d, sizeof snap);
  for (uint32_t l = 0; l < 64; l++) header_level<S>(HostGroup{snap, l}, l % kHeaderGroup, c, d[l]);
}

// The staged fields of n headers (kernels.h launch_header_hash)
struct Staged {
  std::vector<uint32_t> off, u32;
  std::vector<uint64_t> u64;
  std::vector<uint8_t> var;
  uint32_t n;
  uint32_t* var_block = nullptr;
  explicit Staged(uint32_t n_) : off(1, 0u), u32(kHeaderU32Fields * (size_t)n_), u64(kHeaderU64Fields * (size_t)n_), n(n_) {}
  ~Staged() { free(var_block); }
  void bytes(const void* p, uint32_t len) {
    const auto* q = static_cast<const uint8_t*>(p);
    var.insert(var.end(), q, q + len);
    off.push_back((uint32_t)var.size());
  }
  // the variable bytes in a block that ends four bytes past them, as a run stages them
  HeaderFields fields() {
    free(var_block);
    var_block = static_cast<uint32_t*>(calloc(1, var.size() + 4));
    if (!var.empty()) memcpy(var_block, var.data(), var.size());
    return HeaderFields{reinterpret_cast<const uint8_t*>(var_block), off.data(), u64.data(), u32.data(), n};
  }
};

// roots of the staged headers into out (8 words each), wave by wave as the kernel runs
static void hash_staged(const HeaderFields& F, std::vector<uint32_t>& out) {
  out.assign(8 * (size_t)F.n, 0u);
  const uint32_t per_wave = 64 / kHeaderGroup;
  for (uint32_t h0 = 0; h0 < F.n; h0 += per_wave) {
    uint32_t d[64][8];
    for (uint32_t l = 0; l < 64; l++) {
      const uint32_t h = h0 + l / kHeaderGroup, lane = l % kHeaderGroup;
      uint32_t w[32], nb = 1;
      if (h < F.n && lane < kHeaderLeaves)
        nb = header_leaf(w, F, h, lane);
      else
        memset(w, 0, sizeof w);
      sha256_blocks(d[l], w, nb);
    }
    wave_level<1>(d, 14);
    wave_level<2>(d, 7);
    wave_level<4>(d, 4);
    wave_level<8>(d, 2);
    for (uint32_t g = 0; g < per_wave && h0 + g < F.n; g++) memcpy(&out[8 * (size_t)(h0 + g)], d[g * kHeaderGroup], 32);
  }
}

static std::vector<uint8_t> get_bytes() {
  std::vector<uint8_t> b(get<uint32_t>());
  if (!b.empty() && !rd(b.data(), b.size())) exit(2);
  return b;
}

static void headers() {
  const uint32_t n = get<uint32_t>();
  Staged S(n);
  for (uint32_t h = 0; h < n; h++) {
    S.u64[kHeaderVersionBlock * (size_t)n + h] = get<uint64_t>();
    S.u64[kHeaderVersionApp * (size_t)n + h] = get<uint64_t>();
    const auto cid = get_bytes();
    S.u64[kHeaderHeight * (size_t)n + h] = (uint64_t)get<int64_t>();
    S.u64[kHeaderSeconds * (size_t)n + h] = (uint64_t)get<int64_t>();
    S.u32[kHeaderNanos * (size_t)n + h] = (uint32_t)get<int32_t>();
    const auto idh = get_bytes();
    S.u32[kHeaderIdTotal * (size_t)n + h] = get<uint32_t>();
    const auto idp = get_bytes();
    // (bytes() pushes each field's end, which is the next one's start)
    S.bytes(cid.data(), (uint32_t)cid.size());
    S.bytes(idh.data(), (uint32_t)idh.size());
    S.bytes(idp.data(), (uint32_t)idp.size());
    for (int f = 0; f < 9; f++) {
      const auto b = get_bytes();
      S.bytes(b.data(), (uint32_t)b.size());
    }
  }
  std::vector<uint32_t> out;
  hash_staged(S.fields(), out);
  for (uint32_t h = 0; h < n; h++) emit(&out[8 * (size_t)h]);
}

// ------------------------------------------------------------------ bench
static double p50(std::vector<double>& ms) {
  std::sort(ms.begin(), ms.end());
  return ms[ms.size() / 2];
}

// n headers of 32-byte hashes, a 20-byte proposer address and a 15-character
// chain id, leaf by leaf and level by level as a CPU would (no idle lanes)
static int bench_header(uint32_t n, int reps) {
  Staged S(n);
  uint32_t x = 12345;
  for (uint32_t h = 0; h < n; h++) {
    S.u64[kHeaderVersionBlock * (size_t)n + h] = 11;
    S.u64[kHeaderVersionApp * (size_t)n + h] = 1;
    S.u64[kHeaderHeight * (size_t)n + h] = 1000000 + h;
    S.u64[kHeaderSeconds * (size_t)n + h] = 1700000000 + h;
    S.u32[kHeaderNanos * (size_t)n + h] = 123456789;
    S.u32[kHeaderIdTotal * (size_t)n + h] = 1;
    uint32_t b[8];
    const uint32_t lens[12] = {15, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 20};
    for (uint32_t len : lens) {
      for (auto& w : b) w = x = x * 1664525u + 1013904223u;
      S.bytes(b, len);
    }
  }
  const HeaderFields F = S.fields();
  std::vector<double> ms;
  uint32_t acc = 0;
  for (int r = 0; r < reps; r++) {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t h = 0; h < n; h++) {
      uint32_t v[16][8];
      for (uint32_t leaf = 0; leaf < kHeaderLeaves; leaf++) {
        uint32_t w[32];
        const uint32_t nb = header_leaf(w, F, h, leaf);
        sha256_blocks(v[leaf], w, nb);
      }
      for (uint32_t c = kHeaderLeaves; c > 1; c = (c + 1) >> 1) {
        for (uint32_t i = 0; i < c / 2; i++) {
          uint32_t nn[16], o[8];
          memcpy(nn, v[2 * i], 32);
          memcpy(nn + 8, v[2 * i + 1], 32);
          merkle_inner_hash(o, nn);
          memcpy(v[i], o, 32);
        }
        if (c & 1) memcpy(v[c / 2], v[c - 1], 32);
      }
      acc ^= v[0][0];
    }
    ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  const double mid = p50(ms);
  printf("{\"kind\": \"header\", \"n\": %u, \"reps\": %d, \"p50_ms\": %.6f, \"min_ms\": %.6f, \"check\": %u}\n", n, reps, mid,
         ms[0], acc);
  return 0;
}

static int bench_txs(uint32_t n_blocks, uint32_t n_txs, uint32_t tx_len, int reps) {
  std::vector<uint32_t> tx((tx_len + 3) / 4 + 1);
  uint32_t x = 777;
  for (auto& w : tx) w = x = x * 1664525u + 1013904223u;
  std::vector<uint32_t> v(8 * (size_t)std::max(n_txs, 1u));
  std::vector<double> ms;
  uint32_t acc = 0;
  for (int r = 0; r < reps; r++) {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t b = 0; b < n_blocks; b++) {
      tx[0] = b;  // (the time is the hashing's: one buffer, its first word changing)
      for (uint32_t i = 0; i < n_txs; i++) merkle_tx_leaf_hash(&v[8 * (size_t)i], reinterpret_cast<const uint8_t*>(tx.data()), tx_len);
      for (uint32_t c = n_txs; c > 1; c = (c + 1) >> 1) {
        for (uint32_t i = 0; i < c / 2; i++) {
          uint32_t o[8];
          merkle_inner_hash(o, &v[16 * (size_t)i]);
          memcpy(&v[8 * (size_t)i], o, 32);
        }
        if (c & 1) memmove(&v[8 * (size_t)(c / 2)], &v[8 * (size_t)(c - 1)], 32);
      }
      acc ^= v[0];
    }
    ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  const double mid = p50(ms);
  printf("{\"kind\": \"txs\", \"n_blocks\": %u, \"n_txs\": %u, \"tx_len\": %u, \"reps\": %d, \"p50_ms\": %.6f, \"min_ms\": %.6f, \"check\": %u}\n",
         n_blocks, n_txs, tx_len, reps, mid, ms[0], acc);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "bench")) {
    if (argc == 5 && !strcmp(argv[2], "header")) return bench_header((uint32_t)atoi(argv[3]), atoi(argv[4]));
    if (argc == 7 && !strcmp(argv[2], "txs"))
      return bench_txs((uint32_t)atoi(argv[3]), (uint32_t)atoi(argv[4]), (uint32_t)atoi(argv[5]), atoi(argv[6]));
    return 2;
  }
  const uint32_t count = get<uint32_t>();
  for (uint32_t r = 0; r < count; r++) {
    const uint32_t op = get<uint32_t>();
    uint32_t h[8], w[32];
    if (op == 1) {
      const uint32_t al = get<uint32_t>(), len = get<uint32_t>();
      Bytes b(al, len);
      uint32_t fw[16];
      load_be_words<16>(fw, b.p, len);
      const uint32_t nb = header_bytes_leaf(w, fw, len);
      sha256_blocks(h, w, nb);
      emit(h);
    } else if (op == 2) {
      const uint64_t a = get<uint64_t>(), b = get<uint64_t>();
      const uint32_t nb = header_varints_leaf(w, a, b);
      sha256_blocks(h, w, nb);
      emit(h);
    } else if (op == 3) {
      const uint32_t al = get<uint32_t>(), hlen = get<uint32_t>();
      Bytes hash(al, hlen);
      const uint32_t total = get<uint32_t>(), al2 = get<uint32_t>(), plen = get<uint32_t>();
      Bytes part(al2, plen);
      uint32_t hw[8], pw[8];
      load_be_words<8>(hw, hash.p, hlen);
      load_be_words<8>(pw, part.p, plen);
      const uint32_t nb = header_block_id_leaf(w, hw, hlen, total, pw, plen);
      sha256_blocks(h, w, nb);
      emit(h);
    } else if (op == 4) {
      headers();
    } else if (op == 5) {
      const uint32_t al = get<uint32_t>(), len = get<uint32_t>();
      Bytes tx(al, len);
      merkle_tx_leaf_hash(h, tx.p, len);
      emit(h);
    } else {
      fprintf(stderr, "unknown op %u\n", op);
      return 2;
    }
  }
  return 0;
}
