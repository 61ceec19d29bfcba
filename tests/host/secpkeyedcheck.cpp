// Host-side build of the registered-key secp256k1 device code
// (cometbft_amd/csrc/secp256k1.h: secp_qcomb_position, secp_verify_keyed_one)
// with operand-bound assertions on. Test infrastructure only: checks the
// kernel source without a GPU.
//
// Input (stdin), both modes:
//   u32 n_keys, then n_keys x u8 pk[33]: the keys, registered in this order
//   (their tables built position by position with secp_qcomb_position, as
//   k_secp_qcomb_build does with one thread per (key, position))
// Default mode
//   input:  u32 n, then n x { u32 key_idx, u8 sig[64], u32 mlen, u8 msg[mlen] }
//   output: n_keys ok bytes, then n verdict bytes (secp_verify_keyed_one over
//           the key's table and the fixed table built by secp_gtab_row)
// argv[1] == "rows"
//   input:  u32 count, then count x { u32 key, u32 j, u32 d }
//   output: n_keys ok bytes; n_keys bytes, 1 when every word of the key's
//           table is that of the point at infinity (0 : 1 : 0) literally;
//           then per record X, Y, Z mod p as eight little-endian words each
#define CMTV_HD inline
#define CMTV_BOUNDS_CHECK 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../cometbft_amd/csrc/secp256k1.h"

using namespace cmtv;

constexpr size_t kTabWords = (size_t)SECP_GTAB_ENTRIES * SECP_GTAB_ROW_WORDS;

// rows of one table in the kernels' layout
struct HostTab {
  const uint32_t* rows;
  void load(int row, pt256& p) const {
    const uint32_t* q = rows + (size_t)row * SECP_GTAB_ROW_WORDS;
    for (int i = 0; i < 10; i++) {
      p.X.v[i] = q[i];
      p.Y.v[i] = q[10 + i];
      p.Z.v[i] = q[20 + i];
    }
  }
};

static bool rd(void* p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }

static void put_fp(fp a) {
  uint32_t w[8];
  fp_normalize(a);
  fp_to_words(w, a);
  fwrite(w, 4, 8, stdout);
}

int main(int argc, char** argv) {
  const bool rows_mode = argc > 1 && !strcmp(argv[1], "rows");
  uint32_t n_keys;
  if (!rd(&n_keys, 4) || n_keys == 0 || n_keys > 4096) return 1;
  std::vector<uint8_t> pk(33 * (size_t)n_keys), ok(n_keys);
  if (!rd(pk.data(), pk.size())) return 1;
  std::vector<uint32_t> tab(n_keys * kTabWords, 0xFFFFFFFFu);
  for (uint32_t k = 0; k < n_keys; k++)
    for (int j = 0; j < SECP_GTAB_POS; j++) {
      uint32_t* rows = &tab[k * kTabWords + (size_t)j * SECP_GTAB_PER_POS * SECP_GTAB_ROW_WORDS];
      const bool v = secp_qcomb_position(rows, &pk[33 * (size_t)k], j);
      if (j == 0) ok[k] = v ? 1 : 0;
    }
  fwrite(ok.data(), 1, n_keys, stdout);

  if (rows_mode) {
    for (uint32_t k = 0; k < n_keys; k++) {
      uint8_t inf = 1;
      for (size_t r = 0; r < (size_t)SECP_GTAB_ENTRIES; r++)
        for (int w = 0; w < SECP_GTAB_ROW_WORDS; w++)
          if (tab[k * kTabWords + r * SECP_GTAB_ROW_WORDS + w] != (w == 10 ? 1u : 0u)) inf = 0;
      fwrite(&inf, 1, 1, stdout);
    }
    uint32_t count;
    if (!rd(&count, 4)) return 1;
    for (uint32_t c = 0; c < count; c++) {
      uint32_t k, j, d;
      if (!rd(&k, 4) || !rd(&j, 4) || !rd(&d, 4)) return 1;
      if (k >= n_keys || j >= (uint32_t)SECP_GTAB_POS || d < 1 || d > (uint32_t)SECP_GTAB_PER_POS) return 3;
      pt256 p;
      HostTab{&tab[k * kTabWords]}.load((int)(j * SECP_GTAB_PER_POS + d - 1), p);
      put_fp(p.X);
      put_fp(p.Y);
      put_fp(p.Z);
    }
    return 0;
  }

  std::vector<uint32_t> gtab(kTabWords);
  for (int j = 0; j < SECP_GTAB_POS; j++)
    for (int d = 1; d <= SECP_GTAB_PER_POS; d++)
      secp_gtab_row(&gtab[(size_t)(j * SECP_GTAB_PER_POS + d - 1) * SECP_GTAB_ROW_WORDS], j, d);
  const HostTab gt{gtab.data()};
  uint32_t n;
  if (!rd(&n, 4)) return 1;
  for (uint32_t i = 0; i < n; i++) {
    uint8_t sig[64];
    uint32_t k, mlen;
    if (!rd(&k, 4) || !rd(sig, 64) || !rd(&mlen, 4)) return 1;
    if (k >= n_keys) return 3;
    // the message at an odd offset inside a word-aligned buffer
    std::vector<uint32_t> buf((mlen + 16) / 4 + 2, 0);
    uint8_t* msg = reinterpret_cast<uint8_t*>(buf.data()) + 1 + (i % 3);
    if (!rd(msg, mlen)) return 1;
    const HostTab qt{&tab[k * kTabWords]};
    const uint8_t v = secp_verify_keyed_one(ok[k] != 0, sig, msg, mlen, qt, gt) ? 1 : 0;
    fwrite(&v, 1, 1, stdout);
  }
  return 0;
}
