// Host-side build of the secp256k1 device code (cometbft_amd/csrc/secp256k1.h,
// fp256k1.h, sc256k1.h, sha256.h) with operand-bound assertions on. Test
// infrastructure only: checks the kernel source without a GPU.
//
// Default mode
//   input  (stdin):  u32 n, then n x { u8 pk[33], u8 sig[64], u32 mlen, u8 msg[mlen] }
//   output (stdout): n bytes of verdicts (secp_verify_one, the kernel's
//                    per-signature function, over the fixed table built by
//                    secp_gtab_row as the runtime builds it)
// argv[1] == "prim": primitives
//   input:  u32 count, then records { u32 op, operands }
//   output: per record its result, 256-bit values as eight little-endian words
//     1 fp_mul   a[10] b[10] limbs            -> a b mod p
//     2 fp_sq    a[10]                        -> a^2 mod p
//     3 fp_sub   a[10] b[10] u32 mb           -> a - b mod p
//     4 fp_normalize a[10]                    -> a mod p
//     5 fp_sqrt_candidate a[10]               -> a^((p+1)/4) mod p
//     6 scalar load-reduce  u8 be[32]         -> value mod n
//     7 scn_mul   u8 a[32] u8 b[32]           -> a b mod n
//     8 scn_invert u8 a[32]                   -> 1/a mod n
//     9 sha256   u32 len, bytes               -> digest (big-endian words reversed into one integer)
//    10 gtab row u32 j, u32 d                 -> X, Y, Z mod p (three values)
#define CMTV_HD inline
#define CMTV_BOUNDS_CHECK 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../cometbft_amd/csrc/secp256k1.h"

using namespace cmtv;

struct HostQTab {
  pt256 t[SECP_QTAB_ENTRIES];
  void store(int e, const pt256& p) { t[e] = p; }
  void load(int e, pt256& p) const { p = t[e]; }
};

struct HostGTab {
  std::vector<uint32_t> rows;
  HostGTab() : rows((size_t)SECP_GTAB_ENTRIES * SECP_GTAB_ROW_WORDS) {
    for (int j = 0; j < SECP_GTAB_POS; j++)
      for (int d = 1; d <= SECP_GTAB_PER_POS; d++)
        secp_gtab_row(&rows[(size_t)(j * SECP_GTAB_PER_POS + d - 1) * SECP_GTAB_ROW_WORDS], j, d);
  }
  void load(int row, pt256& p) const {
    const uint32_t* q = &rows[(size_t)row * SECP_GTAB_ROW_WORDS];
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

static int primitives() {
  uint32_t count;
  if (!rd(&count, 4)) return 1;
  for (uint32_t c = 0; c < count; c++) {
    uint32_t op;
    if (!rd(&op, 4)) return 1;
    fp a, b, r;
    uint8_t ba[32], bb[32];
    uint32_t w[8];
    scn x, y, z;
    switch (op) {
      case 1:
        if (!rd(a.v, 40) || !rd(b.v, 40)) return 1;
        fp_mul(r, a, b);
        if (!fp_within(r, 1)) return 2;
        put_fp(r);
        break;
      case 2:
        if (!rd(a.v, 40)) return 1;
        fp_sq(r, a);
        if (!fp_within(r, 1)) return 2;
        put_fp(r);
        break;
      case 3: {
        uint32_t mb;
        if (!rd(a.v, 40) || !rd(b.v, 40) || !rd(&mb, 4)) return 1;
        fp_sub(r, a, b, mb);
        put_fp(r);
        break;
      }
      case 4:
        if (!rd(a.v, 40)) return 1;
        put_fp(a);
        break;
      case 5:
        if (!rd(a.v, 40)) return 1;
        fp_sqrt_candidate(r, a);
        put_fp(r);
        break;
      case 6:
        if (!rd(ba, 32)) return 1;
        words_from_be32(w, ba);
        scn_from_words(x, w);
        fwrite(x.v, 4, 8, stdout);
        break;
      case 7:
        if (!rd(ba, 32) || !rd(bb, 32)) return 1;
        words_from_be32(w, ba);
        scn_from_words(x, w);
        words_from_be32(w, bb);
        scn_from_words(y, w);
        scn_mul(z, x, y);
        fwrite(z.v, 4, 8, stdout);
        break;
      case 8:
        if (!rd(ba, 32)) return 1;
        words_from_be32(w, ba);
        scn_from_words(x, w);
        scn_invert(z, x);
        fwrite(z.v, 4, 8, stdout);
        break;
      case 9: {
        uint32_t len;
        if (!rd(&len, 4)) return 1;
        // the message at an odd offset inside a word-aligned buffer
        std::vector<uint32_t> buf((len + 16) / 4 + 2, 0);
        uint8_t* m = reinterpret_cast<uint8_t*>(buf.data()) + 1 + (c % 3);
        if (!rd(m, len)) return 1;
        uint32_t h[8], o[8];
        sha256_msg(h, m, len);
        for (int i = 0; i < 8; i++) o[i] = h[7 - i];
        fwrite(o, 4, 8, stdout);
        break;
      }
      case 10: {
        uint32_t j, d, row[SECP_GTAB_ROW_WORDS];
        if (!rd(&j, 4) || !rd(&d, 4)) return 1;
        secp_gtab_row(row, (int)j, (int)d);
        for (int k = 0; k < 3; k++) {
          memcpy(a.v, row + 10 * k, 40);
          put_fp(a);
        }
        break;
      }
      default:
        return 3;
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "prim")) return primitives();
  HostGTab gt;
  uint32_t n;
  if (!rd(&n, 4)) return 1;
  for (uint32_t i = 0; i < n; i++) {
    uint8_t pk[33], sig[64];
    uint32_t mlen;
    if (!rd(pk, 33) || !rd(sig, 64) || !rd(&mlen, 4)) return 1;
    std::vector<uint32_t> buf((mlen + 16) / 4 + 2, 0);
    uint8_t* msg = reinterpret_cast<uint8_t*>(buf.data()) + 1 + (i % 3);
    if (!rd(msg, mlen)) return 1;
    HostQTab qt;
    const uint8_t v = secp_verify_one(pk, sig, msg, mlen, qt, gt) ? 1 : 0;
    fwrite(&v, 1, 1, stdout);
  }
  return 0;
}
