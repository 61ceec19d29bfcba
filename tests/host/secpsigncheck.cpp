// Host-side build of the secp256k1 signing code (cometbft_amd/csrc/
// secp256k1_sign.h and what it stands on) with operand-bound assertions on,
// built with AddressSanitizer and UBSan by tests/test_secp256k1_sign_host.py.
// Test infrastructure only: checks the kernel source without a GPU.
//
// argv[1] == "sign": whole signatures (secp_sign_one, the kernel's per-lane function)
//   input  (stdin):  u32 n, then n x { u8 priv[32], u32 mlen, u8 msg[mlen] }
//   output (stdout): n x { u8 ok, u8 sig[64] }
// argv[1] == "pub": public keys and addresses (secp_pubkey_one)
//   input:  u32 n, then n x u8 priv[32]
//   output: n x { u8 pk[33], u8 addr[20] }
// argv[1] == "prim": primitives
//   input:  u32 count, then records { u32 op, operands }; 32-byte values big-endian
//   output: per record its result
//     1 hmac_sha256_32  u32 len (32, 33, 97), u8 key[32], u8 data[len]   -> u8[32]
//     2 nonce generator u8 d[32], u8 h[32], u32 steps, u8 retry[steps]   -> steps x { cand[32], K[32], V[32] }
//     3 candidate       u8 v[32]                                         -> u8 accepted
//     4 x -> r          u8 x[32] (x < p)                                 -> u8 r[32]
//     5 sign_with_nonce u8 d[32], u8 e[32], u8 k[32] (k not reduced)     -> u8 ok, u8 sig[64]
//     6 fp_invert       u32 limbs[10]                                    -> u8[32] (1 / a mod p)
//     7 ripemd160_33    u8 digest[32]                                    -> u8[20]
//     8 key in range    u8 priv[32]                                      -> u8
//     9 key from digest u8 c[32]                                         -> u8 priv[32]
#define CMTV_HD inline
#define CMTV_BOUNDS_CHECK 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "../../cometbft_amd/csrc/secp256k1_sign.h"

using namespace cmtv;

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

static const HostGTab& gtab() {
  static std::unique_ptr<HostGTab> g;
  if (!g) g.reset(new HostGTab);
  return *g;
}

static bool rd(void* p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }

// big-endian words <-> bytes
static void be_words(uint32_t* w, const uint8_t* b, int nwords) {
  for (int i = 0; i < nwords; i++)
    w[i] = ((uint32_t)b[4 * i] << 24) | ((uint32_t)b[4 * i + 1] << 16) | ((uint32_t)b[4 * i + 2] << 8) | b[4 * i + 3];
}
static void put_be(const uint32_t* w, int nwords) {
  for (int i = 0; i < nwords; i++) {
    const uint8_t b[4] = {(uint8_t)(w[i] >> 24), (uint8_t)(w[i] >> 16), (uint8_t)(w[i] >> 8), (uint8_t)w[i]};
    fwrite(b, 1, 4, stdout);
  }
}
// 32 big-endian bytes as a scalar's words, not reduced
static void raw_scalar(scn& s, const uint8_t* b) { words_from_be32(s.v, b); }
static void put_scalar(const scn& s) {
  uint32_t w[8];
  for (int i = 0; i < 8; i++) w[i] = s.v[7 - i];
  put_be(w, 8);
}

static int primitives() {
  uint32_t count;
  if (!rd(&count, 4)) return 1;
  for (uint32_t c = 0; c < count; c++) {
    uint32_t op;
    if (!rd(&op, 4)) return 1;
    uint8_t a[32], b[32], k[32];
    switch (op) {
      case 1: {
        uint32_t len;
        uint8_t data[100] = {0};
        if (!rd(&len, 4) || (len != 32 && len != 33 && len != 97) || !rd(a, 32) || !rd(data, len)) return 1;
        uint32_t kw[8], dw[25], out[8];
        be_words(kw, a, 8);
        be_words(dw, data, 25);
        if (len == 32) hmac_sha256_32<32>(out, kw, dw);
        if (len == 33) hmac_sha256_32<33>(out, kw, dw);
        if (len == 97) hmac_sha256_32<97>(out, kw, dw);
        put_be(out, 8);
        break;
      }
      case 2: {
        uint32_t steps;
        if (!rd(a, 32) || !rd(b, 32) || !rd(&steps, 4)) return 1;
        uint32_t x[8], h[8], cand[8];
        be_words(x, a, 8);
        be_words(h, b, 8);
        Rfc6979 g;
        rfc6979_init(g, x, h);
        for (uint32_t s = 0; s < steps; s++) {
          uint8_t retry;
          if (!rd(&retry, 1)) return 1;
          rfc6979_next(g, cand, retry != 0);
          put_be(cand, 8);
          put_be(g.K, 8);
          put_be(g.V, 8);
        }
        break;
      }
      case 3: {
        if (!rd(a, 32)) return 1;
        uint32_t cand[8];
        be_words(cand, a, 8);
        scn kk;
        const uint8_t ok = secp_nonce_scalar(kk, cand) ? 1 : 0;
        fwrite(&ok, 1, 1, stdout);
        break;
      }
      case 4: {
        if (!rd(a, 32)) return 1;
        uint32_t w[8];
        words_from_be32(w, a);
        fp x;
        fp_from_words(x, w);
        scn r;
        secp_r_from_x(r, x);
        put_scalar(r);
        break;
      }
      case 5: {
        if (!rd(a, 32) || !rd(b, 32) || !rd(k, 32)) return 1;
        scn d, e, kk;
        raw_scalar(d, a);
        raw_scalar(e, b);
        raw_scalar(kk, k);
        uint32_t sig[16];
        const uint8_t ok = secp_sign_with_nonce(sig, d, e, kk, gtab()) ? 1 : 0;
        fwrite(&ok, 1, 1, stdout);
        put_be(sig, 16);
        break;
      }
      case 6: {
        fp x, r;
        if (!rd(x.v, 40)) return 1;
        fp_invert(r, x);
        if (!fp_within(r, 1)) return 2;
        fp_normalize(r);
        scn out;
        fp_to_words(out.v, r);
        put_scalar(out);
        break;
      }
      case 7: {
        if (!rd(a, 32)) return 1;
        uint32_t dg[8], out[5];
        be_words(dg, a, 8);
        ripemd160_33(out, dg);
        for (int i = 0; i < 5; i++) {
          const uint8_t le[4] = {(uint8_t)out[i], (uint8_t)(out[i] >> 8), (uint8_t)(out[i] >> 16), (uint8_t)(out[i] >> 24)};
          fwrite(le, 1, 4, stdout);
        }
        break;
      }
      case 8: {
        if (!rd(a, 32)) return 1;
        const uint8_t ok = secp_privkey_in_range(a) ? 1 : 0;
        fwrite(&ok, 1, 1, stdout);
        break;
      }
      case 9: {
        if (!rd(a, 32)) return 1;
        uint32_t cw[8];
        be_words(cw, a, 8);
        secp_privkey_from_digest(b, cw);
        fwrite(b, 1, 32, stdout);
        break;
      }
      default:
        return 3;
    }
  }
  return 0;
}

static bool read_key(scn& d) {
  uint8_t priv[32];
  if (!rd(priv, 32) || !secp_privkey_in_range(priv)) return false;
  raw_scalar(d, priv);
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) return 4;
  if (!strcmp(argv[1], "prim")) return primitives();
  uint32_t n;
  if (!rd(&n, 4)) return 1;
  if (!strcmp(argv[1], "pub")) {
    for (uint32_t i = 0; i < n; i++) {
      scn d;
      if (!read_key(d)) return 1;
      uint32_t pkw[9], addr[5];
      secp_pubkey_one(pkw, addr, true, d, gtab());
      for (int b = 0; b < 33; b++) {
        const uint8_t v = (uint8_t)(pkw[b / 4] >> (24 - 8 * (b % 4)));
        fwrite(&v, 1, 1, stdout);
      }
      fwrite(addr, 4, 5, stdout);
    }
    return 0;
  }
  if (!strcmp(argv[1], "sign")) {
    for (uint32_t i = 0; i < n; i++) {
      scn d;
      uint32_t mlen;
      if (!read_key(d) || !rd(&mlen, 4)) return 1;
      // the message at an odd offset inside a word-aligned buffer
      std::vector<uint32_t> buf((mlen + 16) / 4 + 2, 0);
      uint8_t* msg = reinterpret_cast<uint8_t*>(buf.data()) + 1 + (i % 3);
      if (!rd(msg, mlen)) return 1;
      uint32_t sig[16];
      const uint8_t ok = secp_sign_one(sig, d, msg, mlen, gtab()) ? 1 : 0;
      fwrite(&ok, 1, 1, stdout);
      put_be(sig, 16);
    }
    return 0;
  }
  return 4;
}
