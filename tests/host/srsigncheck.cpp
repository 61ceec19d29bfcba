// Host-side build of the sr25519 signing code (cometbft_amd/csrc/
// sr25519_sign.h and what it stands on) with operand-bound assertions on,
// built with AddressSanitizer and UBSan by tests/test_sr25519_sign_host.py.
// Test infrastructure only: checks the kernel source without a GPU.
//
// argv[1] == "sign": whole signatures (sr_sign_one, the kernel's per-lane function)
//   input  (stdin):  u32 n, then n x { u8 mini[32], u32 mlen, u8 msg[mlen] }
//   output (stdout): n x u8 sig[64]
// argv[1] == "pub": public keys and addresses (sr_pubkey_from_mini, sr_address)
//   input:  u32 n, then n x u8 mini[32]
//   output: n x { u8 pk[32], u8 addr[20] }
// argv[1] == "prim": primitives
//   input:  u32 count, then records { u32 op, operands }; 32-byte values little-endian
//   output: per record its result
//     1 encode a point   u8 x[32], y[32], z[32]: (X, Y, Z, T) = (xz, yz, z, xyz)  -> u8[32]
//     2 encode [s]B      u8 s[32] (s < L)                                         -> u8[32]
//     3 sr_expand        u8 mini[32]                                              -> u8 key[32], nonce[32]
//     4 sr_witness       u8 nonce[32], u32 mlen, u8 msg[mlen]                     -> u8 r[32]
//     5 sr_sign_keyed    u8 key[32], r[32], pk[32], u32 mlen, u8 msg[mlen]        -> u8 sig[64]
#define CMTV_HD inline
#define CMTV_BOUNDS_CHECK 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../cometbft_amd/csrc/sr25519_sign.h"
#include "lazy_btab.h"

using namespace cmtv;

static bool rd(void* p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }

static void to_words(uint32_t* w, const uint8_t* b, int nw) {
  for (int i = 0; i < nw; i++)
    w[i] = b[4 * i] | (b[4 * i + 1] << 8) | (b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
}
static bool rd_words(uint32_t w[8]) {
  uint8_t b[32];
  if (!rd(b, 32)) return false;
  to_words(w, b, 8);
  return true;
}
static void put_words(const uint32_t* w, int nw) {
  for (int i = 0; i < nw; i++) {
    const uint8_t b[4] = {(uint8_t)w[i], (uint8_t)(w[i] >> 8), (uint8_t)(w[i] >> 16), (uint8_t)(w[i] >> 24)};
    fwrite(b, 1, 4, stdout);
  }
}

// a message at an odd offset inside a word-aligned buffer, as the kernels meet them
struct Msg {
  std::vector<uint32_t> buf;
  uint8_t* p = nullptr;
  uint32_t len = 0;
  bool read(uint32_t shift) {
    if (!rd(&len, 4) || len > (1u << 20)) return false;
    buf.assign((len + 16) / 4 + 2, 0);
    p = reinterpret_cast<uint8_t*>(buf.data()) + shift % 4;
    return rd(p, len);
  }
};

static int primitives(const LazyBTab& bt, const uint32_t* prog, int nops) {
  uint32_t count;
  if (!rd(&count, 4)) return 1;
  for (uint32_t c = 0; c < count; c++) {
    uint32_t op, a[8], b[8], d[8], out[16];
    if (!rd(&op, 4)) return 1;
    switch (op) {
      case 1: {
        if (!rd_words(a) || !rd_words(b) || !rd_words(d)) return 1;
        fe x, y, z;
        fe_frombytes(x, a);
        fe_frombytes(y, b);
        fe_frombytes(z, d);
        ge_p3 P;
        fe_mul(P.X, x, z);
        fe_mul(P.Y, y, z);
        P.Z = z;
        fe_mul(P.T, x, P.Y);
        ristretto_encode(out, P);
        put_words(out, 8);
        break;
      }
      case 2: {
        if (!rd_words(a)) return 1;
        ge_p3 P;
        q_bcomb16(P, a, bt);
        ristretto_encode(out, P);
        put_words(out, 8);
        break;
      }
      case 3: {
        if (!rd_words(a)) return 1;
        sr_expand(out, out + 8, a);
        put_words(out, 16);
        break;
      }
      case 4: {
        Msg m;
        if (!rd_words(a) || !m.read(c)) return 1;
        sr_witness(out, a, m.p, m.len);
        put_words(out, 8);
        break;
      }
      case 5: {
        Msg m;
        if (!rd_words(a) || !rd_words(b) || !rd_words(d) || !m.read(c)) return 1;
        ArrayStrobeState st;
        sr_sign_keyed(out, a, d, b, m.p, m.len, prog, nops, st, bt);
        put_words(out, 16);
        break;
      }
      default:
        return 3;
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 4;
  LazyBTab bt;
  uint32_t prog[SR_PREFIX_WORDS];  // the program the runtime uploads
  const int nops = sr_prefix_state(prog);
  if (!strcmp(argv[1], "prim")) return primitives(bt, prog, nops);
  uint32_t n;
  if (!rd(&n, 4)) return 1;
  if (!strcmp(argv[1], "pub")) {
    for (uint32_t i = 0; i < n; i++) {
      uint32_t mini[8], pk[8], addr[5];
      if (!rd_words(mini)) return 1;
      sr_pubkey_from_mini(pk, mini, bt);
      sr_address(addr, pk);
      put_words(pk, 8);
      put_words(addr, 5);
    }
    return 0;
  }
  if (!strcmp(argv[1], "sign")) {
    for (uint32_t i = 0; i < n; i++) {
      uint32_t mini[8], sig[16];
      Msg m;
      if (!rd_words(mini) || !m.read(i)) return 1;
      ArrayStrobeState st;
      sr_sign_one(sig, mini, m.p, m.len, prog, nops, st, bt);
      put_words(sig, 16);
    }
    return 0;
  }
  return 4;
}
