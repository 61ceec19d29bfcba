// sha256.h -- per-lane SHA-256 of a message in global memory, for gfx950 and
// the host checkers.
//
// The ECDSA message scalar of secp256k1.PubKey.VerifySignature is
// e = SHA-256(msg) (reference call site crypto/secp256k1/secp256k1.go:213,
// crypto.Sha256). Lanes of one wave hash messages of different lengths
// (0 included): the block loop runs per lane for that lane's block count.
// The message is read as sha512.h reads it: 4-byte aligned loads re-aligned
// in registers, only words that hold a message byte, all of a block's words
// loaded before any is used.
#pragma once
#include <stdint.h>

#include "sha512.h"  // funnel_bytes, g_sha512_no_word

namespace cmtv {

#define CMTV_SHA256_K                                                                                        \
  {0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,   \
   0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,   \
   0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,   \
   0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,   \
   0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,   \
   0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,   \
   0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,   \
   0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u}

// round constants: a global table (the rolled loop indexes it with a
// wave-uniform round number: scalar loads)
#ifdef __HIP_DEVICE_COMPILE__
static __constant__ uint32_t g_sha256_K[64] = CMTV_SHA256_K;
#else
static const uint32_t g_sha256_K[64] = CMTV_SHA256_K;
#endif
#undef CMTV_SHA256_K

CMTV_HD uint32_t rotr32(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// one compression; w is consumed (the schedule is expanded in place)
CMTV_HD void sha256_compress(uint32_t st[8], uint32_t w[16]) {
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll 1
  for (int t0 = 0; t0 < 64; t0 += 16) {
#pragma unroll
    for (int i = 0; i < 16; i++) {
      if (t0) {
        const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
        w[i] += (rotr32(w15, 7) ^ rotr32(w15, 18) ^ (w15 >> 3)) + w[(i + 9) & 15] +
                (rotr32(w2, 17) ^ rotr32(w2, 19) ^ (w2 >> 10));
      }
      const uint32_t t1 = h + (rotr32(e, 6) ^ rotr32(e, 11) ^ rotr32(e, 25)) + ((e & f) ^ (~e & g)) +
                          g_sha256_K[t0 + i] + w[i];
      const uint32_t t2 = (rotr32(a, 2) ^ rotr32(a, 13) ^ rotr32(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      h = g;
      g = f;
      f = e;
      e = d + t1;
      d = c;
      c = b;
      b = a;
      a = t1 + t2;
    }
  }
  st[0] += a; st[1] += b; st[2] += c; st[3] += d;
  st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

// SHA-256(msg[0 .. mlen)); out[i] = the digest's i-th big-endian 32-bit word
CMTV_HD void sha256_msg(uint32_t out[8], const uint8_t* msg, uint32_t mlen) {
  uint32_t st[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                    0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  const uint32_t nblocks = (mlen + 9 + 63) / 64;
  const uint32_t sh = (uint32_t)((uintptr_t)msg & 3);
  // aligned base (pointer arithmetic keeps msg's address space: global loads)
  const uint32_t* mw = reinterpret_cast<const uint32_t*>(msg - sh);
  const uint32_t nwords = mlen ? (sh + mlen + 3) / 4 : 0u;  // aligned words holding message bytes
  // an index past the message's last word re-reads that word and is masked; an
  // empty message, with no word to read at all, reads g_sha512_no_word
  const uint32_t jmax = nwords ? nwords - 1 : 0u;
  const uint32_t* mb = nwords ? mw : &g_sha512_no_word;
#pragma unroll 1
  for (uint32_t b = 0; b < nblocks; b++) {
    uint32_t mv[17];
#pragma unroll
    for (int k = 0; k < 17; k++) {
      const uint32_t j = b * 16 + k;
      mv[k] = mb[j < nwords ? j : jmax];
    }
#pragma unroll
    for (int k = 0; k < 17; k++) mv[k] = b * 16 + k < nwords ? mv[k] : 0u;
    uint32_t w[16];
#pragma unroll
    for (int t = 0; t < 16; t++) {
      // little-endian stream word at byte position pos, branch-free: message
      // bytes, then the 0x80 pad byte, then zeros
      const uint32_t pos = b * 64 + 4 * t;
      const uint32_t v = funnel_bytes(mv[t + 1], mv[t], sh);
      const int r = (int)mlen - (int)pos;  // message bytes left at this word
      const uint32_t rr = r < 0 ? 0u : (r > 4 ? 4u : (uint32_t)r);
      const uint32_t keep = (uint32_t)((1ull << (8 * rr)) - 1u);
      const uint32_t pad = (r >= 0 && r < 4) ? (0x80u << (8 * rr)) : 0u;
      w[t] = __builtin_bswap32((v & keep) | pad);
    }
    if (b == nblocks - 1) {
      w[14] = mlen >> 29;
      w[15] = mlen << 3;
    }
    sha256_compress(st, w);
  }
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = st[i];
}

}  // namespace cmtv
