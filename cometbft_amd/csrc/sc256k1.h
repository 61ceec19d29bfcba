// sc256k1.h -- integers mod n, the order of secp256k1, for gfx950 VALU and the
// host checkers.
//
// Representation: eight little-endian 32-bit words, always fully reduced
// (value in [0, n)); no lazy bounds to track. Products are 8 x 8 schoolbook
// rows of v_mad_u64_u32 (a * b + word + carry never exceeds 2^64 - 1); the
// 512-bit product folds by 2^256 = C (mod n), C = 2^256 - n < 2^129, four
// times (512 -> 386 -> 260 -> 257 -> 256 bits) and subtracts n at most once.
//
// This is what dcrd's secp256k1.ModNScalar does for the reference's
// secp256k1.PubKey.VerifySignature (crypto/secp256k1/secp256k1.go:192-217):
// SetByteSlice reduces a 32-byte value >= n (the overflow flag is ignored
// there), IsOverHalfOrder is the lower-S rule.
#pragma once
#include <stdint.h>

#include "fe25519.h"  // CMTV_HD, CMTV_ASSERT

namespace cmtv {

struct scn {
  uint32_t v[8];
};

CMTV_HD uint32_t scn_n_word(int i) {
  return i == 0 ? 0xD0364141u : i == 1 ? 0xBFD25E8Cu : i == 2 ? 0xAF48A03Bu : i == 3 ? 0xBAAEDCE6u
         : i == 4 ? 0xFFFFFFFEu : 0xFFFFFFFFu;
}
// C = 2^256 - n (five words)
CMTV_HD uint32_t scn_c_word(int i) {
  return i == 0 ? 0x2FC9BEBFu : i == 1 ? 0x402DA173u : i == 2 ? 0x50B75FC4u : i == 3 ? 0x45512319u : 1u;
}
// (n - 1) / 2
CMTV_HD uint32_t scn_half_word(int i) {
  return i == 0 ? 0x681B20A0u : i == 1 ? 0xDFE92F46u : i == 2 ? 0x57A4501Du : i == 3 ? 0x5D576E73u
         : i == 7 ? 0x7FFFFFFFu : 0xFFFFFFFFu;
}
// p - n: r + n < p exactly when r < p - n
CMTV_HD uint32_t scn_pmn_word(int i) {
  return i == 0 ? 0x2FC9BAEEu : i == 1 ? 0x402DA172u : i == 2 ? 0x50B75FC4u : i == 3 ? 0x45512319u
         : i == 4 ? 1u : 0u;
}

// a < b for eight-word values (b given by a word function)
template <class F>
CMTV_HD bool scn_words_less(const uint32_t a[8], F bword) {
  uint64_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) borrow = (((uint64_t)a[i] - bword(i) - borrow) >> 32) & 1;
  return borrow != 0;
}

// r = a - n if a >= n (a < 2^256 < 2 n)
CMTV_HD void scn_cond_sub_n(uint32_t r[8], const uint32_t a[8]) {
  uint32_t d[8];
  uint64_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t t = (uint64_t)a[i] - scn_n_word(i) - borrow;
    d[i] = (uint32_t)t;
    borrow = (t >> 32) & 1;
  }
  const bool take = borrow == 0;
#pragma unroll
  for (int i = 0; i < 8; i++) r[i] = take ? d[i] : a[i];
}

// 32 big-endian bytes as eight little-endian words (not reduced); reads
// bytes, so the pointer needs no alignment
CMTV_HD void words_from_be32(uint32_t w[8], const uint8_t* b) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint8_t* q = b + 4 * (7 - i);
    w[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
  }
}

CMTV_HD void scn_from_words(scn& r, const uint32_t w[8]) { scn_cond_sub_n(r.v, w); }

CMTV_HD bool scn_is_zero(const scn& a) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) o |= a.v[i];
  return o == 0;
}

// a > (n - 1) / 2
CMTV_HD bool scn_over_half(const scn& a) {
  uint64_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) borrow = (((uint64_t)scn_half_word(i) - a.v[i] - borrow) >> 32) & 1;
  return borrow != 0;
}

// out[0 .. OL) = x[0 .. 8) + x[8 .. 8 + HL) * C; the caller's OL holds the sum
template <int HL, int OL>
CMTV_HD void scn_fold(uint32_t out[OL], const uint32_t* x) {
#pragma unroll
  for (int i = 0; i < OL; i++) out[i] = i < 8 ? x[i] : 0u;
#pragma unroll
  for (int i = 0; i < HL; i++) {
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
      if (i + j < OL) {
        const uint64_t t = (uint64_t)x[8 + i] * scn_c_word(j) + out[i + j] + carry;
        out[i + j] = (uint32_t)t;
        carry = t >> 32;
      }
    }
#pragma unroll
    for (int k = i + 5; k < OL; k++) {
      const uint64_t t = (uint64_t)out[k] + carry;
      out[k] = (uint32_t)t;
      carry = t >> 32;
    }
  }
}

CMTV_HD void scn_mul(scn& r, const scn& a, const scn& b) {
  uint32_t p[16];
#pragma unroll
  for (int i = 0; i < 16; i++) p[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint64_t t = (uint64_t)a.v[i] * b.v[j] + p[i + j] + carry;
      p[i + j] = (uint32_t)t;
      carry = t >> 32;
    }
    p[i + 8] = (uint32_t)carry;
  }
  uint32_t f1[13], f2[9], f3[9], f4[8];
  scn_fold<8, 13>(f1, p);   // < 2^386
  scn_fold<5, 9>(f2, f1);   // < 2^260
  scn_fold<1, 9>(f3, f2);   // < 2^256 + 2^134
  scn_fold<1, 8>(f4, f3);   // f3[8] = 1 only with f3's low half < 2^134: < 2^256
  scn_cond_sub_n(r.v, f4);
  CMTV_SCHED_FENCE();
}

// word i of n - 2
CMTV_HD uint32_t scn_nm2_word(int i) { return i == 0 ? 0xD036413Fu : scn_n_word(i); }

// r = a^(n - 2) = 1 / a (0 for a = 0): square-and-multiply over the constant
// exponent (wave-uniform branches), 256 squarings and 196 multiplications
CMTV_HD void scn_invert(scn& r, const scn& a) {
  scn x;
#pragma unroll
  for (int i = 0; i < 8; i++) x.v[i] = i == 0 ? 1u : 0u;
#pragma unroll 1
  for (int i = 255; i >= 0; i--) {
    scn_mul(x, x, x);
    if ((scn_nm2_word(i >> 5) >> (i & 31)) & 1) scn_mul(x, x, a);
  }
  r = x;
}

}  // namespace cmtv
