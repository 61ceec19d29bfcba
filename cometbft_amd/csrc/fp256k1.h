// fp256k1.h -- GF(p), p = 2^256 - 2^32 - 977 (the secp256k1 field), for gfx950
// VALU and, with CMTV_HD redefined, for the host checkers (tests/host/).
//
// Representation: 10 unsigned 32-bit limbs in radix 2^26 (limb i holds bits
// [26 i, 26 i + 26); limb 9 holds the top 22 bits). A limb product is a
// 32x32->64 multiply-accumulate (v_mad_u64_u32), as in fe25519.h.
//
// Lazy reduction, all limbs unsigned. An element has MAGNITUDE m when
//   v[i] <= 2 m (2^26 - 1) for i < 9 and v[9] <= 2 m (2^22 - 1).
//   fp_mul / fp_sq / fp_mul_small : inputs of magnitude <= 8 (every limb
//       <= 2^30, so the ten-product column sums stay below 2^64); output 1
//   fp_add      : magnitudes add
//   fp_neg(m)   : 2 (m + 1) p - a for a of magnitude <= m; output m + 1
//   fp_sub(m)   : a + fp_neg(b, m)
//   fp_normalize: any magnitude <= 16 -> the canonical value in [0, p)
//   fp_invert   : input of magnitude <= 8; output 1
// The point formulas in secp256k1.h state the magnitude of every operand;
// CMTV_BOUNDS_CHECK builds (tests/host/secpcheck.cpp) assert them.
//
// Reduction folds the high half by 2^256 = 2^32 + 977 (mod p): a carried
// 20-limb product's limbs 10..19 sit at 2^260 = 2^36 + 15632, i.e. 15632 into
// the same limb and 1024 into the next.
//
// This is the field arithmetic dcrd's secp256k1.FieldVal performs (the same
// 10 x 26 layout) for the reference's secp256k1.PubKey.VerifySignature
// (crypto/secp256k1/secp256k1.go:192-217).
#pragma once
#include <stdint.h>

#include "fe25519.h"  // CMTV_HD, CMTV_SCHED_FENCE, CMTV_ASSERT

namespace cmtv {

struct fp {
  uint32_t v[10];
};

constexpr uint32_t FP_M26 = (1u << 26) - 1;
constexpr uint32_t FP_M22 = (1u << 22) - 1;
constexpr uint32_t FP_P0 = 0x3FFFC2F;  // p's limb 0
constexpr uint32_t FP_P1 = 0x3FFFFBF;  // p's limb 1 (limbs 2..8: FP_M26, limb 9: FP_M22)
constexpr uint32_t FP_MAX_MAG = 8;

CMTV_HD uint32_t fp_p_limb(int i) { return i == 0 ? FP_P0 : i == 1 ? FP_P1 : i == 9 ? FP_M22 : FP_M26; }

CMTV_HD bool fp_within(const fp& a, uint32_t m) {
  bool ok = a.v[9] <= 2 * m * FP_M22;
#pragma unroll
  for (int i = 0; i < 9; i++) ok = ok && a.v[i] <= 2 * m * FP_M26;
  return ok;
}

CMTV_HD void fp_set_small(fp& r, uint32_t x) {
#pragma unroll
  for (int i = 1; i < 10; i++) r.v[i] = 0;
  r.v[0] = x;
}

CMTV_HD void fp_add(fp& r, const fp& a, const fp& b) {
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = a.v[i] + b.v[i];
}

// r = 2 (m + 1) p - a, a of magnitude <= m
CMTV_HD void fp_neg(fp& r, const fp& a, uint32_t m) {
  CMTV_ASSERT(m < FP_MAX_MAG && fp_within(a, m));
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = 2 * (m + 1) * fp_p_limb(i) - a.v[i];
}

// r = a - b (mod p), b of magnitude <= mb; magnitude(a) + mb + 1
CMTV_HD void fp_sub(fp& r, const fp& a, const fp& b, uint32_t mb) {
  CMTV_ASSERT(mb < FP_MAX_MAG && fp_within(b, mb));
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = a.v[i] + (2 * (mb + 1) * fp_p_limb(i) - b.v[i]);
}

CMTV_HD void fp_select(fp& r, const fp& a, const fp& b, bool take_b) {
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = take_b ? b.v[i] : a.v[i];
}

// Ten 64-bit limb sums (each < 2^63) at weights 2^(26 i), plus `top` at 2^260
// -> magnitude 1.
CMTV_HD void fp_reduce64(fp& r, uint64_t t[10], uint64_t top) {
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    t[i] += c;
    c = t[i] >> 26;
    t[i] &= FP_M26;
  }
  top += c;  // < 2^49 for fp_mul's input
  t[0] += top * 15632;
  t[1] += top * 1024;
  c = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    t[i] += c;
    c = t[i] >> 26;
    t[i] &= FP_M26;
  }
  t[9] += c;
  const uint64_t x = t[9] >> 22;  // the bits at and above 2^256
  t[9] &= FP_M22;
  t[0] += x * 977;
  t[1] += x << 6;
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = (uint32_t)t[i];
}

CMTV_HD void fp_mul(fp& r, const fp& a, const fp& b) {
  CMTV_ASSERT(fp_within(a, FP_MAX_MAG) && fp_within(b, FP_MAX_MAG));
  uint64_t c[20];
#pragma unroll
  for (int k = 0; k < 19; k++) {
    uint64_t s = 0;
#pragma unroll
    for (int i = 0; i < 10; i++)
      if (k - i >= 0 && k - i < 10) s += (uint64_t)a.v[i] * b.v[k - i];
    c[k] = s;
  }
  // carry the 19 columns (each < 10 * 2^60) to 26 bits
  uint64_t cy = 0;
#pragma unroll
  for (int k = 0; k < 19; k++) {
    c[k] += cy;
    cy = c[k] >> 26;
    c[k] &= FP_M26;
  }
  c[19] = cy;  // < 2^38
  // limbs 10..19 (weight 2^260 * 2^(26 j)) fold to 15632 at j and 1024 at j + 1
  uint64_t t[10];
#pragma unroll
  for (int k = 0; k < 10; k++) t[k] = c[k] + c[10 + k] * 15632 + (k ? c[9 + k] * 1024 : 0);
  fp_reduce64(r, t, c[19] * 1024);
  CMTV_SCHED_FENCE();
}

CMTV_HD void fp_sq(fp& r, const fp& a) { fp_mul(r, a, a); }

// r = k a for a small constant k (k <= 2^10)
CMTV_HD void fp_mul_small(fp& r, const fp& a, uint32_t k) {
  CMTV_ASSERT(fp_within(a, FP_MAX_MAG) && k <= 1024);
  uint64_t t[10];
#pragma unroll
  for (int i = 0; i < 10; i++) t[i] = (uint64_t)a.v[i] * k;
  fp_reduce64(r, t, 0);
}

// the canonical representative in [0, p); any magnitude <= 16
CMTV_HD void fp_normalize(fp& r) {
  CMTV_ASSERT(fp_within(r, 16));
  uint32_t t[10];
#pragma unroll
  for (int i = 0; i < 10; i++) t[i] = r.v[i];
  uint32_t x = t[9] >> 22;
  t[9] &= FP_M22;
  t[0] += x * 977;
  t[1] += x << 6;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    t[i + 1] += t[i] >> 26;
    t[i] &= FP_M26;
  }
  // now below 2^256 + 2^47 < 2 p: one conditional subtraction of p, i.e. an
  // addition of 2^32 + 977 that carries out of bit 256
  uint32_t m = t[2];
#pragma unroll
  for (int i = 3; i < 9; i++) m &= t[i];
  x = (t[9] >> 22) |
      ((t[9] == FP_M22 && m == FP_M26 && (t[1] + 0x40 + ((t[0] + 0x3D1) >> 26)) > FP_M26) ? 1u : 0u);
  t[0] += x * 977;
  t[1] += x << 6;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    t[i + 1] += t[i] >> 26;
    t[i] &= FP_M26;
  }
  t[9] &= FP_M22;
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = t[i];
}

CMTV_HD bool fp_is_zero(const fp& a) {
  fp t = a;
  fp_normalize(t);
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 10; i++) o |= t.v[i];
  return o == 0;
}

CMTV_HD bool fp_equal(const fp& a, const fp& b) {
  fp s = a, t = b;
  fp_normalize(s);
  fp_normalize(t);
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 10; i++) o |= s.v[i] ^ t.v[i];
  return o == 0;
}

// from a 256-bit integer as eight little-endian 32-bit words (any value below
// 2^256: not reduced, limbs canonical) / to words (a normalised)
CMTV_HD void fp_from_words(fp& r, const uint32_t w[8]) {
#pragma unroll
  for (int i = 0; i < 10; i++) {
    const int bit = 26 * i, k = bit >> 5, sh = bit & 31;
    uint32_t x = w[k] >> sh;
    if (sh > 6 && k + 1 < 8) x |= w[k + 1] << (32 - sh);
    r.v[i] = x & FP_M26;
  }
}

CMTV_HD void fp_to_words(uint32_t w[8], const fp& a) {
#pragma unroll
  for (int k = 0; k < 8; k++) w[k] = 0;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    const int bit = 26 * i, k = bit >> 5, sh = bit & 31;
    w[k] |= a.v[i] << sh;
    if (sh > 6 && k + 1 < 8) w[k + 1] |= a.v[i] >> (32 - sh);
  }
}

// r = a^(2^n), n >= 1
CMTV_HD void fp_sqn(fp& r, const fp& a, int n) {
  fp_sq(r, a);
#pragma unroll 1
  for (int i = 1; i < n; i++) fp_sq(r, r);
}

// r = a^((p + 1) / 4): a square root of a when a is a square (the caller
// checks r^2 = a). Fixed chain over the exponent's runs of ones (223, 22 and
// 2 ones): 253 squarings, 13 multiplications.
CMTV_HD void fp_sqrt_candidate(fp& r, const fp& a) {
  fp x2, x3, x22, x44, t;
  fp_sq(t, a);
  fp_mul(x2, t, a);
  fp_sq(t, x2);
  fp_mul(x3, t, a);
  fp_sqn(t, x3, 3);
  fp_mul(t, t, x3);  // x6
  fp_sqn(t, t, 3);
  fp_mul(t, t, x3);  // x9
  fp_sqn(t, t, 2);
  fp_mul(t, t, x2);  // x11
  fp_sqn(x22, t, 11);
  fp_mul(x22, x22, t);
  fp_sqn(x44, x22, 22);
  fp_mul(x44, x44, x22);
  fp x88;
  fp_sqn(x88, x44, 44);
  fp_mul(x88, x88, x44);
  fp_sqn(t, x88, 88);
  fp_mul(t, t, x88);  // x176
  fp_sqn(t, t, 44);
  fp_mul(t, t, x44);  // x220
  fp_sqn(t, t, 3);
  fp_mul(t, t, x3);  // x223
  fp_sqn(t, t, 23);
  fp_mul(t, t, x22);
  fp_sqn(t, t, 6);
  fp_mul(t, t, x2);
  fp_sqn(r, t, 2);
}

// r = a^(p - 2) = 1 / a (0 for a = 0). a of magnitude <= 8 (fp_mul's bound);
// output magnitude 1. Fixed chain over the exponent's runs of ones (223 and 22
// ones, then the low ten bits 0000101101): 255 squarings, 15 multiplications.
// The chain up to x223 is fp_sqrt_candidate's (kept apart so the verifier's
// code stays as it was).
CMTV_HD void fp_invert(fp& r, const fp& a) {
  CMTV_ASSERT(fp_within(a, FP_MAX_MAG));
  fp x2, x3, x22, x44, x88, t;
  fp_sq(t, a);
  fp_mul(x2, t, a);
  fp_sq(t, x2);
  fp_mul(x3, t, a);
  fp_sqn(t, x3, 3);
  fp_mul(t, t, x3);  // x6
  fp_sqn(t, t, 3);
  fp_mul(t, t, x3);  // x9
  fp_sqn(t, t, 2);
  fp_mul(t, t, x2);  // x11
  fp_sqn(x22, t, 11);
  fp_mul(x22, x22, t);
  fp_sqn(x44, x22, 22);
  fp_mul(x44, x44, x22);
  fp_sqn(x88, x44, 44);
  fp_mul(x88, x88, x44);
  fp_sqn(t, x88, 88);
  fp_mul(t, t, x88);  // x176
  fp_sqn(t, t, 44);
  fp_mul(t, t, x44);  // x220
  fp_sqn(t, t, 3);
  fp_mul(t, t, x3);  // x223
  fp_sqn(t, t, 23);
  fp_mul(t, t, x22);
  fp_sqn(t, t, 5);
  fp_mul(t, t, a);
  fp_sqn(t, t, 3);
  fp_mul(t, t, x2);
  fp_sqn(t, t, 2);
  fp_mul(r, t, a);
}

}  // namespace cmtv
