// secp256k1_sign.h -- secp256k1 key derivation and RFC 6979 ECDSA signing, one
// key or signature per lane, for gfx950 and the host checkers: the device form
// of the reference's PrivKey.PubKey, PubKey.Address and PrivKey.Sign
// (crypto/secp256k1/secp256k1.go:45, 156, 128; btcec's ecdsa.SignCompact with
// its recovery byte dropped). For synthetic test data: VARIABLE TIME (table
// rows are picked by secret digits, the nonce loop branches on secret data).
//
// Byte contract (restated from RFC 6979 section 3.2; tests/secp256k1_sign_ref.py):
//   private key  d, 32 bytes big-endian, 0 < d < n (the caller checked)
//   public key   0x02 | (y & 1), then x big-endian, (x, y) = [d]G: 33 bytes
//   address      RIPEMD-160(SHA-256(public key)): 20 bytes
//   signature    r || s, each 32 bytes big-endian:
//     h1 = SHA-256(msg), e = h1 mod n
//     V = 0x01 x 32, K = 0x00 x 32
//     K = HMAC(K, V || 0x00 || d || e), V = HMAC(K, V)        (HMAC-SHA-256;
//     K = HMAC(K, V || 0x01 || d || e), V = HMAC(K, V)         d, e as 32 bytes)
//     loop: V = HMAC(K, V); k = V
//           k = 0, k >= n, r = 0 or s = 0: K = HMAC(K, V || 0x00), V = HMAC(K, V), again
//     r = ([k]G).x mod n, s = (e + r d) / k mod n, s = n - s when s > (n - 1) / 2
// The rejection branch has probability about 2^-128 per signature; the device
// loop gives up after SECP_SIGN_MAX_TRIES candidates (probability 2^-1000) and
// returns false rather than spin on a shared device.
//
// "Big-endian words" below: eight uint32, word 0 the most significant, each
// the big-endian value of its four bytes (sha256.h's digest layout). A scalar
// s (sc256k1.h, little-endian words) has big-endian word i = s.v[7 - i].
//
// [k]G and [d]G are the verifier's comb over the fixed table (secp256k1.h
// secp_comb_add: 33 additions); the affine x (and y) come from one inversion
// mod p (fp256k1.h fp_invert) of the homogeneous Z.
#pragma once
#include <stdint.h>

#include "secp256k1.h"

namespace cmtv {

constexpr int SECP_SIGN_MAX_TRIES = 8;

CMTV_HD void sha256_iv(uint32_t st[8]) {
  st[0] = 0x6a09e667u; st[1] = 0xbb67ae85u; st[2] = 0x3c6ef372u; st[3] = 0xa54ff53au;
  st[4] = 0x510e527fu; st[5] = 0x9b05688cu; st[6] = 0x1f83d9abu; st[7] = 0x5be0cd19u;
}

// ---------------------------------------------------------------- scalars
// r = a + b mod n
CMTV_HD void scn_add(scn& r, const scn& a, const scn& b) {
  uint32_t s[8], d[8];
  uint64_t cy = 0, borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    cy += (uint64_t)a.v[i] + b.v[i];
    s[i] = (uint32_t)cy;
    cy >>= 32;
  }
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t t = (uint64_t)s[i] - scn_n_word(i) - borrow;
    d[i] = (uint32_t)t;
    borrow = (t >> 32) & 1;
  }
  const bool take = cy != 0 || borrow == 0;  // the 257-bit sum is >= n
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = take ? d[i] : s[i];
}

// r = -a mod n
CMTV_HD void scn_neg(scn& r, const scn& a) {
  const bool zero = scn_is_zero(a);
  uint64_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t t = (uint64_t)scn_n_word(i) - a.v[i] - borrow;
    r.v[i] = zero ? 0u : (uint32_t)t;
    borrow = (t >> 32) & 1;
  }
}

// ---------------------------------------------------------------- HMAC-SHA-256
// out = HMAC-SHA-256(key, data): a 32-byte key (big-endian words), so ipad and
// opad are one block each; data of LEN = 32, 33 or 97 bytes as (LEN + 3) / 4
// big-endian words, the bytes past LEN zero. Every block is built in registers
// with static indices; 4 compressions for LEN <= 55, 5 for 97. out may alias
// key or data.
template <int LEN>
CMTV_HD void hmac_sha256_32(uint32_t out[8], const uint32_t key[8], const uint32_t* data) {
  static_assert(LEN == 32 || LEN == 33 || LEN == 97, "the nonce generator's data lengths");
  constexpr int NW = (LEN + 3) / 4, NB = (LEN + 9 + 63) / 64, PADW = LEN / 4;
  constexpr uint32_t PAD = 0x80000000u >> (8 * (LEN % 4));
  uint32_t in[8], st[8], w[16];
  sha256_iv(in);
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = (i < 8 ? key[i] : 0u) ^ 0x36363636u;
  sha256_compress(in, w);
#pragma unroll
  for (int b = 0; b < NB; b++) {
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int j = 16 * b + i;
      w[i] = (j < NW ? data[j] : 0u) | (j == PADW ? PAD : 0u);
    }
    if (b == NB - 1) w[15] = (64u + LEN) * 8u;
    sha256_compress(in, w);
  }
  sha256_iv(st);
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = (i < 8 ? key[i] : 0u) ^ 0x5c5c5c5cu;
  sha256_compress(st, w);
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = i < 8 ? in[i] : 0u;
  w[8] = 0x80000000u;
  w[15] = (64u + 32u) * 8u;
  sha256_compress(st, w);
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = st[i];
}

// ---------------------------------------------------------------- the nonce generator
// RFC 6979 section 3.2's K and V (big-endian words)
struct Rfc6979 {
  uint32_t K[8], V[8];
};

// K = HMAC(K, V || tag || x || h), V = HMAC(K, V)   (steps d-e, f-g)
CMTV_HD void rfc6979_seed_step(Rfc6979& g, uint32_t tag, const uint32_t x[8], const uint32_t h[8]) {
  uint32_t data[25];
#pragma unroll
  for (int i = 0; i < 8; i++) data[i] = g.V[i];
  // the 65 bytes tag || x || h: the 64-byte stream x || h moved one byte down
#pragma unroll
  for (int k = 0; k <= 16; k++) {
    const uint32_t prev = k == 0 ? tag : k <= 8 ? x[k - 1] : h[k - 9];
    const uint32_t cur = k < 8 ? x[k] : k < 16 ? h[k - 8] : 0u;
    data[8 + k] = (prev << 24) | (cur >> 8);
  }
  hmac_sha256_32<97>(g.K, g.K, data);
  hmac_sha256_32<32>(g.V, g.K, g.V);
}

// Steps b-g. x = int2octets(d), h = bits2octets(h1) = h1 mod n: big-endian words.
CMTV_HD void rfc6979_init(Rfc6979& g, const uint32_t x[8], const uint32_t h[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    g.V[i] = 0x01010101u;
    g.K[i] = 0u;
  }
  rfc6979_seed_step(g, 0u, x, h);
  rfc6979_seed_step(g, 1u, x, h);
}

// Step h: the next candidate (big-endian words; qlen = hlen = 256, so T is one
// V). With retry, first the update after a rejected candidate:
// K = HMAC(K, V || 0x00), V = HMAC(K, V).
CMTV_HD void rfc6979_next(Rfc6979& g, uint32_t cand[8], bool retry) {
  if (retry) {
    uint32_t data[9];
#pragma unroll
    for (int i = 0; i < 8; i++) data[i] = g.V[i];
    data[8] = 0u;
    hmac_sha256_32<33>(g.K, g.K, data);
    hmac_sha256_32<32>(g.V, g.K, g.V);
  }
  hmac_sha256_32<32>(g.V, g.K, g.V);
#pragma unroll
  for (int i = 0; i < 8; i++) cand[i] = g.V[i];
}

// k = bits2int(candidate); whether 0 < k < n (k is reduced either way)
CMTV_HD bool secp_nonce_scalar(scn& k, const uint32_t cand[8]) {
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = cand[7 - i];
  const bool below = scn_words_less(w, [](int i) { return scn_n_word(i); });
  scn_from_words(k, w);
  return below && !scn_is_zero(k);
}

// ---------------------------------------------------------------- points
// Affine x (and y, when wanted) of a homogeneous point out of pt_add
// (magnitudes (3, 2, 2)), normalised; infinity gives x = y = 0.
CMTV_HD void pt_affine(fp& x, fp* y, const pt256& p) {
  fp zi;
  fp_invert(zi, p.Z);
  fp_mul(x, p.X, zi);
  fp_normalize(x);
  if (y) {
    fp_mul(*y, p.Y, zi);
    fp_normalize(*y);
  }
}

// r = x mod n for a normalised x (x < p < 2 n: one conditional subtraction)
CMTV_HD void secp_r_from_x(scn& r, const fp& x) {
  uint32_t w[8];
  fp_to_words(w, x);
  scn_from_words(r, w);
}

// ---------------------------------------------------------------- signing
// sig = r || s (16 big-endian words) for the nonce k: r = ([k]G).x mod n,
// s = (e + r d) / k, lower-S. False when r = 0 or s = 0 (sig is then not a
// signature). The signer passes 0 < k < n; k may be any eight words (the comb
// takes every digit string, the products any operand below 2^256: the host
// checker drives the comb's edge digits that way), k = 0 gives r = 0.
template <class GTab>
CMTV_HD bool secp_sign_with_nonce(uint32_t sig[16], const scn& d, const scn& e, const scn& k, const GTab& gt) {
  pt256 acc;
  pt_set_infinity(acc);
  secp_comb_add(acc, k, gt);
  fp x;
  pt_affine(x, nullptr, acc);
  scn r, s, t, ki;
  secp_r_from_x(r, x);
  scn_mul(t, r, d);
  scn_add(t, t, e);
  scn_invert(ki, k);
  scn_mul(s, ki, t);
  const bool ok = !scn_is_zero(r) && !scn_is_zero(s);
  if (scn_over_half(s)) scn_neg(s, s);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    sig[i] = r.v[7 - i];
    sig[8 + i] = s.v[7 - i];
  }
  return ok;
}

// The whole signature of msg by the key d (0 < d < n, little-endian words
// below n). False (sig zeroed) only when SECP_SIGN_MAX_TRIES candidates in a
// row were rejected.
template <class GTab>
CMTV_HD bool secp_sign_one(uint32_t sig[16], const scn& d, const uint8_t* msg, uint32_t mlen, const GTab& gt) {
  scn e;
  secp_msg_scalar(e, msg, mlen);
  uint32_t x[8], h[8], cand[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    x[i] = d.v[7 - i];
    h[i] = e.v[7 - i];
  }
  Rfc6979 g;
  rfc6979_init(g, x, h);
  bool done = false;
#pragma unroll 1
  for (int tries = 0; tries < SECP_SIGN_MAX_TRIES && !done; tries++) {
    rfc6979_next(g, cand, tries != 0);
    scn k;
    done = secp_nonce_scalar(k, cand) && secp_sign_with_nonce(sig, d, e, k, gt);
  }
  if (!done) {
#pragma unroll
    for (int i = 0; i < 16; i++) sig[i] = 0u;
  }
  return done;
}

// ---------------------------------------------------------------- RIPEMD-160
CMTV_HD uint32_t rol32(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }

CMTV_HD uint32_t rmd160_f(int j, uint32_t x, uint32_t y, uint32_t z) {
  return j < 16 ? x ^ y ^ z : j < 32 ? (x & y) | (~x & z) : j < 48 ? (x | ~y) ^ z : j < 64 ? (x & z) | (y & ~z)
                                                                                           : x ^ (y | ~z);
}

// RIPEMD-160 of a 32-byte SHA-256 digest (big-endian words), the second half
// of a 33-byte key's address: one block. out: the digest as five little-endian
// words (its 20 bytes in memory order on a little-endian machine). The 80
// rounds of both lines are unrolled, so the message-word and rotation tables
// are compile-time indices.
CMTV_HD void ripemd160_33(uint32_t out[5], const uint32_t digest[8]) {
  const uint8_t rl[80] = {0, 1, 2,  3,  4,  5,  6,  7, 8, 9,  10, 11, 12, 13, 14, 15, 7, 4,  13, 1,
                          10, 6, 15, 3,  12, 0,  9,  5, 2, 14, 11, 8,  3,  10, 14, 4,  9, 15, 8,  1,
                          2, 7, 0,  6,  13, 11, 5,  12, 1, 9,  11, 10, 0,  8,  12, 4,  13, 3,  7,  15,
                          14, 5, 6,  2,  4,  0,  5,  9, 7, 12, 2,  10, 14, 1,  3,  8,  11, 6,  15, 13};
  const uint8_t rr[80] = {5, 14, 7,  0, 9, 2,  11, 4,  13, 6,  15, 8,  1,  10, 3,  12, 6,  11, 3,  7,
                          0, 13, 5,  10, 14, 15, 8,  12, 4,  9,  1,  2,  15, 5,  1,  3,  7,  14, 6,  9,
                          11, 8, 12, 2, 10, 0,  4,  13, 8,  6,  4,  1,  3,  11, 15, 0,  5,  12, 2,  13,
                          9, 7,  10, 14, 12, 15, 10, 4,  1,  5,  8,  7,  6,  2,  13, 14, 0,  3,  9,  11};
  const uint8_t sl[80] = {11, 14, 15, 12, 5,  8,  7,  9,  11, 13, 14, 15, 6,  7,  9,  8,  7,  6,  8,  13,
                          11, 9,  7,  15, 7,  12, 15, 9,  11, 7,  13, 12, 11, 13, 6,  7,  14, 9,  13, 15,
                          14, 8,  13, 6,  5,  12, 7,  5,  11, 12, 14, 15, 14, 15, 9,  8,  9,  14, 5,  6,
                          8,  6,  5,  12, 9,  15, 5,  11, 6,  8,  13, 12, 5,  12, 13, 14, 11, 8,  5,  6};
  const uint8_t sr[80] = {8,  9,  9,  11, 13, 15, 15, 5,  7,  7,  8,  11, 14, 14, 12, 6,  9,  13, 15, 7,
                          12, 8,  9,  11, 7,  7,  12, 7,  6,  15, 13, 11, 9,  7,  15, 11, 8,  6,  6,  14,
                          12, 13, 5,  14, 13, 13, 7,  5,  15, 5,  8,  11, 14, 14, 6,  14, 6,  9,  12, 9,
                          12, 5,  15, 8,  8,  5,  12, 9,  12, 5,  14, 6,  8,  13, 6,  5,  15, 13, 11, 11};
  const uint32_t kl[5] = {0x00000000u, 0x5A827999u, 0x6ED9EBA1u, 0x8F1BBCDCu, 0xA953FD4Eu};
  const uint32_t kr[5] = {0x50A28BE6u, 0x5C4DD124u, 0x6D703EF3u, 0x7A6D76E9u, 0x00000000u};
  uint32_t x[16];
#pragma unroll
  for (int i = 0; i < 16; i++) x[i] = i < 8 ? __builtin_bswap32(digest[i]) : 0u;
  x[8] = 0x80u;
  x[14] = 256u;
  const uint32_t h0 = 0x67452301u, h1 = 0xEFCDAB89u, h2 = 0x98BADCFEu, h3 = 0x10325476u, h4 = 0xC3D2E1F0u;
  uint32_t al = h0, bl = h1, cl = h2, dl = h3, el = h4;
  uint32_t ar = h0, br = h1, cr = h2, dr = h3, er = h4;
#pragma unroll
  for (int j = 0; j < 80; j++) {
    uint32_t t = rol32(al + rmd160_f(j, bl, cl, dl) + x[rl[j]] + kl[j >> 4], sl[j]) + el;
    al = el;
    el = dl;
    dl = rol32(cl, 10);
    cl = bl;
    bl = t;
    t = rol32(ar + rmd160_f(79 - j, br, cr, dr) + x[rr[j]] + kr[j >> 4], sr[j]) + er;
    ar = er;
    er = dr;
    dr = rol32(cr, 10);
    cr = br;
    br = t;
  }
  out[0] = h1 + cl + dr;
  out[1] = h2 + dl + er;
  out[2] = h3 + el + ar;
  out[3] = h4 + al + br;
  out[4] = h0 + bl + cr;
}

// ---------------------------------------------------------------- public keys
// The compressed key of d (0 < d < n) as nine big-endian words (the 33 bytes
// 0x02 | (y & 1), x; the last word's low three bytes zero) and, with
// want_addr, its address (ripemd160_33's five words; addr is left alone
// otherwise).
template <class GTab>
CMTV_HD void secp_pubkey_one(uint32_t pkw[9], uint32_t addr[5], bool want_addr, const scn& d, const GTab& gt) {
  pt256 acc;
  pt_set_infinity(acc);
  secp_comb_add(acc, d, gt);
  fp x, y;
  pt_affine(x, &y, acc);
  uint32_t xw[8];
  fp_to_words(xw, x);
  const uint32_t prefix = 2u | (y.v[0] & 1u);
#pragma unroll
  for (int k = 0; k <= 8; k++) {
    const uint32_t prev = k == 0 ? prefix : xw[8 - k];
    const uint32_t cur = k < 8 ? xw[7 - k] : 0u;
    pkw[k] = (prev << 24) | (cur >> 8);
  }
  if (want_addr) {
    uint32_t st[8], w[16];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = i <= 8 ? pkw[i] : 0u;
    w[8] |= 0x00800000u;
    w[15] = 33u * 8u;
    sha256_iv(st);
    sha256_compress(st, w);
    ripemd160_33(addr, st);
  }
}

// ---------------------------------------------------------------- host side
// A private key's 32 big-endian bytes are in [1, n - 1]
inline bool secp_privkey_in_range(const uint8_t* priv) {
  uint32_t w[8];
  words_from_be32(w, priv);
  uint32_t o = 0;
  for (int i = 0; i < 8; i++) o |= w[i];
  return o != 0 && scn_words_less(w, [](int i) { return scn_n_word(i); });
}

// GenPrivKeySecp256k1 (secp256k1.go:107): (c mod (n - 1)) + 1 for the digest
// c (big-endian words), as 32 big-endian bytes. n - 1 > 2^255, so the
// remainder is c or c - (n - 1).
inline void secp_privkey_from_digest(uint8_t out[32], const uint32_t c[8]) {
  uint32_t w[8], d[8];
  for (int i = 0; i < 8; i++) w[i] = c[7 - i];
  // c - (n - 1) + 1 = c - n + 2 when c >= n - 1, else c + 1
  uint64_t borrow = 0, cy = 2;
  for (int i = 0; i < 8; i++) {
    const uint64_t t = (uint64_t)w[i] - scn_n_word(i) - borrow;
    d[i] = (uint32_t)t;
    borrow = (t >> 32) & 1;
  }
  // borrow: c < n. c = n - 1 is the one value below n that still wraps (to 1).
  bool is_nm1 = w[0] == scn_n_word(0) - 1;
  for (int i = 1; i < 8; i++) is_nm1 = is_nm1 && w[i] == scn_n_word(i);
  const bool wrap = borrow == 0 || is_nm1;
  if (!wrap) cy = 1;
  for (int i = 0; i < 8; i++) {
    cy += wrap ? d[i] : w[i];
    const uint32_t v = (uint32_t)cy;
    cy >>= 32;
    out[4 * (7 - i)] = (uint8_t)(v >> 24);
    out[4 * (7 - i) + 1] = (uint8_t)(v >> 16);
    out[4 * (7 - i) + 2] = (uint8_t)(v >> 8);
    out[4 * (7 - i) + 3] = (uint8_t)v;
  }
}

}  // namespace cmtv
