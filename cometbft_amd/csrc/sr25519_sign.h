// sr25519_sign.h -- sr25519 (schnorrkel over ristretto255) key derivation and
// signing, one key or signature per lane, for gfx950 (sr25519_sign.hip) and
// the host checker (tests/host/srsigncheck.cpp): the device form of the
// reference's PrivKey.PubKey and PrivKey.Sign (crypto/sr25519/privkey.go:25-61:
// NewMiniSecretKeyFromRaw -> ExpandEd25519 -> Sign) and PubKey.Address
// (pubkey.go:25). For synthetic test data: VARIABLE TIME (the fixed-base
// table rows are picked by secret digits).
//
// Byte contract (oracle/sr25519_ref.py expand_mini / pubkey_from_mini / sign):
//   private key  the 32-byte mini secret; h = SHA-512(mini)
//     key   = clamp(h[0:32]) >> 3   (h[0] &= 248, h[31] &= 63, h[31] |= 64;
//             in [2^251, 2^252): below L as it stands)
//     nonce = h[32:64]
//   public key   ristretto255 ENCODE([key]B)                  (RFC 9496 4.3.2)
//   address      SHA-256(public key)[:20]
//   signature    R || s, sig[63] |= 0x80 (schnorrkel's marker):
//     r = SHA-512("cmtverify/sr25519-witness" || nonce || msg) mod L
//     R = ENCODE([r]B)
//     k = the merlin challenge of NewSigningContext({}, msg) over pk and R
//         (merlin.h sr_transcript: the verifier's), mod L
//     s = k key + r mod L
// go-schnorrkel draws r from a transcript RNG seeded with OS randomness, so no
// Go signature's bytes can be reproduced and any r gives a valid signature:
// the witness above is this project's (the oracle's sign()), nothing of Go's.
//
// [key]B and [r]B are the helper waves' 16-position radix-2^16 comb over the
// shared fixed-base table (quad.h q_bcomb16: 16 mixed additions, no
// doublings; both scalars are below L as it asks).
#pragma once
#include "quad.h"
#include "sha256.h"
#include "sr25519.h"

namespace cmtv {

// RFC 9496 4.3.2 ENCODE of an extended point, any Z: the canonical 32 bytes
// of the point's coset (P, P + T for the four 4-torsion points T, encode
// alike). Computes on every input; selects, no branches, as ristretto_decode.
CMTV_HD void ristretto_encode(uint32_t out[8], const ge_p3& p) {
  fe u1, u2, t, one, invsqrt, den1, den2, z_inv, ix, iy, ench, i, x, y, den_inv, ny;
  fe_add(u1, p.Z, p.Y);
  fe_carry(u1);
  fe_sub(t, p.Z, p.Y);
  fe_carry(t);
  fe_mul(u1, u1, t);            // (Z + Y)(Z - Y)
  fe_mul(u2, p.X, p.Y);
  fe_sq(t, u2);
  fe_mul(t, t, u1);
  fe_1(one);
  (void)fe_sqrt_ratio_m1(invsqrt, one, t);  // 1/sqrt(u1 u2^2); 0 when x y = 0
  fe_mul(den1, invsqrt, u1);
  fe_mul(den2, invsqrt, u2);
  fe_mul(z_inv, den1, den2);
  fe_mul(z_inv, z_inv, p.T);
  fe_const_sqrtm1(i);
  fe_mul(ix, p.X, i);
  fe_mul(iy, p.Y, i);
  fe_const_invsqrt_amd(ench);
  fe_mul(ench, den1, ench);
  fe_mul(t, p.T, z_inv);
  const bool rotate = fe_isneg(t);
  fe_select(x, p.X, iy, rotate);
  fe_select(y, p.Y, ix, rotate);
  fe_select(den_inv, den2, ench, rotate);
  fe_mul(t, x, z_inv);
  fe_neg(ny, y);
  fe_carry(ny);
  fe_select(y, y, ny, fe_isneg(t));
  fe_sub(t, p.Z, y);
  fe_carry(t);
  fe_mul(t, den_inv, t);
  fe_neg(ny, t);
  fe_carry(ny);
  fe_select(t, t, ny, fe_isneg(t));  // CT_ABS
  fe_tobytes(out, t);
}

// MiniSecretKey.ExpandEd25519: key (8 little-endian words, < L) and nonce
CMTV_HD void sr_expand(uint32_t key[8], uint32_t nonce[8], const uint32_t mini[8]) {
  uint32_t h[16];
  sha512_prefixed<8>(h, mini, nullptr, 0);
  h[0] &= 0xFFFFFFF8u;
  h[7] = (h[7] & 0x3FFFFFFFu) | 0x40000000u;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    key[i] = (h[i] >> 3) | (i < 7 ? h[i + 1] << 29 : 0u);  // divideScalarByCofactor
    nonce[i] = h[8 + i];
  }
}

// SHA-256(pk)[:20] as five little-endian byte words
CMTV_HD void sr_address(uint32_t addr[5], const uint32_t pk[8]) {
  uint32_t st[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                    0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = i < 8 ? __builtin_bswap32(pk[i]) : 0u;
  w[8] = 0x80000000u;
  w[15] = 32u * 8u;
  sha256_compress(st, w);
#pragma unroll
  for (int i = 0; i < 5; i++) addr[i] = __builtin_bswap32(st[i]);
}

template <class BTab>
CMTV_HD void sr_pubkey_from_mini(uint32_t pk[8], const uint32_t mini[8], const BTab& btab) {
  uint32_t key[8], nonce[8];
  sr_expand(key, nonce, mini);
  ge_p3 A;
  q_bcomb16(A, key, btab);
  ristretto_encode(pk, A);
}

// The deterministic witness: SHA-512(label || nonce || msg) mod L. The label
// is 25 bytes, so the nonce sits one byte past a word.
CMTV_HD void sr_witness(uint32_t r[8], const uint32_t nonce[8], const uint8_t* msg, uint32_t mlen) {
  // "cmtverify/sr25519-witness"
  uint32_t pre[15] = {0x76746d63u, 0x66697265u, 0x72732f79u, 0x31353532u, 0x69772d39u, 0x73656e74u, 0x73u};
  pre[6] |= nonce[0] << 8;
#pragma unroll
  for (int i = 1; i < 8; i++) pre[6 + i] = (nonce[i - 1] >> 24) | (nonce[i] << 8);
  pre[14] = nonce[7] >> 24;
  uint32_t h[16];
  sha512_prefixed_bytes<57>(h, pre, msg, mlen);
  sc_reduce512(r, h);
}

// The signature of secret scalar `key` with witness r (both < L) under the
// encoded public key pk: R = ENCODE([r]B), s = k key + r, the marker bit.
// On the device every lane of the wave calls it together (sr_transcript).
template <class BTab, class State>
CMTV_HD void sr_sign_keyed(uint32_t sig[16], const uint32_t key[8], const uint32_t pk[8], const uint32_t r[8],
                           const uint8_t* msg, uint32_t mlen, const uint32_t* prog, int nops, State& st,
                           const BTab& btab) {
  uint32_t Rw[8];
  {
    ge_p3 R;
    q_bcomb16(R, r, btab);
    ristretto_encode(Rw, R);
  }
  uint32_t kb[16], k[8], s[8];
  sr_transcript(kb, st, prog, nops, msg, mlen, pk, Rw);
  sc_reduce512(k, kb);
  sc_muladd(s, k, key, r);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    sig[i] = Rw[i];
    sig[8 + i] = s[i];
  }
  sig[15] |= 0x80000000u;
}

// PrivKey.Sign with the deterministic witness. prog/nops: the transcript's
// prefix sponge (merlin.h sr_prefix_state).
template <class BTab, class State>
CMTV_HD void sr_sign_one(uint32_t sig[16], const uint32_t mini[8], const uint8_t* msg, uint32_t mlen,
                         const uint32_t* prog, int nops, State& st, const BTab& btab) {
  uint32_t key[8], nonce[8], pk[8], r[8];
  sr_expand(key, nonce, mini);
  {
    ge_p3 A;
    q_bcomb16(A, key, btab);
    ristretto_encode(pk, A);
  }
  sr_witness(r, nonce, msg, mlen);
  sr_sign_keyed(sig, key, pk, r, msg, mlen, prog, nops, st, btab);
}

}  // namespace cmtv
