// secp256k1.h -- ECDSA verification over secp256k1, one signature per lane:
// the device form of the reference's secp256k1.PubKey.VerifySignature
// (crypto/secp256k1/secp256k1.go:192-217; btcec v2.2.1 / dcrd underneath).
//
// Verdict for a 33-byte key pk, a 64-byte signature sig, a message msg:
//   1. pk[0] is 2 or 3; x = pk[1..33) big-endian, x < p (not reduced);
//      y^2 = x^3 + 7 is a square; y has the parity pk[0] & 1     -> Q
//   2. r = sig[0..32) mod n, s = sig[32..64) mod n (byte values >= n are
//      reduced: ModNScalar.SetByteSlice with its overflow flag ignored);
//      r != 0, s != 0, s <= (n - 1) / 2 (the lower-S rule)
//   3. e = SHA-256(msg) mod n
//   4. w = 1 / s; X = [e w]G + [r w]Q; X is not infinity and X.x mod n = r,
//      i.e. X.x = r, or X.x = r + n when r + n < p
// 33-byte compressed keys only: the 65-byte uncompressed and hybrid encodings
// btcec's ParsePubKey also takes never pass the reference's key codec
// (crypto/encoding/codec.go:53) and are not supported.
//
// Points are homogeneous projective (X : Y : Z), x = X / Z, infinity (0:1:0),
// with the COMPLETE addition and doubling formulas for a = 0 of Renes,
// Costello and Batina (Eurocrypt 2016, algorithms 7 and 9; b3 = 3 b = 21):
// secp256k1 has prime order, so they are correct for every pair of inputs --
// P + P, P + (-P), infinity on either side -- with no exceptional case to
// detect and no divergence. Inputs are adversarial (a key Q = [d]G with small
// d makes the accumulator meet a table entry equal to itself or to its
// negative); Jacobian formulas would compute garbage there.
// The final test needs no inversion: X.x = r <=> X = r Z.
//
// Scalar multiplication (the plain version: no GLV split):
//   [u2]Q : signed radix-16, digits in [-8, 8) from u2 + 0x88..8 read from the
//           top, plus a top carry digit in {0, 1}; 256 doublings, 64 additions
//           of a per-lane table (1..8)Q (8 x 30 words through the QTab policy:
//           lane-interleaved scratch on the device)
//   [u1]G : signed radix-256 comb, digits in [-128, 128) from u1 + 0x80..80,
//           plus a top carry; 33 additions from the fixed table
//           (1..128) [256^j]G, j = 0..32 (GTab policy), no doublings
//   registered keys (secp_verify_keyed_one): [u2]Q by the same comb over the
//           key's own table (1..128) [256^j]Q (secp_qcomb_position); with KB
//           signatures per lane sharing the inversion 1 / s
//           (secp_verify_keyed_batch_lane, for launches of many commits)
// Every lane does every step whatever its inputs (verification handles public
// data: this is for wave uniformity, not constant time); a failed check only
// clears the verdict.
//
// Magnitudes (fp256k1.h): coordinates out of pt_add are (3, 2, 2), out of
// pt_double (2, 2, 1); both accept (3, 3, 2) -- a table entry with Y negated.
#pragma once
#include <stdint.h>

#include "fp256k1.h"
#include "sc256k1.h"
#include "sha256.h"
#include "signbytes.h"

namespace cmtv {

struct pt256 {
  fp X, Y, Z;
};

constexpr int SECP_QTAB_ENTRIES = 8;
constexpr int SECP_PT_WORDS = 30;
constexpr int SECP_GTAB_POS = 33;          // 32 byte positions and the carry
constexpr int SECP_GTAB_PER_POS = 128;
constexpr int SECP_GTAB_ROW_WORDS = 32;    // X, Y, Z and two words of padding (16-byte rows)
constexpr int SECP_GTAB_ENTRIES = SECP_GTAB_POS * SECP_GTAB_PER_POS;

CMTV_HD void pt_set_infinity(pt256& r) {
  fp_set_small(r.X, 0);
  fp_set_small(r.Y, 1);
  fp_set_small(r.Z, 0);
}

CMTV_HD void pt_set_generator(pt256& r) {
  const uint32_t gx[8] = {0x16F81798u, 0x59F2815Bu, 0x2DCE28D9u, 0x029BFCDBu,
                          0xCE870B07u, 0x55A06295u, 0xF9DCBBACu, 0x79BE667Eu};
  const uint32_t gy[8] = {0xFB10D4B8u, 0x9C47D08Fu, 0xA6855419u, 0xFD17B448u,
                          0x0E1108A8u, 0x5DA4FBFCu, 0x26A3C465u, 0x483ADA77u};
  fp_from_words(r.X, gx);
  fp_from_words(r.Y, gy);
  fp_set_small(r.Z, 1);
}

// r = p + q for any p, q on the curve (RCB algorithm 7). Input magnitudes up
// to (3, 3, 2) each; output (3, 2, 2). r may alias p or q.
CMTV_HD void pt_add(pt256& r, const pt256& p, const pt256& q) {
  fp t0, t1, t2, t3, t4, x3, y3, z3;
  fp_mul(t0, p.X, q.X);        // 1
  fp_mul(t1, p.Y, q.Y);        // 1
  fp_mul(t2, p.Z, q.Z);        // 1
  fp_add(t3, p.X, p.Y);        // <= 6
  fp_add(t4, q.X, q.Y);        // <= 6
  fp_mul(t3, t3, t4);          // 1
  fp_add(t4, t0, t1);          // 2
  fp_sub(t3, t3, t4, 2);       // 4
  fp_add(t4, p.Y, p.Z);        // <= 5
  fp_add(x3, q.Y, q.Z);        // <= 5
  fp_mul(t4, t4, x3);          // 1
  fp_add(x3, t1, t2);          // 2
  fp_sub(t4, t4, x3, 2);       // 4
  fp_add(x3, p.X, p.Z);        // <= 5
  fp_add(y3, q.X, q.Z);        // <= 5
  fp_mul(x3, x3, y3);          // 1
  fp_add(y3, t0, t2);          // 2
  fp_sub(y3, x3, y3, 2);       // 4
  fp_add(x3, t0, t0);          // 2
  fp_add(t0, x3, t0);          // 3
  fp_mul_small(t2, t2, 21);    // 1
  fp_add(z3, t1, t2);          // 2
  fp_sub(t1, t1, t2, 1);       // 3
  fp_mul_small(y3, y3, 21);    // 1
  fp_mul(x3, t4, y3);          // 1
  fp_mul(t2, t3, t1);          // 1
  fp_sub(r.X, t2, x3, 1);      // 3
  fp_mul(y3, y3, t0);          // 1
  fp_mul(t1, t1, z3);          // 1
  fp_add(r.Y, t1, y3);         // 2
  fp_mul(t0, t0, t3);          // 1
  fp_mul(z3, z3, t4);          // 1
  fp_add(r.Z, z3, t0);         // 2
}

// r = 2 p (RCB algorithm 9). Input up to (3, 3, 2); output (2, 2, 1).
CMTV_HD void pt_double(pt256& r, const pt256& p) {
  fp t0, t1, t2, x3, y3, z3;
  fp_sq(t0, p.Y);              // 1
  fp_add(z3, t0, t0);          // 2
  fp_add(z3, z3, z3);          // 4
  fp_add(z3, z3, z3);          // 8
  fp_mul(t1, p.Y, p.Z);        // 1
  fp_sq(t2, p.Z);              // 1
  fp_mul_small(t2, t2, 21);    // 1
  fp_mul(x3, t2, z3);          // 1
  fp_add(y3, t0, t2);          // 2
  fp_mul(r.Z, t1, z3);         // 1
  fp_add(t1, t2, t2);          // 2
  fp_add(t2, t1, t2);          // 3
  fp_sub(t0, t0, t2, 3);       // 5
  fp_mul(y3, t0, y3);          // 1
  fp_add(y3, x3, y3);          // 2
  fp_mul(t1, p.X, p.Y);        // 1
  fp_mul(x3, t0, t1);          // 1
  fp_add(r.X, x3, x3);         // 2
  r.Y = y3;
}

// q with Y negated when neg, infinity when zero (q of magnitude (3, 2, 2))
CMTV_HD void pt_signed_or_infinity(pt256& q, bool neg, bool zero) {
  fp ny, one;
  fp_neg(ny, q.Y, 2);  // 3
  fp_select(q.Y, q.Y, ny, neg);
  fp_set_small(one, 1);
  fp_select(q.Y, q.Y, one, zero);
#pragma unroll
  for (int i = 0; i < 10; i++) {
    q.X.v[i] = zero ? 0u : q.X.v[i];
    q.Z.v[i] = zero ? 0u : q.Z.v[i];
  }
}

// Row (j, d) of the fixed table: [d 256^j]G, d = 1..128, as 30 limb words
// (X, Y, Z) and two zero words. One row per thread when the runtime builds
// the table (secp256k1.hip k_secp_gtab_build); tests/host builds it the same way.
CMTV_HD void secp_gtab_row(uint32_t out[SECP_GTAB_ROW_WORDS], int j, int d) {
  pt256 g, acc, t;
  pt_set_generator(g);
  pt_set_infinity(acc);
#pragma unroll 1
  for (int b = 7; b >= 0; b--) {
    pt_double(acc, acc);
    t = g;
    pt_signed_or_infinity(t, false, ((d >> b) & 1) == 0);
    pt_add(acc, acc, t);
  }
#pragma unroll 1
  for (int k = 0; k < 8 * j; k++) pt_double(acc, acc);
#pragma unroll
  for (int i = 0; i < 10; i++) {
    out[i] = acc.X.v[i];
    out[10 + i] = acc.Y.v[i];
    out[20 + i] = acc.Z.v[i];
  }
  out[30] = out[31] = 0;
}

// Parses a 33-byte compressed key into q (affine, Z = 1); false when the key
// is rejected (q is then some point or garbage the caller's verdict ignores).
CMTV_HD bool secp_parse_pubkey(pt256& q, const uint8_t* pk) {
  const uint32_t prefix = pk[0];
  uint32_t xw[8];
  words_from_be32(xw, pk + 1);
  bool ok = prefix == 2 || prefix == 3;
  // x < p = 2^256 - 2^32 - 977
  ok = ok && scn_words_less(xw, [](int i) { return i == 0 ? 0xFFFFFC2Fu : i == 1 ? 0xFFFFFFFEu : 0xFFFFFFFFu; });
  fp x, y, y2, t;
  fp_from_words(x, xw);
  fp_sq(t, x);
  fp_mul(y2, t, x);
  fp_set_small(t, 7);
  fp_add(y2, y2, t);  // 2
  fp_sqrt_candidate(y, y2);
  fp_sq(t, y);
  ok = ok && fp_equal(t, y2);
  fp_normalize(y);
  fp_neg(t, y, 1);  // 2
  fp_select(y, y, t, (y.v[0] & 1) != (prefix & 1));
  q.X = x;
  q.Y = y;
  fp_set_small(q.Z, 1);
  return ok;
}

// Step 2: r and s from the signature's bytes, reduced; false when r or s is
// zero or s is above (n - 1) / 2 (the scalars are then still defined: every
// lane goes on).
CMTV_HD bool secp_sig_scalars(scn& r, scn& s, const uint8_t* sig) {
  uint32_t rw[8], sw[8];
  words_from_be32(rw, sig);
  words_from_be32(sw, sig + 32);
  scn_from_words(r, rw);
  scn_from_words(s, sw);
  return !scn_is_zero(r) && !scn_is_zero(s) && !scn_over_half(s);
}

// Step 3: e = SHA-256(msg) mod n
CMTV_HD void secp_msg_scalar(scn& e, const uint8_t* msg, uint32_t mlen) {
  uint32_t h[8], hw[8];
  sha256_msg(h, msg, mlen);
#pragma unroll
  for (int i = 0; i < 8; i++) hw[i] = h[7 - i];
  scn_from_words(e, hw);
}

// The products of step 4 for a given w = 1 / s: u1 = e w, u2 = r w
CMTV_HD void secp_u1_u2(scn& u1, scn& u2, const scn& e, const scn& r, const scn& w) {
  scn_mul(u1, e, w);
  scn_mul(u2, r, w);
}

// The checks and scalars every verdict starts with (steps 2 and 3 and the
// inversion of step 4): r, u1 = e / s, u2 = r / s; the verdict of
// secp_sig_scalars.
CMTV_HD bool secp_scalars(scn& r, scn& u1, scn& u2, const uint8_t* sig, const uint8_t* msg, uint32_t mlen) {
  scn s, e, w;
  const bool ok = secp_sig_scalars(r, s, sig);
  secp_msg_scalar(e, msg, mlen);
  scn_invert(w, s);
  secp_u1_u2(u1, u2, e, r, w);
  return ok;
}

// acc += [u]B for a scalar u < n and the comb table tab of B, rows (j, d) =
// [d 256^j]B: the bytes of u + 0x80..80 read from the bottom, each minus 128,
// are the signed digits of positions 0..31, and the carry out of bit 255 is
// the digit of position 32. 33 additions, no doublings.
template <class Tab>
CMTV_HD void secp_comb_add(pt256& acc, const scn& u, const Tab& tab) {
  uint32_t d[8];
  uint64_t cy = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    cy += (uint64_t)u.v[i] + 0x80808080u;
    d[i] = (uint32_t)cy;
    cy >>= 32;
  }
  pt256 t;
#pragma unroll 1
  for (int j = 0; j < 32; j++) {
    const int dg = (int)(d[0] & 0xFF) - 128;
#pragma unroll
    for (int k = 0; k < 7; k++) d[k] = (d[k] >> 8) | (d[k + 1] << 24);
    d[7] >>= 8;
    const int mag = dg < 0 ? -dg : dg;
    tab.load(j * SECP_GTAB_PER_POS + (mag ? mag - 1 : 0), t);
    pt_signed_or_infinity(t, dg < 0, mag == 0);
    pt_add(acc, acc, t);
  }
  tab.load(32 * SECP_GTAB_PER_POS, t);
  pt_signed_or_infinity(t, false, cy == 0);
  pt_add(acc, acc, t);
}

// The last step of every verdict: acc is not infinity and acc.x mod n = r,
// without an inversion: X = r Z, or X = (r + n) Z when r + n < p
CMTV_HD bool secp_x_is_r(const pt256& acc, const scn& r) {
  fp fr, rz;
  fp_from_words(fr, r.v);
  fp_mul(rz, fr, acc.Z);
  const bool eq1 = fp_equal(acc.X, rz);
  const bool wraps = scn_words_less(r.v, [](int i) { return scn_pmn_word(i); });
  uint32_t rn[8];
  uint64_t cy = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    cy += (uint64_t)r.v[i] + scn_n_word(i);
    rn[i] = (uint32_t)cy;
    cy >>= 32;
  }
  fp_from_words(fr, rn);
  fp_mul(rz, fr, acc.Z);
  const bool eq2 = wraps && fp_equal(acc.X, rz);
  return !fp_is_zero(acc.Z) && (eq1 || eq2);
}

// The whole verdict. QTab: store(e, pt) / load(e, pt), e = 0..7, this lane's
// table of (e + 1)Q. GTab: load(row, pt), the fixed table's rows.
template <class QTab, class GTab>
CMTV_HD bool secp_verify_one(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, uint32_t mlen, QTab& qt,
                             const GTab& gt) {
  pt256 q;
  bool ok = secp_parse_pubkey(q, pk);
  scn r, u1, u2;
  ok = secp_scalars(r, u1, u2, sig, msg, mlen) && ok;

  // the lane's table (1..8)Q
  pt256 acc = q, t;
  qt.store(0, acc);
#pragma unroll 1
  for (int k = 1; k < SECP_QTAB_ENTRIES; k++) {
    pt_add(acc, acc, q);
    qt.store(k, acc);
  }

  // [u2]Q: digits of u2 + 0x88..8, most significant first
  uint32_t d2[8];
  uint64_t cy = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    cy += (uint64_t)u2.v[i] + 0x88888888u;
    d2[i] = (uint32_t)cy;
    cy >>= 32;
  }
  qt.load(0, acc);
  pt_signed_or_infinity(acc, false, cy == 0);
#pragma unroll 1
  for (int i = 0; i < 64; i++) {
    const int dg = (int)(d2[7] >> 28) - 8;
#pragma unroll
    for (int k = 7; k > 0; k--) d2[k] = (d2[k] << 4) | (d2[k - 1] >> 28);
    d2[0] <<= 4;
    pt_double(acc, acc);
    pt_double(acc, acc);
    pt_double(acc, acc);
    pt_double(acc, acc);
    const int mag = dg < 0 ? -dg : dg;
    qt.load(mag ? mag - 1 : 0, t);
    pt_signed_or_infinity(t, dg < 0, mag == 0);
    pt_add(acc, acc, t);
  }

  // [u1]G: the comb over the fixed table
  secp_comb_add(acc, u1, gt);
  return secp_x_is_r(acc, r) && ok;
}

#ifdef __HIPCC__
// The GTab policy of the kernels (secp256k1.hip, secp256k1_sign.hip): the
// fixed table's, or a registered key's, 32-word rows gathered with dwordx4 loads
struct DevSecpGTab {
  const uint32_t* __restrict__ rows;
  __device__ __forceinline__ void load(int row, pt256& p) const {
    const uint4* q = reinterpret_cast<const uint4*>(rows + (size_t)row * SECP_GTAB_ROW_WORDS);
    uint32_t w[32];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const uint4 v = q[k];
      w[4 * k] = v.x;
      w[4 * k + 1] = v.y;
      w[4 * k + 2] = v.z;
      w[4 * k + 3] = v.w;
    }
#pragma unroll
    for (int i = 0; i < 10; i++) {
      p.X.v[i] = w[i];
      p.Y.v[i] = w[10 + i];
      p.Z.v[i] = w[20 + i];
    }
  }
};
#endif

// ---------------------------------------------------------------- registered keys
// A registered key Q has a comb table of its own in the fixed table's layout:
// row (j, d) = [d 256^j]Q, j = 0..32, d = 1..128 (528 KiB per key). [u2]Q is
// then 33 additions like [u1]G: no decompression, no per-lane table, no
// doublings and no scratch.

// Rows (j, 1..128) of the comb of the key pk, SECP_GTAB_PER_POS rows of
// SECP_GTAB_ROW_WORDS words at rows: the key parsed, 8 j doublings to
// B = [256^j]Q, then d B by repeated addition. The rows' magnitudes are the
// ones pt_signed_or_infinity and pt_add take: (1, 2, 1) for Q itself,
// (2, 2, 1) out of pt_double, (3, 2, 2) out of pt_add. A rejected key
// (secp_parse_pubkey) gets the point at infinity (0 : 1 : 0) in every row;
// returns whether the key was accepted. One thread per (key, j) when the
// runtime registers keys (secp256k1.hip k_secp_qcomb_build); tests/host
// builds tables the same way.
CMTV_HD bool secp_qcomb_position(uint32_t* rows, const uint8_t* pk, int j) {
  pt256 base, acc;
  const bool ok = secp_parse_pubkey(base, pk);
  pt_signed_or_infinity(base, false, !ok);
#pragma unroll 1
  for (int k = 0; k < 8 * j; k++) pt_double(base, base);
  acc = base;
#pragma unroll 1
  for (int d = 1; d <= SECP_GTAB_PER_POS; d++) {
    uint32_t* out = rows + (size_t)(d - 1) * SECP_GTAB_ROW_WORDS;
#pragma unroll
    for (int i = 0; i < 10; i++) {
      out[i] = ok ? acc.X.v[i] : 0u;
      out[10 + i] = ok ? acc.Y.v[i] : (i == 0 ? 1u : 0u);
      out[20 + i] = ok ? acc.Z.v[i] : 0u;
    }
    out[30] = out[31] = 0;
    pt_add(acc, acc, base);
  }
  return ok;
}

// The verdict for a registered key: key_ok and qt from the key's table
// (secp_qcomb_position), gt the fixed table. One accumulator takes the 33
// additions of [u1]G and then the 33 of [u2]Q. (Two accumulators joined by a
// 67th addition, for independent work within the one wave per SIMD of a small
// batch, measured 1% slower at 10,000 and at 200,000 signatures and took 252
// VGPRs for 198: DESIGN 4.6b.)
template <class QTab, class GTab>
CMTV_HD bool secp_verify_keyed_one(bool key_ok, const uint8_t* sig, const uint8_t* msg, uint32_t mlen, const QTab& qt,
                                   const GTab& gt) {
  scn r, u1, u2;
  const bool ok = secp_scalars(r, u1, u2, sig, msg, mlen) && key_ok;
  pt256 acc;
  pt_set_infinity(acc);
  secp_comb_add(acc, u1, gt);
  secp_comb_add(acc, u2, qt);
  return secp_x_is_r(acc, r) && ok;
}

// ---------------------------------------------------------------- templated sign-bytes
// Commit signatures: the lane writes its own message, the CanonicalVote of
// its signature from the commit's template (signbytes.h sb_write: flag,
// seconds and nanos are the signature's), into `slot` through `out` -- a
// byte writer over slot, the lane's LDS slot on the device -- and hashes it
// from there: sha256_msg reads only words that hold message bytes, so the
// lane reads nothing it did not write. The caller has checked that the
// message fits the slot. The verdict is secp_verify_one's / keyed_one's over
// those bytes.
template <class Out, class QTab, class GTab>
CMTV_HD bool secp_verify_tmpl_one(const uint8_t* pk, const uint8_t* sig, Out& out, const uint8_t* slot,
                                  const SbTemplate& t, const uint8_t* blob, bool commit_flag, int64_t sec,
                                  int32_t nanos, QTab& qt, const GTab& gt) {
  const uint32_t ml = sb_write(out, t, blob, commit_flag, sec, nanos);
  return secp_verify_one(pk, sig, slot, ml, qt, gt);
}

template <class Out, class QTab, class GTab>
CMTV_HD bool secp_verify_keyed_tmpl_one(bool key_ok, const uint8_t* sig, Out& out, const uint8_t* slot,
                                        const SbTemplate& t, const uint8_t* blob, bool commit_flag, int64_t sec,
                                        int32_t nanos, const QTab& qt, const GTab& gt) {
  const uint32_t ml = sb_write(out, t, blob, commit_flag, sec, nanos);
  return secp_verify_keyed_one(key_ok, sig, slot, ml, qt, gt);
}

// ---------------------------------------------------------------- KB signatures per lane
// Registered-key verification with KB signatures per lane sharing one
// inversion mod n (Montgomery's trick: one scn_invert and 3 (KB - 1) scalar
// products instead of KB inversions; 1/s is 63k of a keyed verification's
// 144k multiply-adds, a scalar product 139).
//
// Src gives the lane its rounds: active(r), sig(r) (64 bytes; an inactive
// round's are some signature's), key(r, qt) (whether the key is in the set
// and accepted; qt its table), message(r, msg) (the round's message, written
// by the lane itself on the device: its length) and verdict(r, v). Pre holds
// the lane's KB running products: store(r, x) / load(r, x).
//
// Pass 1, per round: r and s and the checks of secp_sig_scalars; the running
// product of the s values, where a zero s and an inactive round enter as 1 so
// they cannot spoil the lane's other signatures (their verdicts are false by
// the ok bit). One inversion. Pass 2, rounds descending: w = 1 / s_r from
// the inverse and the product before it, then what secp_verify_keyed_one
// does with it. Scalars are always fully reduced (sc256k1.h), so w, u1 and u2
// are the words the one-signature form computes, and so are the accumulator
// and the verdict. (s = 0 there gives w = 0 and the point at infinity: false
// too.)
CMTV_HD void secp_batch_s(scn& s, bool active) {
  const bool one = !active || scn_is_zero(s);
#pragma unroll
  for (int i = 0; i < 8; i++) s.v[i] = one ? (i == 0 ? 1u : 0u) : s.v[i];
}

template <int KB, class Src, class Pre, class GTab>
CMTV_HD void secp_verify_keyed_batch_lane(Src& src, Pre& pre, const GTab& gt) {
  uint32_t okbits = 0;
  scn prod;
#pragma unroll 1
  for (int r = 0; r < KB; r++) {
    scn rr, s;
    const bool active = src.active(r);
    const bool ok = secp_sig_scalars(rr, s, src.sig(r)) && active;
    okbits |= (ok ? 1u : 0u) << r;
    secp_batch_s(s, active);
    if (r == 0)
      prod = s;
    else
      scn_mul(prod, prod, s);
    pre.store(r, prod);
  }
  scn inv;
  scn_invert(inv, prod);
#pragma unroll 1
  for (int r = KB - 1; r >= 0; r--) {
    scn rr, s, w;
    (void)secp_sig_scalars(rr, s, src.sig(r));
    secp_batch_s(s, src.active(r));
    if (r > 0) {
      scn before;
      pre.load(r - 1, before);
      scn_mul(w, inv, before);  // 1 / s_r
      scn_mul(inv, inv, s);     // 1 / (s_0 ... s_{r-1})
    } else {
      w = inv;
    }
    typename Src::QTab qt;
    const bool key_ok = src.key(r, qt);
    const uint8_t* msg;
    const uint32_t ml = src.message(r, msg);
    scn e, u1, u2;
    secp_msg_scalar(e, msg, ml);
    secp_u1_u2(u1, u2, e, rr, w);
    pt256 acc;
    pt_set_infinity(acc);
    secp_comb_add(acc, u1, gt);
    secp_comb_add(acc, u2, qt);
    src.verdict(r, secp_x_is_r(acc, rr) && key_ok && ((okbits >> r) & 1u) != 0);
  }
}

}  // namespace cmtv
