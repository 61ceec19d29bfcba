// Stand-alone checker of the device-only code paths: the product headers'
// __HIP_DEVICE_COMPILE__ branches, the DevRow inline-asm products and row
// moves (row_dev.h) and the DevQuad / DevOct DPP blocks (devtables.h), one
// small kernel per primitive, and the verdicts' rejection rules one function
// at a time (ristretto_decode, fe_sqrt_ratio_m1: sr25519.h; secp_parse_pubkey,
// secp_sig_scalars, secp_x_is_r, pt_add, pt_double: secp256k1.h). It links
// nothing of libcmtverify.so and holds no verdict logic of its own:
// tests/test_device_primitives_gpu.py builds the cases, and compares the raw
// results with Python integers.
//
//   devcheck <op>
//   stdin:  u32 n, u32 blob_bytes, n x IN u32 (one record per thread, or per
//           GROUP threads), then blob_bytes of message bytes (the hashes)
//   stdout: n x OUT u32
// Threads are padded with zero records to whole blocks, so every wave runs
// with all 64 lanes live (the row and quad moves read neighbouring lanes).
// Launch shapes are the product kernels': 64 threads for lane ops, 256 for
// row and quad ops. Any HIP error ends the program with a non-zero status
// before anything else is launched.
//
// g++ -x c++ -DDEVCHECK_HOST builds the ops that need no lane exchange as
// plain loops (tests/test_device_primitives_host.py): the same case sets and
// Python references are checked on a CPU first.
#ifdef DEVCHECK_HOST
#define CMTV_HD inline
#define DC_FN inline
#else
#include <hip/hip_runtime.h>
#define DC_FN __device__ __forceinline__
#endif
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../cometbft_amd/csrc/fe25519.h"
#include "../../cometbft_amd/csrc/ge25519.h"
#include "../../cometbft_amd/csrc/sc25519.h"
#include "../../cometbft_amd/csrc/sha512.h"
#include "../../cometbft_amd/csrc/keccak.h"
#include "../../cometbft_amd/csrc/halfscalar.h"
#include "../../cometbft_amd/csrc/quad.h"
#include "../../cometbft_amd/csrc/oct.h"
#include "../../cometbft_amd/csrc/row.h"
#include "../../cometbft_amd/csrc/sr25519.h"
#include "../../cometbft_amd/csrc/secp256k1.h"
#ifndef DEVCHECK_HOST
#include "../../cometbft_amd/csrc/row_dev.h"
#include "../../cometbft_amd/csrc/devtables.h"
#endif

using namespace cmtv;

static DC_FN void ld_fe(fe& f, const uint32_t* p) {
  for (int i = 0; i < 10; i++) f.v[i] = p[i];
}
static DC_FN void st_fe(uint32_t* p, const fe& f) {
  for (int i = 0; i < 10; i++) p[i] = f.v[i];
}

// An op: IN / OUT words per record, BLOCK threads per workgroup, GROUP
// threads per record (64: one record per wave, for wave-uniform code).
#define DC_OP(NAME, IN_, OUT_, BLOCK_, GROUP_)                        \
  struct NAME {                                                       \
    static constexpr int IN = IN_, OUT = OUT_, BLOCK = BLOCK_, GROUP = GROUP_; \
    static DC_FN void run(const uint32_t* in, uint32_t* o, const uint8_t* blob); \
  };                                                                  \
  DC_FN void NAME::run(const uint32_t* in, uint32_t* o, const uint8_t* blob)

// ---- lane field layer (fe25519.h) ---------------------------------------------
DC_OP(op_fe_mul, 20, 10, 64, 1) {
  fe f, g, h;
  ld_fe(f, in);
  ld_fe(g, in + 10);
  fe_mul(h, f, g);
  st_fe(o, h);
}
DC_OP(op_fe_sq, 10, 10, 64, 1) {
  fe f, h;
  ld_fe(f, in);
  fe_sq(h, f);
  st_fe(o, h);
}
template <int N>
struct op_fe_sqn {
  static constexpr int IN = 10, OUT = 10, BLOCK = 64, GROUP = 1;
  static DC_FN void run(const uint32_t* in, uint32_t* o, const uint8_t*) {
    fe f, h;
    ld_fe(f, in);
    fe_sqn(h, f, N);
    st_fe(o, h);
  }
};
DC_OP(op_fe_carry, 10, 10, 64, 1) {
  fe f;
  ld_fe(f, in);
  fe_carry(f);
  st_fe(o, f);
}
// (f + g) k, (f - g) k, (-g) k
DC_OP(op_fe_lin, 30, 30, 64, 1) {
  fe f, g, k, t, h;
  ld_fe(f, in);
  ld_fe(g, in + 10);
  ld_fe(k, in + 20);
  fe_add(t, f, g);
  fe_mul(h, t, k);
  st_fe(o, h);
  fe_sub(t, f, g);
  fe_mul(h, t, k);
  st_fe(o + 10, h);
  fe_neg(t, g);
  fe_mul(h, t, k);
  st_fe(o + 20, h);
}
DC_OP(op_fe_frombytes, 8, 10, 64, 1) {
  uint32_t w[8];
  for (int i = 0; i < 8; i++) w[i] = in[i];
  fe h;
  fe_frombytes(h, w);
  st_fe(o, h);
}
// canonical bytes, iszero, isneg
DC_OP(op_fe_canon, 10, 10, 64, 1) {
  fe f;
  ld_fe(f, in);
  uint32_t s[8];
  fe_tobytes(s, f);
  for (int i = 0; i < 8; i++) o[i] = s[i];
  o[8] = fe_iszero(f) ? 1u : 0u;
  o[9] = fe_isneg(f) ? 1u : 0u;
}
DC_OP(op_fe_equal, 20, 1, 64, 1) {
  fe f, g;
  ld_fe(f, in);
  ld_fe(g, in + 10);
  o[0] = fe_equal(f, g) ? 1u : 0u;
}
// z^(p-2), z^((p-5)/8)
DC_OP(op_fe_pow, 10, 20, 64, 1) {
  fe z, h;
  ld_fe(z, in);
  fe_invert(h, z);
  st_fe(o, h);
  fe_pow22523(h, z);
  st_fe(o + 10, h);
}

// ---- scalars and hashes ---------------------------------------------------------
DC_OP(op_sc_reduce512, 16, 8, 64, 1) {
  uint32_t x[16], r[8];
  for (int i = 0; i < 16; i++) x[i] = in[i];
  sc_reduce512(r, x);
  for (int i = 0; i < 8; i++) o[i] = r[i];
}
DC_OP(op_sc_is_canonical, 8, 1, 64, 1) {
  uint32_t s[8];
  for (int i = 0; i < 8; i++) s[i] = in[i];
  o[0] = sc_is_canonical(s) ? 1u : 0u;
}
DC_OP(op_sc_muladd, 24, 8, 64, 1) {
  uint32_t a[8], b[8], c[8], r[8];
  for (int i = 0; i < 8; i++) {
    a[i] = in[i];
    b[i] = in[8 + i];
    c[i] = in[16 + i];
  }
  sc_muladd(r, a, b, c);
  for (int i = 0; i < 8; i++) o[i] = r[i];
}
static DC_FN void st_half(uint32_t* o, const HalfScalars& h) {
  for (int i = 0; i < 8; i++) {
    o[i] = h.k1[i];
    o[8 + i] = h.k2[i];
  }
  // tests/host/halfcheck.cpp's flag byte
  o[16] = (h.k2_neg ? 1u : 0u) | (h.wide ? 2u : 0u) | ((uint32_t)(h.windows - 32) << 2);
}
// in: k[8], odd_k2
DC_OP(op_half, 9, 17, 64, 1) {
  uint32_t k[8];
  for (int i = 0; i < 8; i++) k[i] = in[i];
  HalfScalars h;
  half_scalars<true, false>(h, k, false, in[8] != 0);
  st_half(o, h);
}
// in: a, b (< 2^31, b > 0), x. out: hs_udiv31(a, b), hs_clz(x)
DC_OP(op_hs_prims, 3, 2, 64, 1) {
  o[0] = hs_udiv31(in[0], in[1]);
  o[1] = (uint32_t)hs_clz(in[2]);
}
template <int PW>
struct op_sha512 {
  // in: message offset in the blob, message length, prefix words
  static constexpr int IN = 2 + PW, OUT = 16, BLOCK = 64, GROUP = 1;
  static DC_FN void run(const uint32_t* in, uint32_t* o, const uint8_t* blob) {
    uint32_t pre[PW], out[16];
    for (int i = 0; i < PW; i++) pre[i] = in[2 + i];
    sha512_prefixed<PW>(out, pre, blob + in[0], in[1]);
    for (int i = 0; i < 16; i++) o[i] = out[i];
  }
};
DC_OP(op_keccak, 50, 50, 64, 1) {
  uint64_t a[25];
  for (int i = 0; i < 25; i++) a[i] = in[2 * i] | ((uint64_t)in[2 * i + 1] << 32);
  keccak_f1600(a);
  for (int i = 0; i < 25; i++) {
    o[2 * i] = (uint32_t)a[i];
    o[2 * i + 1] = (uint32_t)(a[i] >> 32);
  }
}

// ---- the verdicts' rejection rules (sr25519.h, secp256k1.h) ---------------------------
static DC_FN void st_fe_bytes(uint32_t* o, const fe& f) {
  uint32_t s[8];
  fe_tobytes(s, f);
  for (int i = 0; i < 8; i++) o[i] = s[i];
}
// in: the encoding's 8 words. out: verdict, canonical X, Y, T
DC_OP(op_ristretto_decode, 8, 25, 64, 1) {
  uint32_t w[8];
  for (int i = 0; i < 8; i++) w[i] = in[i];
  ge_p3 h;
  o[0] = ristretto_decode(h, w) ? 1u : 0u;
  st_fe_bytes(o + 1, h.X);
  st_fe_bytes(o + 9, h.Y);
  st_fe_bytes(o + 17, h.T);
}
// in: u, v (carried limbs). out: was_square, canonical r
DC_OP(op_sqrt_ratio_m1, 20, 9, 64, 1) {
  fe u, v, r;
  ld_fe(u, in);
  ld_fe(v, in + 10);
  o[0] = fe_sqrt_ratio_m1(r, u, v) ? 1u : 0u;
  st_fe_bytes(o + 1, r);
}
static DC_FN void ld_fp(fp& f, const uint32_t* p) {
  for (int i = 0; i < 10; i++) f.v[i] = p[i];
}
static DC_FN void st_fp_words(uint32_t* o, fp a) {
  uint32_t w[8];
  fp_normalize(a);
  fp_to_words(w, a);
  for (int i = 0; i < 8; i++) o[i] = w[i];
}
// in: the key's 33 bytes in 9 words. out: verdict, x, y normalised
DC_OP(op_secp_parse_pubkey, 9, 17, 64, 1) {
  uint8_t pk[33];
  for (int i = 0; i < 33; i++) pk[i] = (uint8_t)(in[i >> 2] >> (8 * (i & 3)));
  pt256 q;
  o[0] = secp_parse_pubkey(q, pk) ? 1u : 0u;
  st_fp_words(o + 1, q.X);
  st_fp_words(o + 9, q.Y);
}
// in: the signature's 64 bytes. out: verdict, r, s
DC_OP(op_secp_sig_scalars, 16, 17, 64, 1) {
  uint8_t sig[64];
  for (int i = 0; i < 64; i++) sig[i] = (uint8_t)(in[i >> 2] >> (8 * (i & 3)));
  scn r, s;
  o[0] = secp_sig_scalars(r, s, sig) ? 1u : 0u;
  for (int i = 0; i < 8; i++) {
    o[1 + i] = r.v[i];
    o[9 + i] = s.v[i];
  }
}
static DC_FN void ld_pt(pt256& p, const uint32_t* in) {
  ld_fp(p.X, in);
  ld_fp(p.Y, in + 10);
  ld_fp(p.Z, in + 20);
}
// the raw limbs of X, Y, Z, then fp_within(X, mx) | fp_within(Y, my) << 1 | fp_within(Z, mz) << 2
static DC_FN void st_pt(uint32_t* o, const pt256& p, uint32_t mx, uint32_t my, uint32_t mz) {
  for (int i = 0; i < 10; i++) {
    o[i] = p.X.v[i];
    o[10 + i] = p.Y.v[i];
    o[20 + i] = p.Z.v[i];
  }
  o[30] = (fp_within(p.X, mx) ? 1u : 0u) | (fp_within(p.Y, my) ? 2u : 0u) | (fp_within(p.Z, mz) ? 4u : 0u);
}
// in: the accumulator's limbs (X, Y, Z), r (8 words, below n). out: secp_x_is_r
DC_OP(op_secp_x_is_r, 38, 1, 64, 1) {
  pt256 acc;
  ld_pt(acc, in);
  scn r;
  for (int i = 0; i < 8; i++) r.v[i] = in[30 + i];
  o[0] = secp_x_is_r(acc, r) ? 1u : 0u;
}
// in: p, q limbs. out: p + q limbs, its magnitudes within (3, 2, 2)
DC_OP(op_pt_add, 60, 31, 64, 1) {
  pt256 p, q, r;
  ld_pt(p, in);
  ld_pt(q, in + 30);
  pt_add(r, p, q);
  st_pt(o, r, 3, 2, 2);
}
// in: p limbs. out: 2 p limbs, its magnitudes within (2, 2, 1)
DC_OP(op_pt_double, 30, 31, 64, 1) {
  pt256 p, r;
  ld_pt(p, in);
  pt_double(r, p);
  st_pt(o, r, 2, 2, 1);
}

#ifndef DEVCHECK_HOST
// every lane of a wave holds the record's scalar (the row kernels' helper
// waves): k1, k2, flags of lane 0, then whether all 64 lanes agree
DC_OP(op_half_uni, 9, 18, 64, 64) {
  uint32_t k[8];
  for (int i = 0; i < 8; i++) k[i] = in[i];
  HalfScalars h;
  half_scalars<true, true>(h, k, false, in[8] != 0);
  uint32_t w[17];
  st_half(w, h);
  bool same = true;
  for (int i = 0; i < 17; i++) same = same && w[i] == (uint32_t)__builtin_amdgcn_readfirstlane((int)w[i]);
  const bool all = __ballot(!same) == 0;
  if ((threadIdx.x & 63) == 0) {
    for (int i = 0; i < 17; i++) o[i] = w[i];
    o[17] = all ? 1u : 0u;
  }
}

// ---- row layer through DevRow (one record per lane: limb k of row c) --------------
#define DC_ROW_CTX const RowCtx<DevRow> x(DevRow::lane())
DC_OP(op_rf_mul, 2, 1, 256, 1) {
  DC_ROW_CTX;
  o[0] = rf_mul(x, in[0], in[1]);
}
DC_OP(op_rf_sq, 1, 1, 256, 1) {
  DC_ROW_CTX;
  o[0] = rf_sq(x, in[0]);
}
DC_OP(op_rf_sqn3, 1, 1, 256, 1) {
  DC_ROW_CTX;
  o[0] = rf_sqn(x, in[0], 3);
}
template <int S>
struct op_rf_mul_s {
  static constexpr int IN = 2, OUT = 1, BLOCK = 256, GROUP = 1;
  static DC_FN void run(const uint32_t* in, uint32_t* o, const uint8_t*) {
    DC_ROW_CTX;
    o[0] = rf_mul_s<S>(x, in[0], in[1]);
  }
};
template <int S>
struct op_rf_sq_s {
  static constexpr int IN = 1, OUT = 1, BLOCK = 256, GROUP = 1;
  static DC_FN void run(const uint32_t* in, uint32_t* o, const uint8_t*) {
    DC_ROW_CTX;
    o[0] = rf_sq_s<S>(x, in[0]);
  }
};
static DC_FN uint32_t dc_canon(uint32_t f) {
  const RowCanon<DevRow> c = rf_canon<DevRow>(f);
  return (c.zero ? 1u : 0u) | (c.odd ? 2u : 0u);
}
// carry32(f), f - g, -g, canon(f) as zero | odd << 1; then canon(h) and
// canon(h - h) of h = carry32(f) g, and h
DC_OP(op_rf_lin, 2, 7, 256, 1) {
  DC_ROW_CTX;
  o[0] = rf_carry32(x, in[0]);
  o[1] = rf_sub(x, in[0], in[1]);
  o[2] = rf_neg(x, in[1]);
  o[3] = dc_canon(in[0]);
  const uint32_t h = rf_mul(x, o[0], in[1]);
  o[4] = dc_canon(h);
  o[5] = dc_canon(rf_sub(x, h, h));
  o[6] = h;
}
template <int R>
static DC_FN void dc_row_moves(uint32_t* o, uint32_t v) {
  if constexpr (R < 16) {
    if constexpr (R == 0)
      o[R] = v;  // row_ror:0 is no DPP control; the product's term 0 takes f itself
    else
      o[R] = DevRow::ror<R>(v);
    o[16 + R] = DevRow::bcast<R>(v);
    dc_row_moves<R + 1>(o, v);
  }
}
// in: x, lo, hi. out: ror<0..15>, bcast<0..15>, rows (4), the product's
// ror_rows triples (3), sum_rows<2> and <4> of (hi << 32 | lo) (lo, hi each)
DC_OP(op_row_moves, 3, 43, 256, 1) {
  const uint32_t v = in[0];
  dc_row_moves<0>(o, v);
  DevRow::rows(v, o[32], o[33], o[34], o[35]);
  o[36] = DevRow::ror_rows<4, 8, 12>(v);
  o[37] = DevRow::ror_rows<0, 8, 8>(v);
  o[38] = DevRow::ror_rows<12, 8, 4>(v);
  const uint64_t w = ((uint64_t)in[2] << 32) | in[1];
  const uint64_t s2 = DevRow::sum_rows<2>(w), s4 = DevRow::sum_rows<4>(w);
  o[39] = (uint32_t)s2;
  o[40] = (uint32_t)(s2 >> 32);
  o[41] = (uint32_t)s4;
  o[42] = (uint32_t)(s4 >> 32);
}
// in: v (extended, carried), c (cached). out: dbl(v), v + c, to_cached(v),
// cached_neg(c)
DC_OP(op_rp, 2, 4, 256, 1) {
  DC_ROW_CTX;
  uint32_t v = in[0];
  rp_dbl(x, v);
  o[0] = v;
  v = in[0];
  rp_add(x, v, in[1]);
  o[1] = v;
  o[2] = rp_to_cached(x, in[0], x.cst(RowConst::d2));
  o[3] = rp_cached_neg(x, in[1]);
}
// in: y limb (rows c and c ^ 2 the same value), sign. out: x, x y, decoded
DC_OP(op_rf_decode, 2, 3, 256, 1) {
  DC_ROW_CTX;
  uint32_t xo, to;
  const bool ok = rf_decode<0, 2>(x, in[0], in[1] != 0, xo, to);
  o[0] = xo;
  o[1] = to;
  o[2] = ok ? 1u : 0u;
}

// ---- quad and oct policies (one record per lane: coordinate c of a quad) ----------
template <int I, int... PATS>
struct dc_perms;
template <int I>
struct dc_perms<I> {
  static DC_FN void run(const DevQuad&, uint32_t*, uint32_t*, uint32_t*, const fe&, const fe&) {}
};
template <int I, int PAT, int... REST>
struct dc_perms<I, PAT, REST...> {
  // perm<PAT>(v) -> op[10 I ..], perm32<PAT>(v[0]) -> o32[I], permc<PAT>(v) + b -> oc[10 I ..]
  static DC_FN void run(const DevQuad& q, uint32_t* op, uint32_t* o32, uint32_t* oc, const fe& v, const fe& b) {
    fe t;
    q.perm<PAT>(t, v);
    st_fe(op + 10 * I, t);
    o32[I] = q.perm32<PAT>(v.v[0]);
    q.permc<PAT>(t, v);
    for (int i = 0; i < 10; i++) oc[10 * I + i] = t.v[i] + b.v[i];
    dc_perms<I + 1, REST...>::run(q, op, o32, oc, v, b);
  }
};
// every pattern quad.h passes to perm / permc / perm32, in the order of
// QUAD_PATTERNS in the test
constexpr int kDcNPat = 11;
DC_OP(op_q_perm, 20, 21 * kDcNPat, 256, 1) {
  const DevQuad q;
  fe v, b;
  ld_fe(v, in);
  ld_fe(b, in + 10);
  dc_perms<0, QP_B0, QP_B1, QP_B2, QP_B3, QP_SWAP01, qp(0, 1, 2, 0), qp(2, 0, 0, 0), qp(3, 2, 0, 1), qp(1, 2, 2, 1),
           qp(0, 3, 3, 0), qp(2, 3, 1, 0)>::run(q, o, o + 10 * kDcNPat, o + 11 * kDcNPat, v, b);
}
template <int I, int... PATS>
struct dc_fused;
template <int I>
struct dc_fused<I> {
  static DC_FN void run(const DevQuad&, uint32_t*, const fe&, const fe&, uint32_t) {}
};
template <int I, int PAT, int... REST>
struct dc_fused<I, PAT, REST...> {
  static DC_FN void run(const DevQuad& q, uint32_t* o, const fe& src, const fe& b, uint32_t k) {
    fe t;
    q.add_perm<PAT>(t, src, b);
    st_fe(o + 30 * I, t);
    q.xor_perm<PAT>(t, src, k);
    st_fe(o + 30 * I + 10, t);
    q.perm_lane3<PAT>(t, src);
    st_fe(o + 30 * I + 20, t);
    dc_fused<I + 1, REST...>::run(q, o, src, b, k);
  }
};
// every pattern of CMTV_QP_CASES: add_perm, xor_perm, perm_lane3
DC_OP(op_q_fused, 21, 150, 256, 1) {
  const DevQuad q;
  fe src, b;
  ld_fe(src, in);
  ld_fe(b, in + 10);
  dc_fused<0, 0x55, qp(0, 1, 2, 0), qp(2, 0, 0, 0), qp(0, 3, 3, 0), qp(1, 2, 2, 1)>::run(q, o, src, b, in[20]);
}
DC_OP(op_oct_upper, 10, 11, 256, 1) {
  const DevOct q;
  fe v, t;
  ld_fe(v, in);
  q.from_upper(t, v);
  st_fe(o, t);
  o[10] = q.from_upper32(v.v[0]);
}
// in: v (extended), c (cached), neg. out: dbl(v), v + c, to_cached(v),
// cneg(c, neg), small_order(v)
template <int FOLD>
struct op_q_point {
  static constexpr int IN = 21, OUT = 41, BLOCK = 256, GROUP = 1;
  static DC_FN void run(const uint32_t* in, uint32_t* o, const uint8_t*) {
    const DevQuad q;
    fe v0, c, v;
    ld_fe(v0, in);
    ld_fe(c, in + 10);
    v = v0;
    q_dbl<FOLD>(q, v);
    st_fe(o, v);
    v = v0;
    q_add<FOLD>(q, v, c);
    st_fe(o + 10, v);
    q_to_cached(q, v, v0);
    st_fe(o + 20, v);
    v = c;
    q_cached_cneg(q, v, in[20] != 0);
    st_fe(o + 30, v);
    o[40] = q_small_order(q, v0) ? 1u : 0u;
  }
};
#endif  // !DEVCHECK_HOST

// ---- driver -----------------------------------------------------------------------
#ifndef DEVCHECK_HOST
#define DC_HIP(call)                                                                   \
  do {                                                                                 \
    const hipError_t e_ = (call);                                                      \
    if (e_ != hipSuccess) {                                                            \
      fprintf(stderr, "devcheck: %s: %s\n", #call, hipGetErrorString(e_));             \
      exit(3);                                                                         \
    }                                                                                  \
  } while (0)

template <class Op>
__global__ void __launch_bounds__(Op::BLOCK) k_op(const uint32_t* in, uint32_t* out, const uint8_t* blob) {
  const size_t t = (size_t)blockIdx.x * Op::BLOCK + threadIdx.x;
  const size_t rec = t / Op::GROUP;
  Op::run(in + rec * Op::IN, out + rec * Op::OUT, blob);
}
#endif

// records padded to whole blocks; in holds nrec * IN words (zero past n)
template <class Op>
static void run_op(std::vector<uint32_t>& out, const std::vector<uint32_t>& in, size_t nrec,
                   const std::vector<uint32_t>& blob) {
#ifdef DEVCHECK_HOST
  for (size_t r = 0; r < nrec; r++) Op::run(&in[r * Op::IN], &out[r * Op::OUT], (const uint8_t*)blob.data());
#else
  uint32_t *din, *dout, *dblob;
  DC_HIP(hipMalloc(&din, in.size() * 4));
  DC_HIP(hipMalloc(&dout, out.size() * 4));
  DC_HIP(hipMalloc(&dblob, blob.size() * 4));
  DC_HIP(hipMemcpy(din, in.data(), in.size() * 4, hipMemcpyHostToDevice));
  DC_HIP(hipMemcpy(dblob, blob.data(), blob.size() * 4, hipMemcpyHostToDevice));
  DC_HIP(hipMemset(dout, 0, out.size() * 4));
  const size_t threads = nrec * Op::GROUP;
  hipLaunchKernelGGL(k_op<Op>, dim3((unsigned)(threads / Op::BLOCK)), dim3(Op::BLOCK), 0, 0, din, dout,
                     (const uint8_t*)dblob);
  DC_HIP(hipGetLastError());
  DC_HIP(hipDeviceSynchronize());
  DC_HIP(hipMemcpy(out.data(), dout, out.size() * 4, hipMemcpyDeviceToHost));
  DC_HIP(hipFree(din));
  DC_HIP(hipFree(dout));
  DC_HIP(hipFree(dblob));
#endif
}

template <class Op>
static int drive(bool sha) {
  uint32_t hdr[2];
  if (fread(hdr, 4, 2, stdin) != 2) return 1;
  const size_t n = hdr[0], nblob = hdr[1];
  if (n == 0 || n > (1u << 22) || nblob > (1u << 26)) return 1;
  // whole blocks of threads: GROUP threads per record
  const size_t per_block = Op::BLOCK / Op::GROUP ? Op::BLOCK / Op::GROUP : 1;
  const size_t nrec = (n + per_block - 1) / per_block * per_block;
  std::vector<uint32_t> in(nrec * Op::IN, 0u), out(nrec * Op::OUT, 0u);
  // the hashes read whole aligned words: the blob ends on one, with a word to spare
  std::vector<uint32_t> blob(nblob / 4 + 2, 0u);
  if (fread(in.data(), 4 * Op::IN, n, stdin) != n) return 1;
  if (nblob && fread(blob.data(), 1, nblob, stdin) != nblob) return 1;
  if (sha)  // every message inside the blob (padding records: offset 0, length 0)
    for (size_t r = 0; r < n; r++)
      if ((uint64_t)in[r * Op::IN] + in[r * Op::IN + 1] > nblob) return 1;
  run_op<Op>(out, in, nrec, blob);
  if (fwrite(out.data(), 4 * Op::OUT, n, stdout) != n) return 1;
  return fflush(stdout) ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const char* op = argv[1];
#define DC_CASE(NAME, ...) \
  if (!strcmp(op, NAME)) return drive<__VA_ARGS__>(false)
  DC_CASE("fe_mul", op_fe_mul);
  DC_CASE("fe_sq", op_fe_sq);
  DC_CASE("fe_sqn1", op_fe_sqn<1>);
  DC_CASE("fe_sqn2", op_fe_sqn<2>);
  DC_CASE("fe_sqn5", op_fe_sqn<5>);
  DC_CASE("fe_sqn50", op_fe_sqn<50>);
  DC_CASE("fe_carry", op_fe_carry);
  DC_CASE("fe_lin", op_fe_lin);
  DC_CASE("fe_frombytes", op_fe_frombytes);
  DC_CASE("fe_canon", op_fe_canon);
  DC_CASE("fe_equal", op_fe_equal);
  DC_CASE("fe_pow", op_fe_pow);
  DC_CASE("sc_reduce512", op_sc_reduce512);
  DC_CASE("sc_is_canonical", op_sc_is_canonical);
  DC_CASE("sc_muladd", op_sc_muladd);
  DC_CASE("half", op_half);
  DC_CASE("hs_prims", op_hs_prims);
  DC_CASE("keccak", op_keccak);
  DC_CASE("ristretto_decode", op_ristretto_decode);
  DC_CASE("sqrt_ratio_m1", op_sqrt_ratio_m1);
  DC_CASE("secp_parse_pubkey", op_secp_parse_pubkey);
  DC_CASE("secp_sig_scalars", op_secp_sig_scalars);
  DC_CASE("secp_x_is_r", op_secp_x_is_r);
  DC_CASE("pt_add", op_pt_add);
  DC_CASE("pt_double", op_pt_double);
  if (!strcmp(op, "sha512_16")) return drive<op_sha512<16>>(true);
  if (!strcmp(op, "sha512_8")) return drive<op_sha512<8>>(true);
#ifndef DEVCHECK_HOST
  DC_CASE("half_uni", op_half_uni);
  DC_CASE("rf_mul", op_rf_mul);
  DC_CASE("rf_sq", op_rf_sq);
  DC_CASE("rf_sqn3", op_rf_sqn3);
  DC_CASE("rf_mul_s2", op_rf_mul_s<2>);
  DC_CASE("rf_mul_s4", op_rf_mul_s<4>);
  DC_CASE("rf_sq_s2", op_rf_sq_s<2>);
  DC_CASE("rf_sq_s4", op_rf_sq_s<4>);
  DC_CASE("rf_lin", op_rf_lin);
  DC_CASE("row_moves", op_row_moves);
  DC_CASE("rp", op_rp);
  DC_CASE("rf_decode", op_rf_decode);
  DC_CASE("q_perm", op_q_perm);
  DC_CASE("q_fused", op_q_fused);
  DC_CASE("oct_upper", op_oct_upper);
  DC_CASE("q_point0", op_q_point<0>);
  DC_CASE("q_point2", op_q_point<2>);
#endif
  fprintf(stderr, "devcheck: unknown op %s\n", op);
  return 2;
}
