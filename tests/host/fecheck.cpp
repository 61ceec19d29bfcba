// Stand-alone check of fe_mul / fe_sq / fe_sqn (cometbft_amd/csrc/fe25519.h)
// in both carry chains against 256-bit integer arithmetic mod 2^255 - 19.
// Built twice by tests/test_fe_reduce.py: with -DCMTV_BOUNDS_CHECK (the
// header's operand, column and output assertions on) and with
// -fsanitize=address,undefined. Test infrastructure only.
//   fecheck [random cases]   exit 0 and "ok ..." on success, 1 and the case otherwise
#define CMTV_HD inline
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../cometbft_amd/csrc/fe25519.h"

using namespace cmtv;
typedef unsigned __int128 u128;

// ---- integers below 2^256, reduced mod p only by canon() -------------------------------
struct U256 {
  uint64_t w[4];
};

static const int SH[10] = {0, 26, 51, 77, 102, 128, 153, 179, 204, 230};  // ceil(25.5 i)

// x (8 words) mod-p folded into 4 words: 2^256 = 38 (mod p)
static U256 fold512(const uint64_t x[8]) {
  uint64_t r[5];
  u128 c = 0;
  for (int i = 0; i < 4; i++) {
    c += (u128)x[i] + (u128)x[4 + i] * 38;
    r[i] = (uint64_t)c;
    c >>= 64;
  }
  r[4] = (uint64_t)c;  // < 39
  for (int round = 0; round < 2; round++) {
    c = (u128)r[4] * 38;
    r[4] = 0;
    for (int i = 0; i < 4; i++) {
      c += r[i];
      r[i] = (uint64_t)c;
      c >>= 64;
    }
    r[4] = (uint64_t)c;
  }
  return U256{{r[0], r[1], r[2], r[3]}};
}

static U256 mulmod(const U256& a, const U256& b) {
  uint64_t x[8] = {0};
  for (int i = 0; i < 4; i++) {
    u128 c = 0;
    for (int j = 0; j < 4; j++) {
      c += (u128)a.w[i] * b.w[j] + x[i + j];
      x[i + j] = (uint64_t)c;
      c >>= 64;
    }
    x[i + 4] = (uint64_t)c;
  }
  return fold512(x);
}

// the value of ten 32-bit limbs (up to 2^262), folded below 2^256
static U256 from_limbs(const fe& f) {
  uint64_t x[8] = {0};
  for (int i = 0; i < 10; i++) {
    const int wi = SH[i] >> 6, sh = SH[i] & 63;
    u128 c = (u128)f.v[i] << sh;
    for (int k = wi; c != 0; k++) {
      c += x[k];
      x[k] = (uint64_t)c;
      c >>= 64;
    }
  }
  return fold512(x);
}

// the representative in [0, p)
static U256 canon(U256 a) {
  for (int round = 0; round < 2; round++) {
    u128 c = (u128)(a.w[3] >> 63) * 19;
    a.w[3] &= ~(1ull << 63);
    for (int i = 0; i < 4; i++) {
      c += a.w[i];
      a.w[i] = (uint64_t)c;
      c >>= 64;
    }
  }
  const bool ge_p = a.w[3] == 0x7FFFFFFFFFFFFFFFull && a.w[2] == ~0ull && a.w[1] == ~0ull && a.w[0] >= ~0ull - 18;
  if (ge_p) {
    a.w[0] -= ~0ull - 18;
    a.w[1] = a.w[2] = a.w[3] = 0;
  }
  return a;
}

static bool same(const U256& a, const U256& b) {
  const U256 x = canon(a), y = canon(b);
  return x.w[0] == y.w[0] && x.w[1] == y.w[1] && x.w[2] == y.w[2] && x.w[3] == y.w[3];
}

// ---- bounds ("carried", fe25519.h) ------------------------------------------------------
// serial chain: only limb 1 exceeds its mask, by (2^26 - 1 + 19 c_9) >> 26 with
// c_9 < 2^64 / 2^25: below 2^13 (the header's statement; the largest columns
// give 4075). ref10 chain: limbs 1 and 5, as tests/dev/devcases.py derives.
static bool carried(const fe& h, bool serial) {
  for (int i = 0; i < 10; i++) {
    uint32_t lim = (i & 1) ? M25 : M26;
    if (i == 1 || (i == 5 && !serial)) lim += 1u << 13;
    if (h.v[i] > lim) return false;
  }
  return true;
}

static int failures = 0;

static void fail(const char* what, const fe& f, const fe& g) {
  failures++;
  std::fprintf(stderr, "FAIL %s\n  f =", what);
  for (int i = 0; i < 10; i++) std::fprintf(stderr, " %u", f.v[i]);
  std::fprintf(stderr, "\n  g =");
  for (int i = 0; i < 10; i++) std::fprintf(stderr, " %u", g.v[i]);
  std::fprintf(stderr, "\n");
}

// g may have any limb up to MUL_BOUND - 1; sq_ok: f is inside fe_sq's bound too
static void check_pair(const fe& f, const fe& g, bool sq_ok) {
  const U256 F = from_limbs(f), G = from_limbs(g);
  fe s, r;
  fe_mul<FE_CHAIN_SERIAL>(s, f, g);
  fe_mul<FE_CHAIN_REF10>(r, f, g);
  const U256 want = mulmod(F, G);
  if (!same(from_limbs(s), want) || !carried(s, true)) fail("fe_mul serial", f, g);
  if (!same(from_limbs(r), want) || !carried(r, false)) fail("fe_mul ref10", f, g);
  if (!same(from_limbs(s), from_limbs(r))) fail("fe_mul serial != ref10", f, g);
  // a product is a valid operand of the next one
  fe_mul(r, s, g);
  if (!same(from_limbs(r), mulmod(want, G)) || !carried(r, true)) fail("fe_mul of a product", f, g);
  if (!sq_ok) return;
  fe_sq<FE_CHAIN_SERIAL>(s, f);
  fe_sq<FE_CHAIN_REF10>(r, f);
  U256 w = mulmod(F, F);
  if (!same(from_limbs(s), w) || !carried(s, true)) fail("fe_sq serial", f, g);
  if (!same(from_limbs(r), w) || !carried(r, false)) fail("fe_sq ref10", f, g);
  for (int n : {1, 2, 5}) {
    fe_sqn<FE_CHAIN_SERIAL>(s, f, n);
    fe_sqn<FE_CHAIN_REF10>(r, f, n);
    w = F;
    for (int k = 0; k < n; k++) w = mulmod(w, w);
    if (!same(from_limbs(s), w) || !carried(s, true)) fail("fe_sqn serial", f, g);
    if (!same(from_limbs(r), w) || !carried(r, false)) fail("fe_sqn ref10", f, g);
  }
}

static fe limbs_of_p(int times, int minus) {  // times * p - minus, limb-wise (no carry)
  fe h;
  h.v[0] = times * ((1u << 26) - 19) - minus;
  for (int i = 1; i < 10; i++) h.v[i] = times * ((i & 1) ? M25 : M26);
  return h;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t bound) {  // xorshift64*, uniform enough for limbs
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)(((rng_state * 0x2545F4914F6CDD1Dull) >> 32) * (uint64_t)bound >> 32);
}

int main(int argc, char** argv) {
  const int n_random = argc > 1 ? std::atoi(argv[1]) : 100000;
  fe top, sqtop, zero;
  for (int i = 0; i < 10; i++) {
    top.v[i] = MUL_BOUND - 1;
    sqtop.v[i] = (i & 1) ? SQ_ODD_BOUND - 1 : MUL_BOUND - 1;
    zero.v[i] = 0;
  }
  std::vector<fe> edge = {top, sqtop, zero, limbs_of_p(1, 0), limbs_of_p(2, 0), limbs_of_p(1, 1)};
  int cases = 0;
  for (const fe& f : edge)
    for (const fe& g : edge) {
      bool sq_ok = true;
      for (int i = 1; i < 10; i += 2) sq_ok = sq_ok && f.v[i] < SQ_ODD_BOUND;
      check_pair(f, g, sq_ok);
      cases++;
    }
  // lazy inputs: limbs anywhere below the bounds, a quarter of them carried
  for (int t = 0; t < n_random; t++) {
    fe f, g;
    for (int i = 0; i < 10; i++) {
      const uint32_t c = ((i & 1) ? M25 : M26) + 1;
      f.v[i] = (t & 3) == 0 ? rnd(c) : rnd((i & 1) ? SQ_ODD_BOUND : MUL_BOUND);
      g.v[i] = (t & 3) == 1 ? rnd(c) : rnd(MUL_BOUND);
    }
    check_pair(f, g, true);
    cases++;
  }
  if (failures) {
    std::fprintf(stderr, "%d failures in %d cases\n", failures, cases);
    return 1;
  }
  std::printf("ok %d cases\n", cases);
  return 0;
}
