// Host check of the split window sums of k_verify_quad_hs_fold
// (cometbft_amd/csrc/quad.h h_window_addend_eh / _fg / _xy; hs_helper.h
// hs_helper_sums_eh / _fg): two waves form each window's S_w = [dA](-A) +
// [dR](-/+R) between them, and every limb has to be h_window_addend's.
//   argv[1] == "pieces": tables of (0..8)P as extended points for random
//       points, the identity, points of order 8 and 4, and the same with
//       Z != 1; for every pair of tables, every dA, dR in -8..7 and both
//       r_flip the three pieces' four outputs against h_window_addend's limb
//       for limb. stdout: "ok <cases> cases".
//   argv[1] == "fold": q_verify_hs_fold in the four-lane-thread harness of
//       foldcheck.cpp with S_w from the pieces: lane thread 0 plays the hash
//       helper (_eh, then _xy once F and G are there), lane thread 1 the comb
//       wave (_fg), each walking its own copy of the digits, and every sum is
//       compared with h_window_addend's again (exit 3 on a difference).
//       argv[2] == "wide": the 64-window fallback for every signature.
//       stdin as foldcheck.cpp: u32 n, n x { u8 mode, pk[32], sig[64], u32
//       mlen, msg }; stdout: n x { the verdict, q_verify_hs's verdict }.
//       The window count is the signature's own raised by i % 3; the comb
//       wave's share of [s]B is its top i % 17 positions, and every fourth
//       signature's never arrives.
// Compile with -DCMTV_BOUNDS_CHECK for the operand bound assertions. Test
// infrastructure only.
#define CMTV_HD inline
#include <atomic>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>
#include "../../cometbft_amd/csrc/quad.h"
#include "lazy_btab.h"

using namespace cmtv;

static bool fe_same(const fe& a, const fe& b) { return memcmp(a.v, b.v, sizeof(a.v)) == 0; }

// ---------------------------------------------------------------- pieces

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd32() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 16);
}

static void random_point(ge_p3& p) {
  uint32_t w[8];
  do {
    for (int i = 0; i < 8; i++) w[i] = rnd32();
  } while (!p3_frombytes(p, w));
}

static void point_from_hex(ge_p3& p, const char* hex) {
  uint32_t w[8] = {};
  for (int i = 0; i < 32; i++) {
    unsigned b;
    sscanf(hex + 2 * i, "%2x", &b);
    w[i / 4] |= (uint32_t)b << (8 * (i % 4));
  }
  if (!p3_frombytes(p, w)) abort();
}

// the same point with every coordinate multiplied by a random field element
static void rescale(ge_p3& p) {
  ge_p3 l;
  random_point(l);
  fe_mul(p.X, p.X, l.Y);
  fe_mul(p.Y, p.Y, l.Y);
  fe_mul(p.Z, p.Z, l.Y);
  fe_mul(p.T, p.T, l.Y);
}

// (0..8)P, extended
static void build_table(ge_p3 tab[9], const ge_p3& p) {
  p3_identity(tab[0]);
  tab[1] = p;
  ge_cached c;
  p3_to_cached(c, p);
  for (int e = 2; e <= 8; e++) {
    ge_efgh r;
    ge_add_cached(r, tab[e - 1], c);
    efgh_to_p3(tab[e], r);
  }
}

static int run_pieces() {
  std::vector<ge_p3> pts(14);
  for (int i = 0; i < 6; i++) random_point(pts[i]);
  p3_identity(pts[6]);
  // order 8, order 4 (y = 0) and order 2 (y = -1)
  point_from_hex(pts[7], "26e8958fc2b227b045c3f489f2ef98f0d5dfac05d3c63339b13802886d53fc05");
  point_from_hex(pts[8], "0000000000000000000000000000000000000000000000000000000000000000");
  point_from_hex(pts[9], "ecffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff7f");
  for (int i = 10; i < 14; i++) {  // Z != 1: two random points, the identity, the point of order 8
    pts[i] = pts[i == 10 ? 0 : i == 11 ? 1 : i == 12 ? 6 : 7];
    rescale(pts[i]);
  }
  const int N = (int)pts.size();
  std::vector<std::vector<ge_p3>> tabs(N, std::vector<ge_p3>(9));
  for (int i = 0; i < N; i++) build_table(tabs[i].data(), pts[i]);
  long cases = 0;
  for (int a = 0; a < N; a++)
    for (int step = 0; step < 3; step++) {
      const int r = (a + (step == 0 ? 0 : step == 1 ? 1 : 7)) % N;
      auto rd = [&](int P, int e, int c, fe& out) {
        const ge_p3& q = (P == 0 ? tabs[a] : tabs[r])[e];
        out = c == 0 ? q.X : c == 1 ? q.Y : c == 2 ? q.Z : q.T;
      };
      for (int dA = -8; dA <= 7; dA++)
        for (int dR = -8; dR <= 7; dR++)
          for (int flip = 0; flip < 2; flip++) {
            fe want[4], got[4], e, f, g, h;
            h_window_addend(want, rd, dA, dR, flip != 0);
            h_window_addend_eh(got[3], e, h, rd, dA, dR, flip != 0);
            h_window_addend_fg(got[2], f, g, rd, dA, dR, flip != 0);
            h_window_addend_xy(got[0], got[1], e, f, g, h);
            for (int c = 0; c < 4; c++)
              if (!fe_same(want[c], got[c])) {
                fprintf(stderr, "tables %d / %d, dA %d dR %d flip %d: out[%d] differs\n", a, r, dA, dR, flip, c);
                return 3;
              }
            cases++;
          }
    }
  printf("ok %ld cases\n", cases);
  return 0;
}

// ------------------------------------------------------------------ fold

struct SpinBarrier {
  std::atomic<int> count{0};
  std::atomic<int> gen{0};
  void arrive_and_wait() {
    const int g = gen.load(std::memory_order_acquire);
    if (count.fetch_add(1, std::memory_order_acq_rel) == 3) {
      count.store(0, std::memory_order_relaxed);
      gen.store(g + 1, std::memory_order_release);
      return;
    }
    for (int spins = 0; gen.load(std::memory_order_acquire) == g; spins++)
      if (spins > 256) std::this_thread::yield();
  }
};

struct Exchange {
  SpinBarrier bar;
  fe slot[4];
};

// the quad policy of quadcheck.cpp
struct HostQuad {
  int ln;
  Exchange* ex;
  int lane() const { return ln; }
  template <int PAT>
  void perm(fe& o, const fe& v) const {
    ex->slot[ln] = v;
    ex->bar.arrive_and_wait();
    const fe r = ex->slot[(PAT >> (2 * ln)) & 3];
    ex->bar.arrive_and_wait();
    o = r;
  }
  template <int PAT>
  void add_perm(fe& o, const fe& src, const fe& b) const {
    fe t;
    perm<PAT>(t, src);
    for (int i = 0; i < 10; i++) o.v[i] = t.v[i] + b.v[i];
  }
  template <int PAT>
  void xor_perm(fe& o, const fe& src, uint32_t k) const {
    perm<PAT>(o, src);
    for (int i = 0; i < 10; i++) o.v[i] ^= k;
  }
  template <int PAT>
  void perm_lane3(fe& o, const fe& src) const {
    perm<PAT>(o, src);
    for (int i = 0; i < 10; i++) o.v[i] = lane() == 3 ? o.v[i] : 0u;
  }
  template <int PAT>
  void permc(fe& o, const fe& v) const {
    perm<PAT>(o, v);
  }
  template <int PAT>
  uint32_t perm32(uint32_t x) const {
    fe t, o;
    fe_0(t);
    t.v[0] = x;
    perm<PAT>(o, t);
    return o.v[0];
  }
  bool any(bool x) const { return x; }
};

static void to_words(uint32_t* w, const uint8_t* b, int nw) {
  for (int i = 0; i < nw; i++) w[i] = b[4 * i] | (b[4 * i + 1] << 8) | (b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
}

static int run_fold(bool force_wide) {
  LazyBTab bt;
  uint32_t n;
  if (fread(&n, 4, 1, stdin) != 1) return 1;
  for (uint32_t i = 0; i < n; i++) {
    uint8_t mode = 0, pk[32], sig[64];
    uint32_t mlen;
    if (fread(&mode, 1, 1, stdin) != 1 || fread(pk, 32, 1, stdin) != 1 || fread(sig, 64, 1, stdin) != 1 ||
        fread(&mlen, 4, 1, stdin) != 1)
      return 1;
    std::vector<uint8_t> buf(mlen + 16, 0xEE);
    uint8_t* mp = buf.data() + 4 + (i % 4);
    if (mlen && fread(mp, mlen, 1, stdin) != 1) return 1;
    uint32_t pkw[8], sigw[16];
    to_words(pkw, pk, 8);
    to_words(sigw, sig, 16);
    const bool late = i % 4 == 3;
    uint8_t out[2];
    for (int fold = 1; fold >= 0; fold--) {
      // the hash helper
      SigPrep hp;
      if (mode)
        q_prepare<MODE_ZIP215>(hp, pkw, sigw, mp, mlen, force_wide);
      else
        q_prepare<MODE_GO_STDLIB>(hp, pkw, sigw, mp, mlen, force_wide);
      const bool wide = (hp.flags & 2u) != 0;
      const int own = (int)((hp.flags >> 8) & 0xFFu);
      const int W = wide ? HS_WIDE_WINDOWS : (own + (int)(i % 3) > HS_MAX_WINDOWS ? HS_MAX_WINDOWS : own + (int)(i % 3));
      hp.flags |= (uint32_t)W << 16;
      const bool r_flip = (hp.flags & 1u) != 0;
      uint32_t prep[SIG_PREP_WORDS];
      if (fold)
        sig_prep_store_pair(prep, hp);
      else
        sig_prep_store(prep, hp);
      // the two helper waves' walks, [0] the hash helper's, [1] the comb
      // wave's (from prep, as it reads them after barrier 1)
      uint32_t tA[2][8], tR[2][8];
      for (int w = 0; w < 2; w++) {
        SigPrep wp = hp;
        if (w == 1 && fold) sig_prep_load_pair(wp, prep);
        hs_digits16(tA[w], wp.k1, W);
        hs_digits16(tR[w], wp.k2, W);
        sc_shift_out(tA[w], 4);
        sc_shift_out(tR[w], 4);
      }
      const int pre = (int)(i % 17);
      BComb16Ahead bc;
      bc.init(sigw + 8, bt);
      for (int k = 0; k < pre; k++) bc.step(bt);
      const fe* xyz[3] = {&bc.P.X, &bc.P.Y, &bc.P.Z};
      uint32_t bpt[40];
      {
        ge_p3 Bp;
        q_bcomb16(Bp, hp.u, bt);
        bpoint_store(bpt, Bp);
      }
      Exchange ex;
      bool res[4];
      QArrayTab ta[4], tr[4];
      fe S[4], E, F, G, H;
      std::atomic<bool> differs{false};
      std::vector<std::thread> th;
      for (int l = 0; l < 4; l++)
        th.emplace_back([&, l] {
          HostQuad q{l, &ex};
          auto rd = [&](int P, int e, int cc, fe& r) { r = (P == 0 ? ta[cc] : tr[cc]).t[e]; };
          int dA = 0, dR = 0;
          auto get_s = [&](int, fe& c) {
            ex.bar.arrive_and_wait();  // every lane's tables are built
            if (l < 2) {
              dA = (int)sc_shift_out(tA[l], 4) - 8;
              dR = (int)sc_shift_out(tR[l], 4) - 8;
            }
            if (l == 0) h_window_addend_eh(S[3], E, H, rd, dA, dR, r_flip);
            if (l == 1) h_window_addend_fg(S[2], F, G, rd, dA, dR, r_flip);
            ex.bar.arrive_and_wait();  // F and G are published
            if (l == 0) {
              h_window_addend_xy(S[0], S[1], E, F, G, H);
              fe want[4];
              h_window_addend(want, rd, dA, dR, r_flip);
              for (int k = 0; k < 4; k++)
                if (!fe_same(want[k], S[k])) differs = true;
            }
            ex.bar.arrive_and_wait();
            c = S[l];
          };
          if (fold) {
            auto get_ps = [&](fe& ps) {
              if (late) return false;
              fe_mul(ps, *xyz[q_p2_factor_a(l)], *xyz[q_p2_factor_b(l)]);
              return true;
            };
            auto get_prep = [&](SigPrep& p) { sig_prep_load_pair(p, prep); };
            res[l] = mode ? q_verify_hs_fold<MODE_ZIP215>(q, pkw, sigw, bt, 16 - pre, ta[l], tr[l], get_ps, get_prep,
                                                          get_s)
                          : q_verify_hs_fold<MODE_GO_STDLIB>(q, pkw, sigw, bt, 16 - pre, ta[l], tr[l], get_ps,
                                                             get_prep, get_s);
          } else {
            auto get_prep = [&](SigPrep& p) { sig_prep_load(p, prep); };
            auto get_b = [&](fe& c) {
              for (int j = 0; j < 10; j++) c.v[j] = bpt[10 * l + j];
            };
            res[l] = mode ? q_verify_hs<MODE_ZIP215>(q, pkw, sigw, bt, ta[l], tr[l], 0, get_prep, get_s, get_b)
                          : q_verify_hs<MODE_GO_STDLIB>(q, pkw, sigw, bt, ta[l], tr[l], 0, get_prep, get_s, get_b);
          }
        });
      for (auto& t : th) t.join();
      if (res[0] != res[1] || res[0] != res[2] || res[0] != res[3]) {
        fprintf(stderr, "lanes disagree on vector %u (fold %d)\n", i, fold);
        return 2;
      }
      if (differs) {
        fprintf(stderr, "a split sum differs from h_window_addend on vector %u (fold %d)\n", i, fold);
        return 3;
      }
      out[fold ? 0 : 1] = res[0];
    }
    fwrite(out, 1, 2, stdout);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "pieces")) return run_pieces();
  if (argc > 1 && !strcmp(argv[1], "fold")) return run_fold(argc > 2 && !strcmp(argv[2], "wide"));
  return 1;
}
