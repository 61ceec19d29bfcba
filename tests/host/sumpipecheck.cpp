// Host check of the pipelined window sums of k_verify_quad_hs_fold
// (cometbft_amd/csrc/quad.h h_window_addend_front / _back and h_sums_pipe;
// hs_helper.h hs_helper_sums_pipe): two waves form every second window's
// S_w = [dA](-A) + [dR](-/+R) each, half a sum per window, and meet only at
// the window barriers. The loop under test is the device's own (h_sums_pipe),
// run by two host threads.
//   argv[1] == "halves": tables of (0..8)P as extended points for random
//       points, the identity, points of order 8, 4 and 2, and the same with
//       Z != 1; for every pair of tables, every dA, dR in -8..8 and both
//       r_flip, _front + _back against h_window_addend's four outputs limb
//       for limb. stdout: "ok <cases> cases".
//   argv[1] == "schedule": for every W in 2..HS_MAX_WINDOWS and for
//       HS_WIDE_WINDOWS, the two waves and a reader at the window barriers
//       over a 2-slot ring, digits drawn per window: every read of slot
//       (win & 1) after barrier win finds S_win (its tag, and its limbs
//       against h_window_addend on that window's digits); no slot is stored
//       to before its previous content was read; each wave meets W - 1
//       barriers; the lead stores S_{W-2}, owners alternate, so S_0 is the
//       lead's exactly when W is even. stdout: "ok <W values> schedules".
//   argv[1] == "fold": q_verify_hs_fold in the four-lane-thread harness of
//       foldcheck.cpp with S_w from two more threads running h_sums_pipe
//       (the hash helper, and the comb wave with its scalars from prep), then
//       again with the undivided h_window_addend; every pipelined sum is
//       compared with h_window_addend's (exit 3 on a difference).
//       argv[2] == "wide": the 64-window fallback for every signature.
//       stdin as foldcheck.cpp: u32 n, n x { u8 mode, pk[32], sig[64], u32
//       mlen, msg }; stdout: n x { the pipelined verdict, the undivided one }.
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

static std::vector<std::vector<ge_p3>> make_tables() {
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
  std::vector<std::vector<ge_p3>> tabs(pts.size(), std::vector<ge_p3>(9));
  for (size_t i = 0; i < pts.size(); i++) build_table(tabs[i].data(), pts[i]);
  return tabs;
}

// h_window_addend's table read over two tables of extended points
struct PointTabs {
  const ge_p3 *a, *r;
  void operator()(int P, int e, int c, fe& out) const {
    const ge_p3& q = (P == 0 ? a : r)[e];
    out = c == 0 ? q.X : c == 1 ? q.Y : c == 2 ? q.Z : q.T;
  }
};

// ---------------------------------------------------------------- halves

static int run_halves() {
  const auto tabs = make_tables();
  const int N = (int)tabs.size();
  long cases = 0;
  for (int a = 0; a < N; a++)
    for (int step = 0; step < 3; step++) {
      const int r = (a + (step == 0 ? 0 : step == 1 ? 1 : 7)) % N;
      const PointTabs rd{tabs[a].data(), tabs[r].data()};
      for (int dA = -8; dA <= 8; dA++)
        for (int dR = -8; dR <= 8; dR++)
          for (int flip = 0; flip < 2; flip++) {
            fe want[4], got[4], e, f, g, h;
            h_window_addend(want, rd, dA, dR, flip != 0);
            h_window_addend_front(e, f, g, h, rd, dA, dR, flip != 0);
            h_window_addend_back(got, e, f, g, h);
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

// -------------------------------------------------------------- the waves

struct SpinBarrier {
  const int parties;
  std::atomic<int> count{0};
  std::atomic<int> gen{0};
  explicit SpinBarrier(int n) : parties(n) {}
  void arrive_and_wait() {
    const int g = gen.load(std::memory_order_acquire);
    if (count.fetch_add(1, std::memory_order_acq_rel) == parties - 1) {
      count.store(0, std::memory_order_relaxed);
      gen.store(g + 1, std::memory_order_release);
      return;
    }
    for (int spins = 0; gen.load(std::memory_order_acquire) == g; spins++)
      if (spins > 256) std::this_thread::yield();
  }
};

// The 2-slot ring with what the schedule has to keep: a slot's window tag,
// who stored it, and whether its content has been read since. The window
// barriers order every access, so plain fields would do; atomics keep the
// checker itself free of races if the schedule under test is wrong.
struct Ring {
  struct Slot {
    fe out[4];
    std::atomic<int> win{-1}, unread{0};
  } slot[2];
  std::atomic<int> owner[HS_WIDE_WINDOWS];  // by window: 0 the lead, 1 the other wave
  std::atomic<int> errors{0};
  Ring() {
    for (auto& o : owner) o = -1;
  }
  void store(int win, const fe* out, bool lead) {
    Slot& s = slot[win & 1];
    if (s.unread.load() != 0) errors++;  // stored to before its content was read
    for (int c = 0; c < 4; c++) s.out[c] = out[c];
    s.win = win;
    s.unread = 1;
    if (owner[win].exchange(lead ? 0 : 1) != -1) errors++;  // one store per window
  }
  // after barrier win; last: the last of the slot's readers
  bool load(int win, fe out[4], bool last) {
    Slot& s = slot[win & 1];
    const bool ok = s.win.load() == win && s.unread.load() == 1;
    for (int c = 0; c < 4; c++) out[c] = s.out[c];
    if (last) s.unread = 0;
    return ok;
  }
};

// One of the two waves: h_sums_pipe over walk, storing to ring and meeting
// bar once per window. Returns the barriers it met.
template <class Walk>
static int run_wave(Walk& walk, int W, bool lead, Ring& ring, SpinBarrier& bar) {
  int met = 0;
  h_sums_pipe(
      walk, W, lead, [&](int win, const fe* out) { ring.store(win, out, lead); },
      [&](int) {
        bar.arrive_and_wait();
        met++;
      });
  return met;
}

// -------------------------------------------------------------- schedule

// digits by window, handed out from window W - 2 down
struct ListWalk {
  PointTabs tabs;
  const int *dA, *dR;
  int at;
  bool r_flip;
  void next(int& a, int& r) {
    a = at >= 0 ? dA[at] : 0;  // each wave steps over one pair past window 0
    r = at >= 0 ? dR[at] : 0;
    at--;
  }
  void operator()(int P, int e, int c, fe& out) const { tabs(P, e, c, out); }
};

static int run_schedule() {
  const auto tabs = make_tables();
  std::vector<int> Ws;
  for (int W = 2; W <= HS_MAX_WINDOWS; W++) Ws.push_back(W);
  Ws.push_back(HS_WIDE_WINDOWS);
  for (int W : Ws) {
    const PointTabs pt{tabs[W % 6].data(), tabs[(W + 1) % 14].data()};
    const bool flip = (W & 2) != 0;
    std::vector<int> dA(W), dR(W);
    for (int w = 0; w < W; w++) {
      dA[w] = (int)(rnd32() % 16) - 8;
      dR[w] = (int)(rnd32() % 16) - 8;
    }
    Ring ring;
    SpinBarrier bar(3);
    int met[2] = {0, 0};
    std::thread waves[2];
    for (int k = 0; k < 2; k++)
      waves[k] = std::thread([&, k] {
        ListWalk walk{pt, dA.data(), dR.data(), W - 2, flip};
        met[k] = run_wave(walk, W, k == 0, ring, bar);
      });
    int bad_reads = 0;
    for (int win = W - 2; win >= 0; win--) {  // the quads
      bar.arrive_and_wait();
      fe got[4], want[4];
      if (!ring.load(win, got, true)) bad_reads++;
      h_window_addend(want, pt, dA[win], dR[win], flip);
      for (int c = 0; c < 4; c++)
        if (!fe_same(want[c], got[c])) bad_reads++;
    }
    for (auto& t : waves) t.join();
    if (bad_reads || ring.errors) {
      fprintf(stderr, "W %d: %d reads of another window's sum, %d stores out of turn\n", W, bad_reads,
              ring.errors.load());
      return 3;
    }
    if (met[0] != W - 1 || met[1] != W - 1) {
      fprintf(stderr, "W %d: the waves met %d and %d barriers\n", W, met[0], met[1]);
      return 4;
    }
    for (int win = W - 2; win >= 0; win--)
      if (ring.owner[win] != ((W - 2 - win) & 1)) {
        fprintf(stderr, "W %d: window %d stored by wave %d\n", W, win, ring.owner[win].load());
        return 5;
      }
    if (ring.owner[W - 2] != 0 || ring.owner[0] != (W % 2 == 0 ? 0 : 1)) {
      fprintf(stderr, "W %d: the first or the last window's owner\n", W);
      return 5;
    }
  }
  printf("ok %zu schedules\n", Ws.size());
  return 0;
}

// ------------------------------------------------------------------ fold

struct Exchange {
  SpinBarrier bar{4};
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

// hs_helper.h HsWalk over the four lane threads' tables: the digits of k1 and
// k2 from window W - 2 down
struct PrepWalk {
  const QArrayTab *ta, *tr;
  uint32_t tA[8], tR[8];
  bool r_flip;
  PrepWalk(const SigPrep& p, int W, const QArrayTab* a, const QArrayTab* r) : ta(a), tr(r) {
    r_flip = (p.flags & 1u) != 0;
    hs_digits16(tA, p.k1, W);
    hs_digits16(tR, p.k2, W);
    sc_shift_out(tA, 4);
    sc_shift_out(tR, 4);
  }
  void next(int& dA, int& dR) {
    dA = (int)sc_shift_out(tA, 4) - 8;
    dR = (int)sc_shift_out(tR, 4) - 8;
  }
  void operator()(int P, int e, int c, fe& r) const { r = (P == 0 ? ta[c] : tr[c]).t[e]; }
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
    for (int pipe = 1; pipe >= 0; pipe--) {
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
      uint32_t prep[SIG_PREP_WORDS];
      sig_prep_store_pair(prep, hp);
      const int pre = (int)(i % 17);
      BComb16Ahead bc;
      bc.init(sigw + 8, bt);
      for (int k = 0; k < pre; k++) bc.step(bt);
      const fe* xyz[3] = {&bc.P.X, &bc.P.Y, &bc.P.Z};
      Exchange ex;
      SpinBarrier wbar(pipe ? 6 : 4);  // barrier 1 and the window barriers: the quad's lanes and the two waves
      Ring ring;
      bool res[4];
      QArrayTab ta[4], tr[4];
      std::atomic<int> differs{0};
      int met[2] = {W - 1, W - 1};
      std::vector<std::thread> th;
      if (pipe)
        for (int k = 0; k < 2; k++)
          th.emplace_back([&, k] {
            wbar.arrive_and_wait();  // 1: the tables are built, prep is written
            SigPrep wp = hp;
            if (k == 1) sig_prep_load_pair(wp, prep);  // the comb wave's scalars
            PrepWalk walk(wp, W, ta, tr);
            met[k] = run_wave(walk, W, k == 0, ring, wbar);
          });
      // the undivided sums, and what the pipelined ones are compared with
      PrepWalk ref(hp, W, ta, tr);
      fe S[4];
      for (int l = 0; l < 4; l++)
        th.emplace_back([&, l] {
          HostQuad q{l, &ex};
          auto get_s = [&](int win, fe& c) {
            wbar.arrive_and_wait();  // window win
            if (l == 0) {
              int dA, dR;
              ref.next(dA, dR);
              h_window_addend(S, ref, dA, dR, ref.r_flip);
            }
            ex.bar.arrive_and_wait();
            if (pipe) {
              fe got[4];
              if (!ring.load(win, got, false)) differs++;
              for (int k = 0; k < 4; k++)
                if (!fe_same(S[k], got[k])) differs++;
              c = got[l];
              ex.bar.arrive_and_wait();  // every lane has read the slot
              if (l == 0) ring.slot[win & 1].unread = 0;
            } else {
              c = S[l];
            }
            ex.bar.arrive_and_wait();
          };
          auto get_ps = [&](fe& ps) {
            if (late) return false;
            fe_mul(ps, *xyz[q_p2_factor_a(l)], *xyz[q_p2_factor_b(l)]);
            return true;
          };
          auto get_prep = [&](SigPrep& p) {
            wbar.arrive_and_wait();  // 1
            sig_prep_load_pair(p, prep);
          };
          res[l] = mode ? q_verify_hs_fold<MODE_ZIP215>(q, pkw, sigw, bt, 16 - pre, ta[l], tr[l], get_ps, get_prep, get_s)
                        : q_verify_hs_fold<MODE_GO_STDLIB>(q, pkw, sigw, bt, 16 - pre, ta[l], tr[l], get_ps, get_prep,
                                                           get_s);
        });
      for (auto& t : th) t.join();
      if (res[0] != res[1] || res[0] != res[2] || res[0] != res[3]) {
        fprintf(stderr, "lanes disagree on vector %u (pipe %d)\n", i, pipe);
        return 2;
      }
      if (differs || ring.errors) {
        fprintf(stderr, "vector %u: %d pipelined sums differ from h_window_addend's, %d stores out of turn\n", i,
                differs.load(), ring.errors.load());
        return 3;
      }
      if (met[0] != W - 1 || met[1] != W - 1) {
        fprintf(stderr, "vector %u: the waves met %d and %d of %d barriers\n", i, met[0], met[1], W - 1);
        return 4;
      }
      out[pipe ? 0 : 1] = res[0];
    }
    fwrite(out, 1, 2, stdout);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "halves")) return run_halves();
  if (argc > 1 && !strcmp(argv[1], "schedule")) return run_schedule();
  if (argc > 1 && !strcmp(argv[1], "fold")) return run_fold(argc > 2 && !strcmp(argv[2], "wide"));
  return 1;
}
