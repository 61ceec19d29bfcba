// Host emulation of k_verify_quad_hs_fold's path (cometbft_amd/csrc/quad.h
// q_verify_hs_fold): [s]B folded into R, the windows without fixed-base
// additions. Four std::threads run the quad's source in lockstep (as
// quadcheck.cpp); what the kernel's other waves compute is computed once per
// signature the way they do it: the top i % 17 comb positions of [s]B by
// BComb16Ahead on s, handed over as (X, Y, Z) (the comb wave; the quads add the
// other positions themselves), the scalars without u (the hash helper) and
// every window's summed addend from the four lanes' tables (h_window_addend).
// The operand bound assertions are on (CMTV_BOUNDS_CHECK).
//   argv[1] == "late": the comb wave's share never arrives and the quads add
//                      those comb rows too, the path of a quad wave that
//                      stopped waiting
//   argv[2] == "wide": the 64-window fallback for every signature
//   stdin as quadcheck.cpp: u32 n, n x { u8 mode, pk[32], sig[64], u32 mlen, msg }
//   stdout: n x { the folded verdict, q_verify_hs's verdict }
// The window count is the signature's own raised by i % 3, as a workgroup's
// count can be any other signature's. Test infrastructure only.
#define CMTV_HD inline
#define CMTV_BOUNDS_CHECK 1
#include <atomic>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>
#include "../../cometbft_amd/csrc/quad.h"
#include "lazy_btab.h"

using namespace cmtv;

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

int main(int argc, char** argv) {
  const bool late = argc > 1 && !strcmp(argv[1], "late");
  const bool force_wide = argc > 2 && !strcmp(argv[2], "wide");
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
      uint32_t prep[SIG_PREP_WORDS];
      if (fold)
        sig_prep_store_pair(prep, hp);
      else
        sig_prep_store(prep, hp);
      uint32_t tA[8], tR[8];
      hs_digits16(tA, hp.k1, W);
      hs_digits16(tR, hp.k2, W);
      sc_shift_out(tA, 4);
      sc_shift_out(tR, 4);
      // the comb wave: its positions of [s]B from s alone, whatever s is
      const int pre = (int)(i % 17);
      BComb16Ahead bc;
      bc.init(sigw + 8, bt);
      for (int k = 0; k < pre; k++) bc.step(bt);
      const fe* xyz[3] = {&bc.P.X, &bc.P.Y, &bc.P.Z};
      // q_verify_hs's [u]B, all of it from its helper
      uint32_t bpt[40];
      {
        ge_p3 Bp;
        q_bcomb16(Bp, hp.u, bt);
        bpoint_store(bpt, Bp);
      }
      Exchange ex;
      bool res[4];
      QArrayTab ta[4], tr[4];
      fe S[4];
      std::vector<std::thread> th;
      for (int l = 0; l < 4; l++)
        th.emplace_back([&, l] {
          HostQuad q{l, &ex};
          auto get_s = [&](int, fe& c) {
            ex.bar.arrive_and_wait();  // every lane's tables are built
            if (l == 0) {
              const int dA = (int)sc_shift_out(tA, 4) - 8;
              const int dR = (int)sc_shift_out(tR, 4) - 8;
              auto rd = [&](int P, int e, int cc, fe& r) { r = (P == 0 ? ta[cc] : tr[cc]).t[e]; };
              h_window_addend(S, rd, dA, dR, (hp.flags & 1u) != 0);
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
      out[fold ? 0 : 1] = res[0];
    }
    fwrite(out, 1, 2, stdout);
  }
  return 0;
}
