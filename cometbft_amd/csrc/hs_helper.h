// hs_helper.h -- the helper wave of the helper-summed quad kernels
// (kernels.hip k_verify_quad_hs_fold and k_verify_quad_hs, sr25519.hip
// k_verify_sr25519_quad_hs): the
// workgroup's window count before barrier 1, and after it the per-window sums
// S_w = [dA](-A) + [dR](-/+R) of its 48 signatures (quad.h h_window_addend,
// one per lane) handed to the quads through a 2-slot LDS ring at one barrier
// per window, then the helper's part of [u]B. The quad side is quad.h
// q_hs_straus. Device code only.
#pragma once
#include "devtables.h"
#include "quad.h"

namespace cmtv {

// [u]B's comb positions the helper adds while the quads build their tables
// (the quads add the rest inside their windows); CMTV_HS_PRE overrides it.
// Each one the helper takes saves the quads ~1 us of window time and costs
// barrier 1 ~3 us once the helper arrives last. Ed25519: 6 with the message
// in HBM (the helper reaches barrier 1 with the quads, profiles/
// r05_ed_phase_hbm.json); 3 when the helper builds the sign-bytes itself
// from zero-copy staged templates (the node's commit path: its first loads
// cross PCIe; profiles/r05_hs_pre_ab.txt). sr25519: none -- its merlin
// transcript already brings the helper to barrier 1 with the quads (1 and 2
// measured 1-3% slower, profiles/r05_sr_hs_pre_ab.txt)
constexpr int kHsCombPre = 6, kHsCombPreFused = 3, kHsCombPreSr = 0;
// one ring slot: 3 quad waves x 5 uint2 x 64 lanes
constexpr uint32_t kHsSlotU2 = 3 * 5 * 64;
// a quad wave's two tables in LDS: 2 points x 9 entries x 5 uint2 x 64 lanes
constexpr uint32_t kHsTabU2 = 2 * 9 * 5 * 64;

// the folded form's P_s = [s]B of one signature on its way from the comb wave
// to the quads: X, Y, Z, 10 words each
constexpr uint32_t kHsPsWords = 30;
// ... and the comb positions of [s]B that wave adds (the top ones; the quads
// add the rest before they wait for it); CMTV_HS_PRE overrides it. 15 since
// the serial carry chain shortened the quads' decode and tables more than the
// comb wave's additions, so that the quads came to the flag 11k cycles before
// P_s: 15 and 14 measure 1.4% faster than all 16, 13 1.0% (profiles/
// r08_fe_carry_ab.txt; before it 15, 14 and 13 were 0.3%, 0.8% and 1.4%
// slower than 16, profiles/r07_hs_fold_ab.txt)
constexpr int kHsFoldCombPre = 15;

// the number of [u]B's comb positions the helper takes (launcher's hs_tune
// bits 0..7: CMTV_HS_PRE + 1; 0 = the kernel's default)
__device__ __forceinline__ int hs_comb_pre(uint32_t hs_tune, int dflt) {
  const int c = (hs_tune & 0xFFu) ? (int)(hs_tune & 0xFFu) - 1 : dflt;
  return c > 16 ? 16 : c;
}

// The workgroup's window count: quad.h q_wave_windows over the helper's 48
// signatures (lane t < 48 holds signature t's flags)
__device__ __forceinline__ int hs_workgroup_windows(uint32_t flags, uint32_t t) {
  const bool wide = __ballot(t < 48 && (flags & 2u) != 0) != 0;
  int W = HS_WINDOWS;
#pragma unroll 1
  for (int x = HS_WINDOWS; x < HS_MAX_WINDOWS; x++) W += __ballot(t < 48 && (int)((flags >> 8) & 0xFFu) > x) ? 1 : 0;
  return wide ? HS_WIDE_WINDOWS : W;
}

// lane t < 48 writes coordinate c of its signature's cached sum where the
// quads' hs_slot_load finds it
__device__ __forceinline__ void hs_slot_store_coord(uint2* dst, uint32_t t, int c, const fe& v) {
  if (t < 48) {
#pragma unroll
    for (int k = 0; k < 5; k++) dst[(t >> 4) * 320 + k * 64 + 4 * (t & 15) + c] = make_uint2(v.v[2 * k], v.v[2 * k + 1]);
  }
}

// ... and all four, out[0..3]
__device__ __forceinline__ void hs_slot_store(uint2* dst, uint32_t t, const fe* out) {
#pragma unroll
  for (int c = 0; c < 4; c++) hs_slot_store_coord(dst, t, c, out[c]);
}

// A helper lane's walk down its signature's windows after barrier 1: the
// digits of k1 and k2 from window W-2 down (the top window is the quads' own)
// and the read of the quads' tables h_window_addend takes. tabs = the
// workgroup's three quad waves' tables; lane t < 48 owns signature t (quad
// wave t >> 4, quad t & 15).
struct HsWalk {
  uint32_t tA[8], tR[8];
  const uint2* tw;
  bool r_flip;
  __device__ __forceinline__ HsWalk(const SigPrep& p, int W, const uint2* tabs, uint32_t t) {
    const uint32_t slot = t < 48 ? t : 47;
    r_flip = (p.flags & 1u) != 0;
    hs_digits16(tA, p.k1, W);
    hs_digits16(tR, p.k2, W);
    sc_shift_out(tA, 4);
    sc_shift_out(tR, 4);
    tw = tabs + (slot >> 4) * kHsTabU2 + 4 * (slot & 15);
  }
  __device__ __forceinline__ void next(int& dA, int& dR) {
    dA = (int)sc_shift_out(tA, 4) - 8;
    dR = (int)sc_shift_out(tR, 4) - 8;
  }
  __device__ __forceinline__ void operator()(int P, int e, int c, fe& r) const {
    const uint2* src = tw + (P * 9 + e) * 5 * 64 + c;
#pragma unroll
    for (int k = 0; k < 5; k++) {
      const uint2 x = src[k * 64];
      r.v[2 * k] = x.x;
      r.v[2 * k + 1] = x.y;
    }
  }
};

// After barrier 1: windows W-2 .. 0 (the top one is the quads'), each sum
// written to ring slot (win & 1) before that window's barrier (a slot is
// rewritten only after the quads read it, one barrier later). tabs = the
// workgroup's three quad waves' tables, ring = 2 slots; lane t < 48 owns
// signature t (quad wave t >> 4, quad t & 15). Meets W - 1 barriers. hwait:
// cycles spent at the window barriers when clock() counts them (the probe
// build). This is the whole helper of the folded form (k_verify_quad_hs_fold),
// which has no [u]B.
template <class Clock>
__device__ __forceinline__ void hs_helper_sums(const SigPrep& p, int W, const uint2* tabs, uint2* ring, uint32_t t,
                                               const Clock& clock, uint64_t& hwait) {
  HsWalk rd(p, W, tabs, t);
#pragma unroll 1
  for (int win = W - 2; win >= 0; win--) {
    int dA, dR;
    rd.next(dA, dR);
    fe out[4];
    h_window_addend(out, rd, dA, dR, rd.r_flip);
    hs_slot_store(ring + (win & 1) * kHsSlotU2, t, out);
    const uint64_t c0 = clock();
    __syncthreads();  // window win
    hwait += clock() - c0;
  }
}

// hs_helper_sums software-pipelined over the two waves of the folded form's
// helper SIMD (k_verify_quad_hs_fold; quad.h h_sums_pipe): both the hash
// helper (lead) and the comb wave run this, on the same lanes, digits and
// table reads, and each forms every second window's sum -- its front half in
// one interval, its back half and the store to ring slot (win & 1) in the
// next, the interval in which hs_helper_sums stores it. The window barrier
// is the only synchronisation; both meet all W - 1. In interval 0 the lead
// forms all of S_{W-2} while the other wave starts S_{W-3} beside it, and the
// quads need S_{W-2} after one addition and four doublings: the caller gives
// the lead the SIMD's issue priority for it, and first_done() after that
// first barrier takes it back.
template <class Clock, class FirstDone>
__device__ __forceinline__ void hs_helper_sums_pipe(const SigPrep& p, int W, const uint2* tabs, uint2* ring,
                                                    uint32_t t, bool lead, const Clock& clock, uint64_t& hwait,
                                                    const FirstDone& first_done) {
  HsWalk rd(p, W, tabs, t);
  h_sums_pipe(
      rd, W, lead, [&](int win, const fe* out) { hs_slot_store(ring + (win & 1) * kHsSlotU2, t, out); },
      [&](int win) {
        const uint64_t c0 = clock();
        __syncthreads();  // window win
        hwait += clock() - c0;
        if (win == W - 2) first_done();
      });
}

// hs_helper_sums split over the two waves of the folded form's helper SIMD
// (k_verify_quad_hs_fold): the hash helper runs hs_helper_sums_eh and the comb
// wave hs_helper_sums_fg, on the same lanes, digits and table reads. Per
// window the comb wave computes F, G and the sum's 2Z (quad.h
// h_window_addend_fg), writes 2Z to the ring slot and F and G to the exchange
// area fg (kHsFgU2 uint2: word pair k of F at [k * 48 + t], of G at
// [(5 + k) * 48 + t]), and publishes the window's index in *fg_ready behind a
// release fence; the hash helper computes E, H and 2dT (h_window_addend_eh),
// takes F and G once *fg_ready names its window, and finishes Y-X and Y+X
// (h_window_addend_xy). Both meet every window barrier, W - 1 in all.
//
// fg_wait bounds the hash helper's poll, so the wait never decides a verdict:
// when it runs out the helper computes the whole of h_window_addend for that
// window itself (the comb wave may still store the same 2Z later, before the
// window's barrier) and hs_helper_sums_eh returns true. fg_wait = 0: it never
// polls, and the comb wave is expected to idle at the barriers instead.
constexpr uint32_t kHsFgU2 = 2 * 5 * 48;
constexpr uint32_t kHsFgNone = 0xFFFFFFFFu;  // *fg_ready before the first window

__device__ __forceinline__ void hs_helper_sums_fg(const SigPrep& p, int W, const uint2* tabs, uint2* ring, uint2* fg,
                                                  uint32_t* fg_ready, uint32_t t) {
  HsWalk rd(p, W, tabs, t);
#pragma unroll 1
  for (int win = W - 2; win >= 0; win--) {
    int dA, dR;
    rd.next(dA, dR);
    fe z2, f, g;
    h_window_addend_fg(z2, f, g, rd, dA, dR, rd.r_flip);
    if (t < 48) {
#pragma unroll
      for (int k = 0; k < 5; k++) {
        fg[k * 48 + t] = make_uint2(f.v[2 * k], f.v[2 * k + 1]);
        fg[(5 + k) * 48 + t] = make_uint2(g.v[2 * k], g.v[2 * k + 1]);
      }
    }
    hs_slot_store_coord(ring + (win & 1) * kHsSlotU2, t, 2, z2);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (t == 0) __hip_atomic_store(fg_ready, (uint32_t)win, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();  // window win
  }
}

// fwait: cycles at the poll when clock() counts them (the probe build)
template <class Clock>
__device__ __forceinline__ bool hs_helper_sums_eh(const SigPrep& p, int W, const uint2* tabs, uint2* ring,
                                                  const uint2* fg, uint32_t* fg_ready, uint32_t fg_wait, uint32_t t,
                                                  const Clock& clock, uint64_t& hwait, uint64_t& fwait) {
  HsWalk rd(p, W, tabs, t);
  const uint32_t slot = t < 48 ? t : 47;
  bool late = false;
#pragma unroll 1
  for (int win = W - 2; win >= 0; win--) {
    int dA, dR;
    rd.next(dA, dR);
    uint2* dst = ring + (win & 1) * kHsSlotU2;
    fe out[4], e, h;
    h_window_addend_eh(out[3], e, h, rd, dA, dR, rd.r_flip);
    const uint64_t f0 = clock();
    bool ready = false;
    for (uint32_t spins = 0; spins < fg_wait; spins++) {
      ready = __hip_atomic_load(fg_ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == (uint32_t)win;
      if (ready) break;
      __builtin_amdgcn_s_sleep(1);
    }
    fwait += clock() - f0;
    if (__builtin_expect(__ballot(ready) != __ballot(1), 0)) {
      late = true;
      h_window_addend(out, rd, dA, dR, rd.r_flip);
      hs_slot_store(dst, t, out);
    } else {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      fe f, g;
#pragma unroll
      for (int k = 0; k < 5; k++) {
        const uint2 a = fg[k * 48 + slot], b = fg[(5 + k) * 48 + slot];
        f.v[2 * k] = a.x;
        f.v[2 * k + 1] = a.y;
        g.v[2 * k] = b.x;
        g.v[2 * k + 1] = b.y;
      }
      h_window_addend_xy(out[0], out[1], e, f, g, h);
      hs_slot_store_coord(dst, t, 0, out[0]);
      hs_slot_store_coord(dst, t, 1, out[1]);
      hs_slot_store_coord(dst, t, 3, out[3]);
    }
    const uint64_t c0 = clock();
    __syncthreads();  // window win
    hwait += clock() - c0;
  }
  return late;
}

// hs_helper_sums, then [u]B's partial sum bc.P in slot 1 before the last
// barrier, which the caller meets: W barriers in all
template <class Clock>
__device__ __forceinline__ void hs_helper_windows(const SigPrep& p, int W, const BComb16& bc, const uint2* tabs,
                                                  uint2* ring, uint32_t t, const Clock& clock, uint64_t& hwait) {
  hs_helper_sums(p, W, tabs, ring, t, clock, hwait);
  fe out[4], d2;
  fe_sub(out[0], bc.P.Y, bc.P.X);
  fe_add(out[1], bc.P.Y, bc.P.X);
  fe_add(out[2], bc.P.Z, bc.P.Z);
  fe_const_d2(d2);
  fe_mul(out[3], bc.P.T, d2);
  hs_slot_store(ring + kHsSlotU2, t, out);  // slot 1: last read for window 1, before barrier 0
}

// the quads' read of their coordinate of a ring slot (or of [u]B)
__device__ __forceinline__ void hs_slot_load(const uint2* sl, uint32_t wave, uint32_t t, fe& c) {
#pragma unroll
  for (int k = 0; k < 5; k++) {
    const uint2 x = sl[wave * 320 + k * 64 + t];
    c.v[2 * k] = x.x;
    c.v[2 * k + 1] = x.y;
  }
}

}  // namespace cmtv
