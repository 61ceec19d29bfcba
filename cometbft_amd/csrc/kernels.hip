// kernels.hip -- the generic Ed25519 verify kernels of libcmtverify (gfx950)
// and their launcher, launch_verify. The registered-key forms are in
// keyed_forms.hip and keyed_lane.hip, the table, key generation and signing
// kernels in keygen.hip, the device code they share in kernel_parts.h.
//
//   k_verify<MODE>: one signature per lane: SHA-512 + mod-L + decompression +
//                   Straus [s]B - [k]A + GO_STDLIB / ZIP215 final check, then a
//                   wavefront ballot packs 64 verdicts into one bitmap word
//   k_verify_quad_hs_fold / k_verify_quad_hs / k_verify_oct_split /
//   k_verify_row_split / k_verify_row4_split<MODE>: the same with 4 / 4 / 8 /
//                   64 / 256 lanes per signature and a helper wave (smaller
//                   batches; kernels.h forms)
//
// Memory layout (HBM):
//   pk   : n x 32 B   (row i = 8 words, read as 2 x dwordx4)
//   sig  : n x 64 B   (row i = 16 words, 4 x dwordx4)
//   msg  : flat bytes + (n+1) u32 offsets
//   btab : 2 x 128 rows x 36 words (ypx, ymx, 2dxy; 10 limbs + 2 pad each) = 36 KiB:
//          (1..128)B, then (1..128)[2^124]B (quad kernel's high-half table),
//          L1/L2-resident; one coordinate gathered per lane as 2 x dwordx4 + dwordx2
//   atab : per-lane (1..8)(-A) cached table, word-major / lane-minor
//          [(e*40 + w) * stride + lane] so each of the 40 word loads of a row
//          is one coalesced 256-byte wave access when lanes share the digit
//          magnitude, and at most 8 distinct 256-byte segments otherwise.
#include <hip/hip_runtime.h>

#include "devtables.h"
#include "hs_helper.h"
#include "kernel_parts.h"
#include "kernels.h"
#include "phase_probe.h"
#include "quad.h"
#include "signbytes.h"
#include "verify_core.h"

CMTV_PHASE_BUFFER()  // cmtv_debug_phase_times

// Minimum waves per SIMD the verify kernel is compiled for (the second
// __launch_bounds__ argument): caps VGPRs at 512 / waves.
#ifndef CMTV_QUAD_WAVES_PER_EU
#define CMTV_QUAD_WAVES_PER_EU 1
#endif

#ifndef CMTV_VERIFY_WAVES_PER_EU
#define CMTV_VERIFY_WAVES_PER_EU 2
#endif

namespace cmtv {

template <uint32_t MODE>
__global__ __launch_bounds__(64, CMTV_VERIFY_WAVES_PER_EU) void k_verify(uint32_t n, const uint32_t* __restrict__ pk,
                                               const uint32_t* __restrict__ sig, const uint8_t* __restrict__ msg,
                                               const uint32_t* __restrict__ off, const uint32_t* __restrict__ btab,
                                               uint32_t* __restrict__ atab, uint8_t* __restrict__ out_valid,
                                               uint64_t* __restrict__ out_bitmap) {
  const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
  const bool active = gid < n;
  const uint32_t i = active ? gid : n - 1;
  const uint32_t m0 = off[i], m1 = off[i + 1];
  DevATab at{atab, gridDim.x * 64u, gid};
  DevBTab bt{btab};
  // verify_one, not verify_one_half: with one signature per lane the kernel is
  // bound by the latency of its per-lane table loads (tables of 2 x 64 x 1280 B
  // per wave miss L2), and the half-size-scalar form keeps the number of
  // dependent lookups (68 vs 64) while removing the doublings that hid them:
  // measured 60.0 vs 61.7 M verifs/s at 1M signatures.
  bool v = verify_one<MODE>(pk + 8 * (size_t)i, sig + 16 * (size_t)i, msg + m0, m1 - m0, at, bt);
  lane_verdict_store(gid, active, v, out_valid, out_bitmap);
}

// The helper-summed quad verifier (quad.h q_verify_hs, hs_helper.h): a 4-wave
// workgroup takes 48 signatures; waves 0-2 are quad waves (16 signatures
// each) and wave 3 hashes and splits the scalars of all 48 (one lane each,
// q_prepare, the templated sign-bytes included) while they decompress A and R
// and build both tables (extended points); the scalars reach them at barrier
// 1. LDS (3 x 45 KiB tables + scalars + the window ring) allows one workgroup
// per CU, i.e. 4 waves on its 4 SIMDs: 256 workgroups = 12,288 signatures per
// round. After barrier 1 the helper wave sums every window's two table entries for its 48
// signatures (h_window_addend, one per lane) and hands the sums over through a
// 2-slot LDS ring, one barrier per window: the quads' windows lose one of
// their two additions. [u]B: while the quads build their tables the helper
// adds the top kHsCombPre positions of u's 16-position comb and hands that
// part over at a last barrier; the quads add the other digits inside their
// windows (q_hs_straus). Nothing of [u]B runs inside the helper's window
// loop: the per-window barriers go at the slower side's pace, so helper work
// there stalls all three quads (measured: comb additions cut into
// one-multiplication phases, two per window, cost the quads 1.6k cycles a
// window; tools/gpu_hs.sh). The slot ring overlays the fused sign-bytes
// buffer (dead once the hashes are done). hs_tune (the launcher's kflags bits
// 16..31, CMTV_HS_PRE) overrides kHsCombPre (0..16) for tuning.
template <uint32_t MODE>
__global__ __launch_bounds__(256, CMTV_QUAD_WAVES_PER_EU) void k_verify_quad_hs(
    uint32_t n, const uint32_t* __restrict__ pk, const uint32_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    const uint32_t* __restrict__ off, const uint32_t* __restrict__ btab, uint8_t* __restrict__ out_valid,
    uint64_t* __restrict__ out_bitmap, uint32_t force_wide, SbFuse sb, uint32_t hs_tune, RowSlot tags) {
  CMTV_URGENT();
  const uint32_t wave = threadIdx.x >> 6, t = threadIdx.x & 63;
  const uint32_t base = blockIdx.x * 48;
  const int comb_pre = hs_comb_pre(hs_tune, sb.tmpls ? kHsCombPreFused : kHsCombPre);
  __shared__ uint32_t prep[48][SIG_PREP_WORDS + 1];
  __shared__ uint2 tab_lds[3][kHsTabU2];
  __shared__ uint2 xbuf[2 * kHsSlotU2];  // sign-bytes (48 x kSbFuseMaxMsg B), then the 2-slot ring
  static_assert(sizeof(xbuf) >= 48 * kSbFuseMaxMsg, "ring must cover the sign-bytes buffer");
  CMTV_STAMP(0);
  if (wave == 3) {
    const uint32_t slot = t < 48 ? t : 47;
    const uint32_t s = base + slot;
    const uint32_t i = s < n ? s : n - 1;
    const uint8_t* mp;
    uint32_t ml;
    CMTV_STAMP(5);  // the helper's slots 5 / 4: before / after locating its message
    helper_message(sb, i, msg, off, reinterpret_cast<uint32_t*>(xbuf) + slot * (kSbFuseMaxMsg / 4), mp, ml);
#ifdef CMTV_PHASE_PROBE
    __builtin_amdgcn_s_waitcnt(0);  // the offsets arrived
#endif
    CMTV_STAMP(4);
    SigPrep p;
    q_prepare<MODE>(p, pk + 8 * (size_t)i, sig + 16 * (size_t)i, mp, ml, force_wide != 0,
                    [] { CMTV_STAMP(7); });
    const int W = hs_workgroup_windows(p.flags, t);
    p.flags |= (uint32_t)W << 16;
    if (t < 48) sig_prep_store(prep[t], p);
    BComb16 bc;
    bc.init(p.u);
    const DevBTab bt{btab};
#pragma unroll 1
    for (int k = 0; k < comb_pre; k++) bc.step(bt);
    CMTV_STAMP(1);
    __syncthreads();  // 1: the scalars; the tables are built
    CMTV_STAMP(2);
    uint64_t hwait = 0;  // probe build: cycles the helper waits at the window barriers
    hs_helper_windows(p, W, bc, &tab_lds[0][0], xbuf, t, [] { return (uint64_t)CMTV_CLOCK(); }, hwait);
    CMTV_STAMP_VAL(6, hwait);
    CMTV_STAMP(3);
    __syncthreads();  // B: [u]B
    return;
  }
  const uint32_t ls = wave * 16 + (t >> 2);
  const uint32_t s = base + ls;
  const bool active = s < n;
  const uint32_t i = active ? s : n - 1;
  DevQuad q;
  DevATabQ ta{tab_lds[wave], t}, tr{tab_lds[wave] + 9 * 5 * 64, t};
  uint64_t qwait = 0;  // probe build: cycles this quad wave waits at the window barriers
  (void)qwait;
  DevBTabQ bt{btab};
  bool v = q_verify_hs<MODE>(
      q, pk + 8 * (size_t)i, sig + 16 * (size_t)i, bt, ta, tr, 16 - comb_pre,
      [&](SigPrep& p) {
        CMTV_STAMP(1);
        __syncthreads();
        CMTV_STAMP(2);
        sig_prep_load(p, prep[ls]);
      },
      [&](int win, fe& c) {
        const uint64_t c0 = CMTV_CLOCK();
        __syncthreads();
        qwait += CMTV_CLOCK() - c0;
        hs_slot_load(xbuf + (win & 1) * kHsSlotU2, wave, t, c);
      },
      [&](fe& c) {
        CMTV_STAMP(3);
        __syncthreads();
        CMTV_STAMP(4);
        hs_slot_load(xbuf + kHsSlotU2, wave, t, c);
      });
  CMTV_STAMP(5);
  CMTV_STAMP_VAL(6, qwait);
  quad_verdict_store(v, active, s, n, wave, t, out_valid, out_bitmap, tags);
}

// k_verify_quad_hs with [s]B folded into R (quad.h q_verify_hs_fold): a fifth
// wave, the comb wave, runs the 16-position comb on every signature's s from
// the first cycle, one lane per signature (BComb16Ahead; it needs no hash),
// and publishes P_s = [s]B through an LDS flag. The quads build A's table,
// take P_s, form P_s - R and build its table; their windows then carry no
// fixed-base addition at all, the helper computes no u = k2 s mod L, and the
// last barrier with its [u]B addition is gone.
//
// 5 waves on 4 SIMDs: wave 4 lands on wave 0's SIMD (the probe's HW_ID stamp,
// every workgroup), so wave 0 is the hash helper and waves 1-3 are the quads.
// The helper reaches barrier 1 some 56k cycles before the quads even with
// the comb beside it, so the comb fills that SIMD's slack; beside a quad wave
// the same comb costs the kernel 12%. The comb wave takes the top
// kHsFoldCombPre positions (15 of the 16, measured best; CMTV_HS_PRE overrides it)
// and the quads add the rest themselves before they look at the flag.
//
// P_s travels as (X, Y, Z), 30 words a signature, in the tail of xbuf: the
// sign-bytes take its first 48 x kSbFuseMaxMsg bytes and the ring is written
// only after barrier 1, which the comb wave meets after its stores -- so a
// comb wave that comes late harms nothing, which an entry slot of R's table
// (rewritten by a quad wave that stopped waiting) would not allow. A quad lane
// multiplies the two factors of its coordinate of (XZ, YZ, Z^2, XY), the same
// point as an extended one.
//
// The quads poll the flag at most ps_wait times. The verdict never depends on
// that wait: a quad wave that stops waiting adds the comb wave's rows itself
// (q_sbase16_add) and counts itself in diag[kDiagLatePs] (cmtv_stats.
// late_ps_waves); ps_wait = 0 (the CMTV_FORCE_PS_LATE test knob) skips the
// comb wave's work and the flag, so every quad wave takes that path. The
// comb wave meets barrier 1 and every window barrier (the count is in prep
// after barrier 1) and returns with the helper. hs_tune bits 8..10
// (CMTV_HS_FOLD_TUNE): 1 = the hash helper is wave 3 and the quads waves 0-2
// (the comb then shares a quad's SIMD), 2 / 4 = the comb wave at issue
// priority 0 / 3.
//
// After barrier 1 the helper's SIMD decides the window barriers when one wave
// forms S_w alone at the lone-wave issue rate, so with hs_tune's
// kHsTuneSumSplit (CMTV_HS_SUM_SPLIT=1; off by default, it measured a tie:
// DESIGN.md 5 round 9) the two waves of that SIMD share every
// window's sum (hs_helper.h hs_helper_sums_eh / _fg): the comb wave takes the
// T and Z half (F, G, 2Z; the scalars from prep), the hash helper the X and Y
// half and the last two products, F and G crossing through fgx. The helper's
// poll for them is bounded like the quads' for P_s: when it runs out the
// helper forms the whole sum itself, and the workgroup counts once in
// diag[kDiagLateSum] (cmtv_late_sum_waves); kHsTuneFgLate (the
// CMTV_FORCE_FG_LATE test knob) makes the comb wave idle and every window take
// that path.
//
// PIPE (the launcher picks it for hs_tune's kHsTunePipe, CMTV_HS_SUM_PIPE,
// unless kHsTuneSumSplit is set or the helper is on wave 3) keeps every sum
// whole and pipelines the sums over the two waves instead (hs_helper.h
// hs_helper_sums_pipe): each forms every second window's sum, half of it per
// window, and the window barrier stays the only synchronisation -- no flag, no
// poll, no exchange area, no late path. It is a kernel of its own, so that the
// other one stays instruction for instruction what it was: a rebuild of this
// kernel around unrelated code has moved its time by 2% either way (DESIGN.md
// 5 rounds 9 and 10).
template <uint32_t MODE, bool PIPE>
__global__ __launch_bounds__(320, 1) void k_verify_quad_hs_fold(
    uint32_t n, const uint32_t* __restrict__ pk, const uint32_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    const uint32_t* __restrict__ off, const uint32_t* __restrict__ btab, uint8_t* __restrict__ out_valid,
    uint64_t* __restrict__ out_bitmap, uint32_t force_wide, SbFuse sb, uint32_t hs_tune, uint32_t ps_wait,
    uint32_t* __restrict__ diag, RowSlot tags) {
  CMTV_URGENT();
  const uint32_t hw = threadIdx.x >> 6, t = threadIdx.x & 63;
  const uint32_t base = blockIdx.x * 48;
  const uint32_t tune = hs_tune >> 8;
  const int comb_pre = hs_comb_pre(hs_tune, kHsFoldCombPre);
  const uint32_t helper_wave = (tune & 1u) ? 3u : 0u;
  // the window sums split over the helper and the comb wave; not with the
  // helper on wave 3, where the comb wave's share would take a quad's issue slots
  const bool sum_split = (hs_tune & kHsTuneSumSplit) != 0 && helper_wave == 0;
  const bool fg_late = (hs_tune & kHsTuneFgLate) != 0;
  __shared__ uint32_t prep[48][SIG_PREP_WORDS + 1];
  __shared__ uint2 tab_lds[3][kHsTabU2];
  __shared__ uint2 xbuf[2 * kHsSlotU2];  // sign-bytes | P_s, then the 2-slot ring
  __shared__ uint32_t ps_ready;
  // F and G of the window in flight, from the comb wave to the hash helper
  // (hs_helper.h hs_helper_sums_fg / _eh), and the index of the window they
  // belong to. One copy is enough, and the window barrier is its only reuse
  // fence: the comb wave writes window w-1's F and G only after barrier w, and
  // the helper has read window w's before it reaches barrier w.
  __shared__ uint2 fgx[kHsFgU2];
  __shared__ uint32_t fg_ready;
  static_assert(sizeof(xbuf) >= 48 * (kSbFuseMaxMsg + 4 * kHsPsWords), "P_s goes behind the sign-bytes buffer");
  static_assert(sizeof(prep) + sizeof(tab_lds) + sizeof(xbuf) + sizeof(fgx) + 2 * sizeof(uint32_t) <= 160 * 1024,
                "a workgroup's LDS");
  uint32_t* pspt = reinterpret_cast<uint32_t*>(xbuf) + 48 * (kSbFuseMaxMsg / 4);
  // probe slots: 0 entry, 6 HW_ID; 1 / 2 before / after barrier 1; comb wave
  // 3 = P_s published; helper 3 = its last sum, 7 = cycles at the window
  // barriers, 4 = cycles at its polls for F and G; quads 4 = P_s taken,
  // 3 = cycles at the flag, 5 = exit, 7 as the helper; PIPE: comb wave 7 as
  // the helper
  CMTV_STAMP5(0);
  CMTV_HWID5();
  if (threadIdx.x == 0) {
    ps_ready = 0u;
    fg_ready = kHsFgNone;
  }
  __syncthreads();  // the flags are clear before any wave can set or read them
  if (hw == 4) {
    if (tune & 2u) __builtin_amdgcn_s_setprio(0);
    if (tune & 4u) __builtin_amdgcn_s_setprio(3);
    if (ps_wait != 0) {
      const uint32_t slot = t < 48 ? t : 47;
      const uint32_t s = base + slot;
      const uint32_t i = s < n ? s : n - 1;
      uint32_t sw[8];
      load_words(sw, sig + 16 * (size_t)i + 8, 2);
      const DevBTab bt{btab};
      BComb16Ahead bc;
      bc.init(sw, bt);
#pragma unroll 1
      for (int k = 0; k < comb_pre; k++) bc.step(bt);
      if (t < 48) {
#pragma unroll
        for (int j = 0; j < 10; j++) {
          pspt[t * kHsPsWords + j] = bc.P.X.v[j];
          pspt[t * kHsPsWords + 10 + j] = bc.P.Y.v[j];
          pspt[t * kHsPsWords + 20 + j] = bc.P.Z.v[j];
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      if (t == 0) __hip_atomic_store(&ps_ready, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    CMTV_STAMP5(3);
    CMTV_STAMP5(1);
    __syncthreads();  // 1
    CMTV_STAMP5(2);
    const int W = (int)__builtin_amdgcn_readfirstlane((prep[0][24] >> 16) & 0xFFu);
    if constexpr (PIPE) {
      SigPrep p;
      sig_prep_load_pair(p, prep[t < 48 ? t : 47]);
      uint64_t hwait = 0;
      hs_helper_sums_pipe(
          p, W, &tab_lds[0][0], xbuf, t, false, [] { return (uint64_t)CMTV_CLOCK(); }, hwait, [] {});
      CMTV_STAMP5_VAL(7, hwait);
      return;
    }
    if (sum_split && !fg_late) {
      SigPrep p;
      sig_prep_load_pair(p, prep[t < 48 ? t : 47]);
      hs_helper_sums_fg(p, W, &tab_lds[0][0], xbuf, fgx, &fg_ready, t);
      return;
    }
#pragma unroll 1
    for (int win = W - 2; win >= 0; win--) __syncthreads();  // window win
    return;
  }
  if (hw == helper_wave) {
    const uint32_t slot = t < 48 ? t : 47;
    const uint32_t s = base + slot;
    const uint32_t i = s < n ? s : n - 1;
    const uint8_t* mp;
    uint32_t ml;
    helper_message(sb, i, msg, off, reinterpret_cast<uint32_t*>(xbuf) + slot * (kSbFuseMaxMsg / 4), mp, ml);
    SigPrep p;
    q_prepare<MODE>(p, pk + 8 * (size_t)i, sig + 16 * (size_t)i, mp, ml, force_wide != 0);
    const int W = hs_workgroup_windows(p.flags, t);
    p.flags |= (uint32_t)W << 16;
    if (t < 48) sig_prep_store_pair(prep[t], p);  // u is never used, so never computed
    CMTV_STAMP5(1);
    __syncthreads();  // 1: the scalars; the tables are built
    CMTV_STAMP5(2);
    uint64_t hwait = 0, fwait = 0;  // probe build: cycles the helper waits at the window barriers, for F and G
    (void)fwait;
    auto clock = [] { return (uint64_t)CMTV_CLOCK(); };
    if constexpr (PIPE) {
      // S_{W-2} is all this wave's, beside the comb wave's first front half, and
      // the quads need it after one addition and four doublings
      __builtin_amdgcn_s_setprio(3);
      hs_helper_sums_pipe(p, W, &tab_lds[0][0], xbuf, t, true, clock, hwait, [] { CMTV_URGENT(); });
    } else if (sum_split) {
      const bool late = hs_helper_sums_eh(p, W, &tab_lds[0][0], xbuf, fgx, &fg_ready, fg_late ? 0u : kPsWaitDefault, t,
                                          clock, hwait, fwait);
      if (late && t == 0 && diag) atomicAdd(diag + kDiagLateSum, 1u);
    } else {
      hs_helper_sums(p, W, &tab_lds[0][0], xbuf, t, clock, hwait);
    }
    CMTV_STAMP5_VAL(4, fwait);
    CMTV_STAMP5_VAL(7, hwait);
    CMTV_STAMP5(3);
    return;
  }
  const uint32_t wave = hw - (hw > helper_wave ? 1u : 0u);  // the quad wave's index, 0..2
  const uint32_t ls = wave * 16 + (t >> 2);
  const uint32_t s = base + ls;
  const bool active = s < n;
  const uint32_t i = active ? s : n - 1;
  DevQuad q;
  DevATabQ ta{tab_lds[wave], t}, tr{tab_lds[wave] + 9 * 5 * 64, t};
  uint64_t qwait = 0;  // probe build: cycles this quad wave waits at the window barriers
  (void)qwait;
  bool v = q_verify_hs_fold<MODE>(
      q, pk + 8 * (size_t)i, sig + 16 * (size_t)i, DevBTabQ{btab}, 16 - comb_pre, ta, tr,
      [&](fe& ps) {
        // the comb wave's flag, polled at most ps_wait times (a wave never
        // spins forever)
        const uint64_t c0 = CMTV_CLOCK();
        (void)c0;
        bool ready = false;
        for (uint32_t spins = 0; spins < ps_wait; spins++) {
          ready = __hip_atomic_load(&ps_ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0u;
          if (ready) break;
          __builtin_amdgcn_s_sleep(2);
        }
        CMTV_STAMP5_VAL(3, CMTV_CLOCK() - c0);
        if (__builtin_expect(__ballot(ready) != __ballot(1), 0)) {
          // the comb wave's share did not arrive in time: the quad adds those
          // comb rows too, so the wait bounds only the time, never the verdict
          if (t == 0 && diag) atomicAdd(diag + kDiagLatePs, 1u);
          return false;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const int lane = (int)(t & 3);
        const uint32_t* pp = pspt + ls * kHsPsWords;
        fe a, b;
#pragma unroll
        for (int j = 0; j < 10; j++) {
          a.v[j] = pp[10 * q_p2_factor_a(lane) + j];
          b.v[j] = pp[10 * q_p2_factor_b(lane) + j];
        }
        fe_mul(ps, a, b);
        CMTV_STAMP5(4);
        return true;
      },
      [&](SigPrep& p) {
        CMTV_STAMP5(1);
        __syncthreads();
        CMTV_STAMP5(2);
        sig_prep_load_pair(p, prep[ls]);
      },
      [&](int win, fe& c) {
        const uint64_t c0 = CMTV_CLOCK();
        __syncthreads();
        qwait += CMTV_CLOCK() - c0;
        hs_slot_load(xbuf + (win & 1) * kHsSlotU2, wave, t, c);
      });
  CMTV_STAMP5(5);
  CMTV_STAMP5_VAL(7, qwait);
  quad_verdict_store(v, active, s, n, wave, t, out_valid, out_bitmap, tags);
}

// whether a launch with these hs_tune bits runs k_verify_quad_hs_fold's PIPE form
static bool hs_fold_pipe(uint32_t hs_tune) {
  return (hs_tune & kHsTunePipe) != 0 && (hs_tune & kHsTuneSumSplit) == 0 && ((hs_tune >> 8) & 1u) == 0;
}

// The oct verifier over two waves per 8 signatures: wave 1 hashes and splits
// the scalars (q_prepare) while wave 0 decompresses A and R; the scalars
// reach wave 0 through LDS at one barrier, and wave 1 exits. For batches up
// to 4,096 signatures (1,024 waves), where SIMDs are idle anyway, this takes
// the hash and the half-scalar Euclid (~11% of a wave) off the chain.
template <uint32_t MODE>
__global__ __launch_bounds__(128, CMTV_QUAD_WAVES_PER_EU) void k_verify_oct_split(
    uint32_t n, const uint32_t* __restrict__ pk, const uint32_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    const uint32_t* __restrict__ off, const uint32_t* __restrict__ btab, uint8_t* __restrict__ out_valid,
    uint64_t* __restrict__ out_bitmap, uint32_t force_wide, SbFuse sb) {
  CMTV_URGENT();
  const uint32_t t = threadIdx.x & 63;
  const uint32_t gid = blockIdx.x * 64 + t;
  const uint32_t s = gid >> 3;
  const bool active = s < n;
  const uint32_t i = active ? s : n - 1;
  __shared__ uint32_t prep[8][SIG_PREP_WORDS + 1];
  __shared__ uint32_t bpt[8][40];
  __shared__ uint2 tab_lds[9 * 5 * 64];
  __shared__ uint32_t sbm[8][kSbFuseMaxMsg / 4];  // fused sign-bytes
  if (threadIdx.x >= 64) {
    // the oct's 8 helper lanes write the same bytes to the same slot, and
    // each hashes what it wrote
    const uint8_t* mp;
    uint32_t ml;
    helper_message(sb, i, msg, off, sbm[t >> 3], mp, ml);
    SigPrep p;
    q_prepare<MODE>(p, pk + 8 * (size_t)i, sig + 16 * (size_t)i, mp, ml, force_wide != 0);
    if ((t & 7) == 0) sig_prep_store(prep[t >> 3], p);
    __syncthreads();  // 1: the scalars
    ge_p3 B;
    q_bcomb16(B, p.u, DevBTab{btab});
    if ((t & 7) == 0) bpoint_store(bpt[t >> 3], B);
    __syncthreads();  // 2: [u]B
    return;
  }
  DevOct q;
  DevBTabQ bt{btab};
  DevATabQ ta{tab_lds, t};
  const uint32_t* bq = &bpt[t >> 3][10 * (t & 3)];
  bool v = o_verify_split<MODE, true>(
      q, pk + 8 * (size_t)i, sig + 16 * (size_t)i, bt, ta,
      [&](SigPrep& p) {
        __syncthreads();
        sig_prep_load(p, prep[t >> 3]);
      },
      [&](fe& c) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 10; j++) c.v[j] = bq[j];
      });
  v = v && active;
  if (active && (t & 7) == 0 && out_valid) out_valid[s] = v ? 1 : 0;
  uint64_t x = __ballot(v && (t & 7) == 0) & 0x0101010101010101ull;
  x = (x | (x >> 7)) & 0x0003000300030003ull;
  x = (x | (x >> 14)) & 0x0000000F0000000Full;
  x = (x | (x >> 28)) & 0xFFull;
  if (t == 0 && out_bitmap) reinterpret_cast<uint8_t*>(out_bitmap)[gid >> 6] = (uint8_t)x;
}

// [u]B for a helper wave whose 64 lanes all hold the same signature (the
// row forms with one signature per workgroup): the 16 comb rows (digit j of
// u is 16-bit chunk j of u + 0x8000...8000, verify_core.h BC16 blocks) are
// fetched at once -- lane L loads a quarter of row L / 4 into LDS -- and
// q_bcomb16 then reads them from LDS (one round trip to the 75 MB table
// instead of sixteen dependent ones).
struct LdsCombB {
  const uint32_t* rows;  // [16][BTAB_ROW_WORDS]
  __device__ __forceinline__ void load_fe(int e, int c, fe& r) const {
    const uint32_t* q = rows + ((e - BC16_BASE) >> 15) * BTAB_ROW_WORDS + c * BTAB_COORD_WORDS;
#pragma unroll
    for (int i = 0; i < 10; i++) r.v[i] = q[i];
  }
};
static_assert(BT16_ENTRIES == 1 << 15, "LdsCombB maps a comb row to its position by >> 15");

__device__ __forceinline__ void helper_bcomb_prefetched(ge_p3& B, const uint32_t u[8], const uint32_t* btab,
                                                        uint32_t* lds_rows, uint32_t* lds_pts, uint32_t t) {
  bcomb_rows_prefetch(lds_rows, u, btab, t);
  uint32_t tb[8];  // u's digits again, for the tree
  hs_recode65536(tb, u);
  auto digit = [&](uint32_t j) -> int {
    uint32_t w = tb[0];
#pragma unroll
    for (int i = 1; i < 8; i++) w = (j >> 1) == (uint32_t)i ? tb[i] : w;
    return (int)((w >> (16 * (j & 1))) & 0xFFFFu) - 0x8000;
  };
  // a tree instead of q_bcomb16's chain of 16: lane j (< 8) adds comb rows
  // 2j and 2j+1, then three levels of full additions through LDS (lanes
  // 0..3, 0..1, 0) -- 2 mixed + 3 full additions on the path instead of 16
  // mixed ones. The sum is the same point as q_bcomb16's in another
  // projective representation; the row kernels use it only as a point.
  const uint32_t l = t & 7;
  ge_p3 P;
  p3_identity(P);
  ge_efgh e;
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const uint32_t j = 2 * l + h;
    const int d = digit(j);
    const int ib = d < 0 ? -d : d;
    ge_add_table<false>(e, P, LdsCombB{lds_rows}, BC16_BASE + (int)j * BT16_ENTRIES, d < 0, ib == 0);
    efgh_to_p3(P, e);
  }
#pragma unroll 1
  for (uint32_t width = 4; width >= 1; width >>= 1) {
    if (t < 2 * width) p3_lds_store(lds_pts + t * 40, P);
    wave_sync();
    const uint32_t a = (2 * t) & 7, b = a + 1;  // lanes < width combine slots 2t, 2t+1
    ge_p3 Q, S;
    p3_lds_load(Q, lds_pts + a * 40);
    p3_lds_load(S, lds_pts + b * 40);
    wave_sync();
    ge_cached sc;
    p3_to_cached(sc, S);
    ge_add_cached(e, Q, sc);
    efgh_to_p3(P, e);
  }
  B = P;
}

// One signature per wave (row.h): for the smallest batches (a 150-validator
// commit), where SIMDs are idle and each signature's chain of field products
// is the kernel time. A 4-wave workgroup takes 3 signatures: waves 0-2
// decode A and R (rows 0/2 and 1/3) and build their tables while wave 3's
// lanes 0-2 hash and split the scalars (q_prepare, the templated sign-bytes
// included); the scalars reach them at barrier 1 and [u]B (q_bcomb16, as
// four canonical encodings) at barrier 2, after which wave 3 exits. LDS:
// 3 x 9 KiB tables, one workgroup per CU, i.e. one wave per SIMD.
// Verdicts: lane 0 of each wave writes its byte to out_valid and adds its
// field to the launch's ring slot (row_bitmap_add).
template <uint32_t MODE>
__global__ __launch_bounds__(256, 1) void k_verify_row_split(
    uint32_t n, const uint32_t* __restrict__ pk, const uint32_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    const uint32_t* __restrict__ off, const uint32_t* __restrict__ btab, uint8_t* __restrict__ out_valid,
    uint64_t* __restrict__ out_bitmap, uint32_t force_wide, SbFuse sb, RowSlot slot) {
  CMTV_URGENT();
  const uint32_t wave = threadIdx.x >> 6, t = threadIdx.x & 63;
  const uint32_t base = blockIdx.x * 3;
  __shared__ uint32_t prep[3][SIG_PREP_WORDS + 1];
  __shared__ uint32_t bpt[3][32];
  __shared__ uint32_t tab_lds[3][kRowTabWords];
  __shared__ uint32_t sbm[3][kSbFuseMaxMsg / 4];
  CMTV_STAMP(0);
  if (wave == 3) {
    const uint32_t ls = t < 3 ? t : 2;
    const uint32_t s = base + ls;
    const uint32_t i = s < n ? s : n - 1;
    const uint8_t* mp;
    uint32_t ml;
    helper_message(sb, i, msg, off, sbm[ls], mp, ml);
    SigPrep p;
    q_prepare<MODE>(p, pk + 8 * (size_t)i, sig + 16 * (size_t)i, mp, ml, force_wide != 0);
    if (t < 3) sig_prep_store(prep[t], p);
    CMTV_STAMP(1);
    __syncthreads();  // 1: the scalars
    CMTV_STAMP(2);
    ge_p3 B;
    q_bcomb16(B, p.u, DevBTab{btab});
    if (t < 3) bpoint_store_bytes(bpt[t], B);
    CMTV_STAMP(3);
    __syncthreads();  // 2: [u]B
    CMTV_STAMP(4);
    return;
  }
  const uint32_t s = base + wave;
  const bool active = s < n;
  const uint32_t i = active ? s : n - 1;
  const uint32_t* pkp = pk + 8 * (size_t)i;
  const uint32_t* sgp = sig + 16 * (size_t)i;
  uint32_t pkw[8], sigw[8];
  load_words(pkw, pkp, 2);
  load_words(sigw, sgp, 2);
  const uint32_t limb = reinterpret_cast<const uint16_t*>(((t >> 4) & 1) ? sgp : pkp)[t & 15];
  DevRowTab tab{tab_lds[wave], t};
  const uint32_t* bq = bpt[wave];
  bool v = r_verify_split<MODE>(
      DevRow(), limb, pkw, sigw, tab,
      [&](SigPrep& p) {
        CMTV_STAMP(1);
        __syncthreads();
        CMTV_STAMP(2);
        sig_prep_load(p, prep[wave]);
      },
      [&]() -> uint32_t {
        CMTV_STAMP(3);
        __syncthreads();
        CMTV_STAMP(4);
        return bpt_limb(bq, t);
      });
  CMTV_STAMP(5);
  v = v && active;
  if (t == 0 && active && out_valid) out_valid[s] = v ? 1 : 0;
  if (out_bitmap && active) row_bitmap_add(slot, s, n, v, out_bitmap, t);
}

// The row verifier over four waves per signature (row.h r_sum_ar / r_part<·,
// kRowLoWindows> / r_join4), one signature per workgroup and CU, for batches
// of at most 256: wave 0 (lo) decodes A and R and runs the lowest 21
// windows of both; waves 1 and 2 (A-hi, R-hi) each decode their point, scale
// it by 2^84 while the helper (wave 3) hashes, and run the windows above;
// the helper computes [u]B. Waves 1-2 hand their sums (cached) over at
// barrier 2; wave 0 adds them and [u]B and checks. The critical path is a
// high wave's decode + 4W doublings + its additions, instead of the two-wave
// form's decode + 4W doublings + W additions + the second table.
template <uint32_t MODE>
__global__ __launch_bounds__(256, 1) void k_verify_row4_split(
    uint32_t n, const uint32_t* __restrict__ pk, const uint32_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    const uint32_t* __restrict__ off, const uint32_t* __restrict__ btab, uint8_t* __restrict__ out_valid,
    uint64_t* __restrict__ out_bitmap, uint32_t force_wide, SbFuse sb, RowSlot slot) {
  CMTV_URGENT();
  const uint32_t wave = threadIdx.x >> 6, t = threadIdx.x & 63;
  const uint32_t s = blockIdx.x;
  const uint32_t i = s < n ? s : n - 1;
  __shared__ uint32_t prep[SIG_PREP_WORDS + 1];
  __shared__ uint32_t bpt[32];
  __shared__ uint32_t brows[16 * BTAB_ROW_WORDS];  // the helper's [u]B comb rows
  __shared__ uint32_t bpts[8 * 40];                // ... and its partial sums
  __shared__ uint32_t tab_lo[kRowTabWords];
  __shared__ uint32_t tab_hi[2][kRowTabWords / 2];
  __shared__ uint32_t sbm[kSbFuseMaxMsg / 4];
  __shared__ uint32_t xh[2][64];  // the high parts' sums (cached)
  const uint32_t* pkp = pk + 8 * (size_t)i;
  const uint32_t* sgp = sig + 16 * (size_t)i;
  CMTV_STAMP(0);
  CMTV_STAMP_RT(7);
  if (wave == 3) {
    const uint8_t* mp;
    uint32_t ml;
    helper_message(sb, i, msg, off, sbm, mp, ml);
    SigPrep p;
    q_prepare<MODE, true>(p, pkp, sgp, mp, ml, force_wide != 0);  // one signature on every lane
    if (t == 0) sig_prep_store(prep, p);
    CMTV_STAMP(1);
    __syncthreads();  // 1: the scalars
    CMTV_STAMP(2);
    ge_p3 B;
    helper_bcomb_prefetched(B, p.u, btab, brows, bpts, t);
    if (t == 0) bpoint_store_bytes(bpt, B);
    CMTV_STAMP(3);
    __syncthreads();  // 2: [u]B and the high parts
    CMTV_STAMP(4);
    return;
  }
  const RowCtx<DevRow> x(DevRow::lane());
  SigPrep p;
  auto stamp = [&](int k) { CMTV_STAMP(k); (void)k; };
  auto get_prep = [&](SigPrep& q) {
    CMTV_STAMP(1);
    __syncthreads();
    CMTV_STAMP(2);
    sig_prep_load(q, prep);
  };
  if (wave != 0) {
    const uint32_t* src = wave == 2 ? sgp : pkp;
    const uint32_t limb = reinterpret_cast<const uint16_t*>(src)[t & 15];
    const bool sign = (src[7] >> 31) != 0;
    DevRowTab tab{tab_hi[wave - 1], t};
    bool dec, x0;
    const uint32_t v = wave == 1 ? r_part<0, kRowLoWindows>(x, limb, sign, tab, get_prep, p, dec, x0, stamp)
                                 : r_part<1, kRowLoWindows>(x, limb, sign, tab, get_prep, p, dec, x0, stamp);
    xh[wave - 1][t] = rp_to_cached(x, v, x.cst(RowConst::d2));
    CMTV_STAMP(3);
    __syncthreads();  // 2
    CMTV_STAMP(4);
    return;
  }
  uint32_t pkw[8], sigw[8];
  load_words(pkw, pkp, 2);
  load_words(sigw, sgp, 2);
  const uint32_t limb = reinterpret_cast<const uint16_t*>(((t >> 4) & 1) ? sgp : pkp)[t & 15];
  DevRowTab tab{tab_lo, t};
  bool a_ok, r_ok, r_canon;
  const uint32_t v = r_sum_ar(x, limb, pkw, sigw, tab, get_prep, kRowLoWindows, p, a_ok, r_ok, r_canon);
  CMTV_STAMP(3);
  __syncthreads();  // 2
  CMTV_STAMP(4);
  const uint32_t cb = bpt_limb(bpt, t);
  bool v_ok = r_join4<MODE>(x, v, xh[0][t], xh[1][t], cb, (p.flags & 4u) != 0 && a_ok && r_ok, r_canon);
  CMTV_STAMP(5);
  CMTV_STAMP_RT(6);
  const bool active = s < n;
  v_ok = v_ok && active;
  if (t == 0 && active && out_valid) out_valid[s] = v_ok ? 1 : 0;
  if (out_bitmap && active) row_bitmap_add(slot, s, n, v_ok, out_bitmap, t);
}

hipError_t launch_verify(uint32_t mode, uint32_t n, const void* pk, const void* sig, const void* msg,
                         const void* off, const uint32_t* btab, uint32_t* atab, void* valid, void* bitmap,
                         uint32_t kflags, hipStream_t s, const SbFuse* sb, const RowSlot* row_slot, uint32_t ps_wait,
                         uint32_t* diag) {
  const SbFuse fz = sb ? *sb : SbFuse{};
  const uint32_t form = kflags & kFormMask;
  const uint32_t fw = (kflags & kLaunchForceWide) ? 1u : 0u;
  if (n == 0) return hipSuccess;
  auto pkp = static_cast<const uint32_t*>(pk);
  auto sgp = static_cast<const uint32_t*>(sig);
  auto mp = static_cast<const uint8_t*>(msg);
  auto op = static_cast<const uint32_t*>(off);
  auto vp = static_cast<uint8_t*>(valid);
  auto bp = static_cast<uint64_t*>(bitmap);
  const RowSlot rs = row_slot ? *row_slot : RowSlot{};
  if ((form == kFormRow4 || form == kFormRow) && (n > kRowMaxCap || (bp && !rs.words))) return hipErrorInvalidValue;
  if (form != kFormLane && form != kFormQuad && form != kFormOct2 && form != kFormRow && form != kFormRow4)
    return hipErrorInvalidValue;
  if (fz.tmpls && form == kFormLane) return hipErrorInvalidValue;
  with_mode(mode, [&](auto m) {
    constexpr uint32_t M = decltype(m)::value;
    switch (form) {
      case kFormRow4:  // one signature per 256-lane block (lo, A-hi, R-hi, the helper)
        hipLaunchKernelGGL(k_verify_row4_split<M>, dim3(n), dim3(256), 0, s, n, pkp, sgp, mp, op, btab, vp, bp, fw, fz,
                           rs);
        break;
      case kFormRow:  // 3 signatures per 256-lane block (3 row waves + the helper)
        hipLaunchKernelGGL(k_verify_row_split<M>, dim3((n + 2) / 3), dim3(256), 0, s, n, pkp, sgp, mp, op, btab, vp, bp,
                           fw, fz, rs);
        break;
      case kFormOct2:  // one 128-lane block (2 waves) = 8 signatures; whole groups of 8 blocks
        hipLaunchKernelGGL(k_verify_oct_split<M>, dim3(((n + 63) / 64) * 8), dim3(128), 0, s, n, pkp, sgp, mp, op, btab,
                           vp, bp, fw, fz);
        break;
      case kFormQuad: {
        // 48 signatures per 256-lane block; enough blocks for every 16-bit
        // slice of every bitmap word; of rs, its tagged entries only
        const uint32_t slices = 4 * ((n + 63) / 64);
        if ((kflags & kLaunchHsFold) && hs_fold_pipe(kflags >> 16))
          hipLaunchKernelGGL((k_verify_quad_hs_fold<M, true>), dim3((slices + 2) / 3), dim3(320), 0, s, n, pkp, sgp, mp,
                             op, btab, vp, bp, fw, fz, kflags >> 16, ps_wait, diag, rs);
        else if (kflags & kLaunchHsFold)
          hipLaunchKernelGGL((k_verify_quad_hs_fold<M, false>), dim3((slices + 2) / 3), dim3(320), 0, s, n, pkp, sgp, mp,
                             op, btab, vp, bp, fw, fz, kflags >> 16, ps_wait, diag, rs);
        else
          hipLaunchKernelGGL(k_verify_quad_hs<M>, dim3((slices + 2) / 3), dim3(256), 0, s, n, pkp, sgp, mp, op, btab,
                             vp, bp, fw, fz, kflags >> 16, rs);
        break;
      }
      default:
        hipLaunchKernelGGL(k_verify<M>, dim3((n + 63) / 64), dim3(64), 0, s, n, pkp, sgp, mp, op, btab, atab, vp, bp);
    }
  });
  return hipGetLastError();
}

}  // namespace cmtv
