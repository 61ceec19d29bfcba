// kernel_parts.h -- the pieces the kernel files (*.hip) share: the verdict
// epilogues of the lane, quad and row forms, the helper waves' message and
// comb-row fetches and a few index expressions, and for their launchers the
// mode dispatch. Included by the .hip files only. Every device function is
// __device__ __forceinline__: a kernel that uses one contains the code it
// would contain with the function written out.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kernels.h"
#include "signbytes.h"
#include "verify_core.h"

// The small-batch (latency) forms raise their waves' issue priority: beside a
// pipeline's bulk launch (k_verify_keyed_batch, k_sign_bytes at priority 0)
// a 150-validator commit's workgroup lands on a SIMD that already holds bulk
// waves, and the SIMD's oldest-first arbitration starves the younger wave
// (round 6, tools/lat_trace_report.py: its kernel ran 2-2.7 ms instead of
// 0.05 ms while the bulk launch still had milliseconds to go). Within one
// kernel every wave has the same priority, so alone it changes nothing.
#define CMTV_URGENT() __builtin_amdgcn_s_setprio(2)

namespace cmtv {

// The lanes of a wave see each other's LDS writes from before this point
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Byte writer (signbytes.h sb_write) into a helper lane's LDS slot
struct LdsBytes {
  uint8_t* p;
  __device__ __forceinline__ void put(uint32_t pos, uint8_t b) { p[pos] = b; }
  // a template byte run from HBM: aligned dword loads issued 8 at a time
  // (one memory round trip per 32 bytes instead of one per byte), bytes
  // placed into the LDS slot
  __device__ __forceinline__ void copy(uint32_t pos, const uint8_t* src, uint32_t len) {
    const uintptr_t a = (uintptr_t)src;
    const int sh = (int)(a & 3);
    const uint32_t* w = (const uint32_t*)(a - sh);
    const uint32_t nw = ((uint32_t)sh + len + 3) >> 2;  // words holding bytes of the run
#pragma unroll 1
    for (uint32_t j = 0; j < nw; j += 8) {
      uint32_t v[8];
#pragma unroll
      for (int k = 0; k < 8; k++) v[k] = j + k < nw ? w[j + k] : 0u;
#pragma unroll
      for (int k = 0; k < 8; k++) {
#pragma unroll
        for (int b = 0; b < 4; b++) {
          const int q = 4 * (int)(j + k) + b - sh;
          if (q >= 0 && q < (int)len) p[pos + q] = (uint8_t)(v[k] >> (8 * b));
        }
      }
    }
  }
};

// Message of signature i for a helper lane: the CanonicalVote written into
// this lane's LDS slot from the commit template (sb.tmpls set; the host
// checked every message fits kSbFuseMaxMsg bytes), else msg[off[i]..off[i+1]).
// A lane hashes only bytes it wrote itself (sha512_prefixed loads only words
// holding message bytes), so no barrier is needed.
__device__ __forceinline__ void helper_message(const SbFuse& sb, uint32_t i, const uint8_t* msg, const uint32_t* off,
                                               uint32_t* slot, const uint8_t*& mp, uint32_t& ml) {
  if (sb.tmpls) {
    LdsBytes out{reinterpret_cast<uint8_t*>(slot)};
    // tidx null: one template for the whole batch (a single commit)
    const SbTemplate tp = static_cast<const SbTemplate*>(sb.tmpls)[sb.tidx ? sb.tidx[i] : 0u];
    ml = sb_write(out, tp, sb.blob, sb.flag[i] != 0, sb.sec[i], sb.nanos[i]);
    mp = reinterpret_cast<const uint8_t*>(slot);
  } else {
    const uint32_t m0 = off[i];
    mp = msg + m0;
    ml = off[i + 1] - m0;
  }
}

// Verdict epilogue of the one-signature-per-lane kernels: lane gid's byte,
// and its wave's 64 verdicts as bitmap word gid / 64 (a wavefront ballot).
__device__ __forceinline__ void lane_verdict_store(uint32_t gid, bool active, bool v, uint8_t* __restrict__ out_valid,
                                                   uint64_t* __restrict__ out_bitmap) {
  v = v && active;
  if (active && out_valid) out_valid[gid] = v ? 1 : 0;
  const uint64_t mask = __ballot(v);
  if (threadIdx.x == 0 && out_bitmap) out_bitmap[gid >> 6] = mask;
}

// Verdict epilogue of the quad kernels (3 quad waves of 16 signatures per
// workgroup; lane t of `wave` holds signature s's verdict on its quad's four
// lanes): the signature's byte, and the wave's 16 verdicts -- every fourth
// ballot bit, compacted -- as 16-bit slice (3 * block + wave) of the bitmap.
// The grid is rounded up to whole workgroups, so slices past the bitmap's
// last word are dropped. tags.tagged set: a polled host call (kernels.h
// RowSlot), the slice goes there with the call's tag instead.
__device__ __forceinline__ void quad_verdict_store(bool v, bool active, uint32_t s, uint32_t n, uint32_t wave,
                                                   uint32_t t, uint8_t* __restrict__ out_valid,
                                                   uint64_t* __restrict__ out_bitmap, const RowSlot& tags) {
  v = v && active;
  if (active && (t & 3) == 0 && out_valid) out_valid[s] = v ? 1 : 0;
  uint64_t x = __ballot(v && (t & 3) == 0) & 0x1111111111111111ull;
  x = (x | (x >> 3)) & 0x0303030303030303ull;
  x = (x | (x >> 6)) & 0x000F000F000F000Full;
  x = (x | (x >> 12)) & 0x000000FF000000FFull;
  x = (x | (x >> 24)) & 0xFFFFull;
  const uint32_t slice = blockIdx.x * 3 + wave;
  if (t == 0 && slice < 4 * ((n + 63) / 64)) {
    if (tags.tagged)
      __hip_atomic_store(tags.tagged + slice, ((uint64_t)tags.seq << 32) | x, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
    else if (out_bitmap)
      reinterpret_cast<uint16_t*>(out_bitmap)[slice] = (uint16_t)x;
  }
}

// The row kernels' bitmap epilogue, on one slot of the per-device ring
// (kernels.h kRowSlots). Slot word j (64 bits) collects the verdicts of
// signatures 32j .. 32j+31 as 2-bit fields (01 rejected, 10 accepted), each
// added by its signature's wave with ONE agent-scope relaxed atomic; the wave
// whose add fills the word's last field packs the word into 32-bit half j of
// out_bitmap (and the unused upper half of the last 64-bit word) and zeroes
// the slot word for the slot's next launch. Every access to a slot word is an
// atomic on that word, so nothing else needs ordering and no fence is issued:
// the round-4 form (verdict bytes, a release fence and an acq_rel ticket per
// wave, the last wave packing) made every wave write back and invalidate its
// XCD's L2 (buffer_wbl2 sc1 / buffer_inv sc1), ~10 us of a 150-signature
// launch (tools/microbench/launch_lat.hip).
__device__ __forceinline__ void row_bitmap_add(const RowSlot& slot, uint32_t s, uint32_t n, bool v,
                                               uint64_t* __restrict__ out_bitmap, uint32_t t) {
  uint64_t* sw = reinterpret_cast<uint64_t*>(slot.words);
  const uint32_t j = s >> 5, f = s & 31;
  uint64_t x = 0;
  if (t == 0) {
    const uint64_t add = (uint64_t)(v ? 2u : 1u) << (2 * f);
    x = __hip_atomic_fetch_add(sw + j, add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + add;
  }
  x = __shfl(x, 0);
  const uint32_t nf = n - 32 * j < 32 ? n - 32 * j : 32u;  // fields of word j
  const uint64_t m = 0x5555555555555555ull >> (64 - 2 * nf);
  if (((x | (x >> 1)) & m) != m) return;  // a field of word j is still empty
  const uint64_t acc = __ballot(t < 32 && ((x >> (2 * (t & 31) + 1)) & 1) != 0);
  if (t == 0) {
    __hip_atomic_store(sw + j, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (slot.tagged) {  // kernels.h RowSlot
      __hip_atomic_store(slot.tagged + j, ((uint64_t)slot.seq << 32) | (uint32_t)acc, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
      return;
    }
    uint32_t* ob = reinterpret_cast<uint32_t*>(out_bitmap);
    ob[j] = (uint32_t)acc;
    if ((j & 1) == 0 && 32 * (j + 1) >= n) ob[j + 1] = 0u;
  }
}

// The 16 B-comb rows (verify_core.h BC16 blocks) of a scalar's radix-2^16
// digits into lds_rows[16][BTAB_ROW_WORDS] at once, for a wave whose 64 lanes
// hold the same scalar: lane L fetches a quarter of row L / 4 (one memory
// round trip instead of 16 dependent ones); row j is that of |digit j| (of 1
// for a zero digit). Ends with wave_sync: every lane may read every row.
__device__ __forceinline__ void bcomb_rows_prefetch(uint32_t* lds_rows, const uint32_t scalar[8],
                                                    const uint32_t* btab, uint32_t t) {
  uint32_t tb[8];
  hs_recode65536(tb, scalar);
  const uint32_t j = t >> 2, part = t & 3;
  uint32_t w = tb[0];  // word j / 2 of tb, by selects
#pragma unroll
  for (int q = 1; q < 8; q++) w = (j >> 1) == (uint32_t)q ? tb[q] : w;
  const int d = (int)((w >> (16 * (j & 1))) & 0xFFFFu) - 0x8000;
  const int ib = d < 0 ? -d : d;
  const uint32_t* src =
      btab + (size_t)(BC16_BASE + j * BT16_ENTRIES + (ib > 0 ? ib - 1 : 0)) * BTAB_ROW_WORDS + 9 * part;
  uint32_t v[9];
#pragma unroll
  for (int i = 0; i < 9; i++) v[i] = src[i];
#pragma unroll
  for (int i = 0; i < 9; i++) lds_rows[j * BTAB_ROW_WORDS + 9 * part + i] = v[i];
  wave_sync();
}

// An extended point as 40 words of LDS (X, Y, Z, T)
__device__ __forceinline__ void p3_lds_store(uint32_t* lds, const ge_p3& P) {
#pragma unroll
  for (int i = 0; i < 10; i++) {
    lds[i] = P.X.v[i];
    lds[10 + i] = P.Y.v[i];
    lds[20 + i] = P.Z.v[i];
    lds[30 + i] = P.T.v[i];
  }
}

__device__ __forceinline__ void p3_lds_load(ge_p3& P, const uint32_t* lds) {
#pragma unroll
  for (int i = 0; i < 10; i++) {
    P.X.v[i] = lds[i];
    P.Y.v[i] = lds[10 + i];
    P.Z.v[i] = lds[20 + i];
    P.T.v[i] = lds[30 + i];
  }
}

// Row lane t's 16-bit limb of [u]B as the helper left it (bpoint_store_bytes:
// four canonical encodings of 8 words, one per row of 16 lanes)
__device__ __forceinline__ uint32_t bpt_limb(const uint32_t* bpt, uint32_t t) {
  return (bpt[8 * (t >> 4) + ((t & 15) >> 1)] >> (16 * (t & 1))) & 0xFFFFu;
}

// Launchers: f(std::integral_constant<uint32_t, M>) for the verification mode
// M, so that a kernel template's launch is written once (k<decltype(m)::value>).
template <class F>
inline void with_mode(uint32_t mode, F&& f) {
  if (mode != MODE_ZIP215)
    f(std::integral_constant<uint32_t, MODE_GO_STDLIB>{});
  else
    f(std::integral_constant<uint32_t, MODE_ZIP215>{});
}

}  // namespace cmtv
