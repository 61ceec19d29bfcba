// keyed_forms.hip -- the registered-key Ed25519 kernels with helper waves
// (gfx950) and the registered-key launcher:
//
//   k_comb_build  : registered-key combs (keyed.h), one workgroup per key
//   k_verify_keyed_row_split / k_verify_keyed_quad_split<MODE>: one signature
//                   per workgroup / per quad of lanes against a registered key
//   launch_verify_keyed: these two, or keyed_lane.hip's one signature per lane
//
// Inputs as kernels.hip's, with key_idx (n x u32 into the key set) in place of
// pk; ktabs holds one comb (COMB_TABLE_WORDS, keyed.h) per registered key.
#include <hip/hip_runtime.h>

#include "devtables.h"
#include "kernel_parts.h"
#include "kernels.h"
#include "keyed.h"
#include "keyed_quad.h"
#include "phase_probe.h"
#include "signbytes.h"

CMTV_PHASE_BUFFER(_keyed)  // cmtv_debug_phase_times_keyed

namespace cmtv {

// the keyed row kernel's R wave meets barrier 1 86 squarings into the decode's
// run of 100 (~198 of its ~265 products, ~54k cycles with the split
// products: when the hash helper publishes k)
constexpr int kKeyedRowMidAt = 86;

// Registered keys, one signature per workgroup in the row layout (row.h
// r_decode_neg_r / r_kcomb / r_bcomb16 / r_keyed_join), for batches of at
// most 256 (the 150-validator VerifyCommit with the keyset cache): wave 3
// hashes k; wave 2 adds [s]B over the B table's 16-position radix-2^16 comb
// (s needs no hash), then positions 31..16 of [k](-A) over the key's
// radix-256 comb; wave 1 takes k at barrier 1 and adds positions 15..0;
// wave 0 decodes R, meeting barrier 1 inside its square-root chain (about
// when the hash is done, so it does not wait), and after barrier 2 adds both
// sums to -R and checks. Comb rows are
// converted to the row layout as they are read (DevRow::niels_limb).
// Bitmap as k_verify_row_split.
template <uint32_t MODE>
__global__ __launch_bounds__(256, 1) void k_verify_keyed_row_split(
    uint32_t n, uint32_t n_keys, const uint32_t* __restrict__ key_idx, const uint32_t* __restrict__ sig,
    const uint8_t* __restrict__ msg, const uint32_t* __restrict__ off, const uint32_t* __restrict__ keys_pk,
    const uint8_t* __restrict__ keys_ok, const uint32_t* __restrict__ ktabs, const uint32_t* __restrict__ btab,
    uint8_t* __restrict__ out_valid, uint64_t* __restrict__ out_bitmap, RowSlot slot, SbFuse sb) {
  CMTV_URGENT();
  const uint32_t wave = threadIdx.x >> 6, t = threadIdx.x & 63;
  const uint32_t s = blockIdx.x;
  const uint32_t i = s < n ? s : n - 1;
  __shared__ uint32_t tks[8];
  __shared__ uint32_t sbm[kSbFuseMaxMsg / 4];  // fused sign-bytes (every helper lane writes the same bytes)
  __shared__ uint32_t xa[64], xb[64];
  __shared__ uint32_t arows[COMB_WINDOWS * COMB_ROW_WORDS];  // the 32 key-comb rows of k's digits
  __shared__ uint32_t brows[16 * BTAB_ROW_WORDS];            // the 16 B-comb rows of s's digits
  uint32_t kid = key_idx ? key_idx[i] : i;  // null: signature i is by key i (one commit)
  const bool kin = kid < n_keys;
  kid = kin ? kid : 0;
  const uint32_t* sgp = sig + 16 * (size_t)i;
  CMTV_STAMP(0);
  if (wave == 3) {
    const uint8_t* mp;
    uint32_t ml;
    helper_message(sb, i, msg, off, sbm, mp, ml);
    uint32_t tk[8];
    q_keyed_challenge(tk, keys_pk + 8 * (size_t)kid, sgp, mp, ml);
    if (t == 0)
#pragma unroll
      for (int j = 0; j < 8; j++) tks[j] = tk[j];
    CMTV_STAMP(1);
    __syncthreads();  // 1: k
    CMTV_STAMP(2);
    __syncthreads();  // 2
    return;
  }
  const RowCtx<DevRow> x(DevRow::lane());
  const uint32_t d2 = x.cst(RowConst::d2);
  // k's key-comb rows of positions hi .. hi - 15 into LDS at once (lane L
  // fetches a quarter of row L / 4), then added onto v
  auto kcomb_half = [&](uint32_t& v, int hi) {
    uint32_t tk[8];
#pragma unroll
    for (int j = 0; j < 8; j++) tk[j] = tks[j];
    {
      const uint32_t j = (uint32_t)(hi - 15) + (t >> 2), part = t & 3;
      uint32_t w = tk[0];
#pragma unroll
      for (int q = 1; q < 8; q++) w = (j >> 2) == (uint32_t)q ? tk[q] : w;
      const int d = (int)((w >> (8 * (j & 3))) & 0xFFu) - 128;
      const int ia = d < 0 ? -d : d;
      const uint4* src = reinterpret_cast<const uint4*>(
          ktabs + (size_t)kid * COMB_TABLE_WORDS + ((size_t)j * COMB_ENTRIES + (ia > 0 ? ia - 1 : 0)) * COMB_ROW_WORDS +
          8 * part);
      const uint4 r0 = src[0], r1 = src[1];
      uint4* dst = reinterpret_cast<uint4*>(arows + j * COMB_ROW_WORDS + 8 * part);
      dst[0] = r0;
      dst[1] = r1;
      wave_sync();
    }
    r_kcomb(x, v, tk, [&](int j, int) { return arows + j * COMB_ROW_WORDS; }, hi, hi - 15);
  };
  if (wave == 2) {
    uint32_t sw[8];
    load_words(sw, sgp + 8, 2);
    bcomb_rows_prefetch(brows, sw, btab, t);  // the 16 comb rows of s's digits, one round trip
    uint32_t v = r_bcomb16(x, sw, [&](int e) { return brows + ((e - BC16_BASE) >> 15) * BTAB_ROW_WORDS; });
    CMTV_STAMP(1);
    __syncthreads();  // 1: k
    CMTV_STAMP(2);
    kcomb_half(v, 31);
    xb[t] = rp_to_cached(x, v, d2);
    CMTV_STAMP(3);
    __syncthreads();  // 2: [s]B + positions 31..16 of [k](-A)
    return;
  }
  if (wave == 1) {
    CMTV_STAMP(1);
    __syncthreads();  // 1: k
    CMTV_STAMP(2);
    uint32_t v = rp_identity(x);
    kcomb_half(v, 15);
    xa[t] = rp_to_cached(x, v, d2);
    CMTV_STAMP(3);
    __syncthreads();  // 2: positions 15..0 of [k](-A)
    return;
  }
  uint32_t sigw[8], sw[8];
  load_words(sigw, sgp, 2);
  load_words(sw, sgp + 8, 2);
  const uint32_t limb = reinterpret_cast<const uint16_t*>(sgp)[t & 15];
  bool r_ok;
  const uint32_t nr = r_decode_neg_r<MODE, kKeyedRowMidAt>(x, limb, sigw, r_ok, [&]() {
    CMTV_STAMP(1);
    __syncthreads();  // 1
    CMTV_STAMP(2);
  });
  CMTV_STAMP(3);
  __syncthreads();  // 2
  CMTV_STAMP(4);
  const bool s_ok = (sw[7] & 0xE0000000u) == 0 && sc_is_canonical(sw);
  const bool ok = kin && keys_ok[kid] != 0 && s_ok && r_ok;
  bool v_ok = r_keyed_join<MODE>(x, nr, xa[t], xb[t], ok);
  CMTV_STAMP(5);
  const bool active = s < n;
  v_ok = v_ok && active;
  if (t == 0 && active && out_valid) out_valid[s] = v_ok ? 1 : 0;
  if (out_bitmap && active) row_bitmap_add(slot, s, n, v_ok, out_bitmap, t);
}

// Comb of (negate ? -P : P) for n_keys encoded points; workgroup = key,
// thread = multiple d = 1..128. keys_ok[key] records whether P decoded.
__global__ __launch_bounds__(128) void k_comb_build(const uint32_t* __restrict__ keys_pk, uint8_t* __restrict__ keys_ok,
                                                    uint32_t* __restrict__ tabs, uint32_t* __restrict__ scratch,
                                                    int negate) {
  const uint32_t key = blockIdx.x;
  uint32_t w[8];
  load_words(w, keys_pk + 8 * (size_t)key, 2);
  ge_p3 A, nA;
  const bool ok = p3_frombytes(A, w);
  if (negate) {
    cached_neg_point(nA, A);
    A = nA;
  }
  if (threadIdx.x == 0 && keys_ok) keys_ok[key] = ok ? 1 : 0;
  DevCombScratch sc{scratch, gridDim.x * 128u, blockIdx.x * 128u + threadIdx.x};
  comb_build_column(tabs + (size_t)key * COMB_TABLE_WORDS, A, (int)threadIdx.x + 1, sc);
}

hipError_t launch_comb_build(uint32_t n_keys, const void* keys_pk, uint8_t* keys_ok, uint32_t* tabs,
                             uint32_t* scratch, bool negate, hipStream_t s) {
  if (n_keys == 0) return hipSuccess;
  hipLaunchKernelGGL(k_comb_build, dim3(n_keys), dim3(128), 0, s, static_cast<const uint32_t*>(keys_pk), keys_ok, tabs,
                     scratch, negate ? 1 : 0);
  return hipGetLastError();
}

// Registered-key quads with two helper waves: 3 quad waves (48 signatures)
// run the 32 fixed-base comb additions, take k from the hash helper (wave 4,
// q_keyed_challenge; published through an LDS flag, not a barrier), run the
// 32 key-comb additions and take R at the one barrier; the decode helper
// (wave 3, q_keyed_decode_r) starts R's square-root chain at the first cycle,
// one lane per signature. With one helper hashing and then decoding, the
// hash + decode chain (~225k cycles) set the kernel time; now the longer of
// the decode (~140k) and the quads' 64 additions does. 5 waves on 4 SIMDs:
// the short hash helper shares one.
//
// The quads wait for the hash helper's flag for at most k_wait polls. The
// verdict never depends on that wait: a quad wave that stops waiting hashes
// its own signatures (q_keyed_challenge, the same k the helper computes) and
// counts itself in diag[kDiagLateK] (cmtv_stats.late_k_waves). k_wait = 0
// (the CMTV_FORCE_K_LATE test knob) skips the flag entirely, so every quad
// wave takes that path.
template <uint32_t MODE>
__global__ __launch_bounds__(320, 1) void k_verify_keyed_quad_split(
    uint32_t n, uint32_t n_keys, const uint32_t* __restrict__ key_idx, const uint32_t* __restrict__ sig,
    const uint8_t* __restrict__ msg, const uint32_t* __restrict__ off, const uint32_t* __restrict__ keys_pk,
    const uint8_t* __restrict__ keys_ok, const uint32_t* __restrict__ ktabs, uint8_t* __restrict__ out_valid, uint64_t* __restrict__ out_bitmap, uint32_t k_wait, uint32_t* __restrict__ diag,
    const uint32_t* __restrict__ btab, SbFuse sb, RowSlot tags) {
  CMTV_URGENT();
  const uint32_t wave = threadIdx.x >> 6, t = threadIdx.x & 63;
  const uint32_t base = blockIdx.x * 48;
  __shared__ uint32_t tks[48][9];
  __shared__ uint32_t sbm[48][kSbFuseMaxMsg / 4];  // fused sign-bytes
  __shared__ uint32_t rpt[48][31];  // R: x, y, t (10 words each), decode flag
  __shared__ uint32_t k_ready;
  CMTV_STAMP5(0);
  CMTV_HWID5();
  if (threadIdx.x == 0) k_ready = 0u;
  __syncthreads();  // the flag is clear before any wave can set or read it
  // probe slots: 0 entry; hash helper 3 = k published; decode helper 3 = R
  // decoded; quads 4 = k taken, 1 / 2 = before / after the barrier (the combs
  // done / R in hand), 5 = exit; every wave 2 = after the barrier
  if (wave >= 3) {
    const uint32_t s = base + (t < 48 ? t : 47);
    const uint32_t i = s < n ? s : n - 1;
    if (wave == 4) {
      // hash helper: k for all 48 signatures, published through k_ready so
      // the decode helper never waits on it
      const uint8_t* mp;
      uint32_t ml;
      helper_message(sb, i, msg, off, sbm[t < 48 ? t : 47], mp, ml);
      uint32_t kid = key_idx ? key_idx[i] : i;
      kid = kid < n_keys ? kid : 0;
      uint32_t tk[8];
      q_keyed_challenge(tk, keys_pk + 8 * (size_t)kid, sig + 16 * (size_t)i, mp, ml);
      if (t < 48)
#pragma unroll
        for (int j = 0; j < 8; j++) tks[t][j] = tk[j];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      if (t == 0) __hip_atomic_store(&k_ready, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      CMTV_STAMP5(3);
    } else {
      // decode helper: R from the first cycle, overlapping the quads' fixed-
      // base and key combs (the chain that bounded the one-helper form)
      ge_p3 R;
      const bool r_ok = q_keyed_decode_r<MODE>(R, sig + 16 * (size_t)i);
      if (t < 48) {
#pragma unroll
        for (int j = 0; j < 10; j++) {
          rpt[t][j] = R.X.v[j];
          rpt[t][10 + j] = R.Y.v[j];
          rpt[t][20 + j] = R.T.v[j];
        }
        rpt[t][30] = r_ok ? 1u : 0u;
      }
      CMTV_STAMP5(3);
    }
    __syncthreads();  // R (and k)
    CMTV_STAMP5(2);
    return;
  }
  const uint32_t ls = wave * 16 + (t >> 2);
  const uint32_t s = base + ls;
  const bool active = s < n;
  const uint32_t i = active ? s : n - 1;
  uint32_t kid = key_idx ? key_idx[i] : i;  // null: signature i is by key i (one commit)
  const bool kin = kid < n_keys;
  kid = kin ? kid : 0;
  DevQuad q;
  const int lane = (int)(t & 3);
  // [s]B over the B table's radix-2^16 comb (16 additions)
  bool v = q_verify_keyed_split<MODE, true>(
      q, kin && keys_ok[kid] != 0, sig + 16 * (size_t)i, ktabs + (size_t)kid * COMB_TABLE_WORDS, nullptr,
      [&](uint32_t tk[8]) {
        // the hash helper's flag, polled at most k_wait times (a wave never
        // spins forever)
        bool ready = false;
        for (uint32_t spins = 0; spins < k_wait; spins++) {
          ready = __hip_atomic_load(&k_ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0u;
          if (ready) break;
          __builtin_amdgcn_s_sleep(2);
        }
        if (__builtin_expect(__ballot(ready) != __ballot(1), 0)) {
          // the helper's k did not arrive in time: hash this signature here
          // (identical k), so the wait bounds only the time, never the verdict;
          // fused sign-bytes are written again into the signature's slot (the
          // helper may be writing the same bytes there)
          const uint8_t* mp;
          uint32_t ml;
          helper_message(sb, i, msg, off, sbm[ls], mp, ml);
          q_keyed_challenge(tk, keys_pk + 8 * (size_t)kid, sig + 16 * (size_t)i, mp, ml);
          if (t == 0) atomicAdd(diag + kDiagLateK, 1u);
        } else {
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
          for (int j = 0; j < 8; j++) tk[j] = tks[ls][j];
        }
        CMTV_STAMP5(4);
      },
      [&](fe& rc, bool& r_ok) {
        CMTV_STAMP5(1);
        __syncthreads();
        CMTV_STAMP5(2);
        // this lane's coordinate: x, y, 1, t
        const uint32_t* p = rpt[ls] + 10 * (lane == 3 ? 2 : lane);
#pragma unroll
        for (int j = 0; j < 10; j++) rc.v[j] = lane == 2 ? (j == 0 ? 1u : 0u) : p[j];
        r_ok = rpt[ls][30] != 0;
      },
      DevBTabQ{btab});
  quad_verdict_store(v, active, s, n, wave, t, out_valid, out_bitmap, tags);
  CMTV_STAMP5(5);
}

hipError_t launch_verify_keyed(uint32_t mode, uint32_t n, uint32_t n_keys, const void* key_idx, const void* sig,
                               const void* msg, const void* off, const uint32_t* keys_pk, const uint8_t* keys_ok,
                               const uint32_t* ktabs, void* valid, void* bitmap, uint32_t form, uint32_t k_wait,
                               uint32_t* diag, uint32_t batch_kb, uint32_t* scr, const uint32_t* wtabs,
                               const uint32_t* btab, hipStream_t s, const RowSlot* row_slot, const SbFuse* sbp) {
  if (n == 0) return hipSuccess;
  const SbFuse sb = sbp ? *sbp : SbFuse{};
  // fused sign-bytes and identity keys only in the forms whose helper wave
  // hashes (row, quad)
  if ((sb.tmpls || !key_idx) && form == kKeyedLane) return hipErrorInvalidValue;
  if (form == kKeyedRow && (n > kRowMaxCap || (bitmap && !(row_slot && row_slot->words))))
    return hipErrorInvalidValue;
  auto ki = static_cast<const uint32_t*>(key_idx);
  auto sgp = static_cast<const uint32_t*>(sig);
  auto mp = static_cast<const uint8_t*>(msg);
  auto op = static_cast<const uint32_t*>(off);
  auto vp = static_cast<uint8_t*>(valid);
  auto bp = static_cast<uint64_t*>(bitmap);
  const RowSlot rs = row_slot ? *row_slot : RowSlot{};
  if (form == kKeyedRow) {
    // one signature per 256-lane block
    with_mode(mode, [&](auto m) {
      hipLaunchKernelGGL(k_verify_keyed_row_split<decltype(m)::value>, dim3(n), dim3(256), 0, s, n, n_keys, ki, sgp, mp,
                         op, keys_pk, keys_ok, ktabs, btab, vp, bp, rs, sb);
    });
    return hipGetLastError();
  }
  if (form == kKeyedQuad) {
    // of rs, only its tagged entries (16 signatures each) and seq
    const uint32_t slices = 4 * ((n + 63) / 64);
    with_mode(mode, [&](auto m) {
      hipLaunchKernelGGL(k_verify_keyed_quad_split<decltype(m)::value>, dim3((slices + 2) / 3), dim3(320), 0, s, n,
                         n_keys, ki, sgp, mp, op, keys_pk, keys_ok, ktabs, vp, bp, k_wait, diag, btab, sb, rs);
    });
    return hipGetLastError();
  }
  if (form != kKeyedLane) return hipErrorInvalidValue;
  return launch_verify_keyed_lane(mode, n, n_keys, ki, sgp, mp, op, keys_pk, keys_ok, ktabs, vp, bp, batch_kb, scr,
                                  wtabs, btab, s);
}

}  // namespace cmtv
