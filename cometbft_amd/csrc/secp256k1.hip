// secp256k1.hip -- gfx950 kernels for secp256k1 ECDSA batch verification
// (reference path crypto/secp256k1/secp256k1.go:192-217).
//
//   k_verify_secp256k1: one signature per lane (secp256k1.h secp_verify_one):
//     key decompression, scalars mod n, SHA-256 of the lane's message,
//     [r/s]Q by signed 4-bit windows over a per-lane table and [e/s]G from
//     the fixed comb table, projective comparison; a wavefront ballot packs
//     64 verdicts into one bitmap word.
//   k_secp_gtab_build: the fixed table (1..128)[256^j]G, one row per thread;
//     the runtime runs it once per context, on the first secp256k1 batch.
//   k_secp_qcomb_build: the same table for each registered key Q,
//     (1..128)[256^j]Q, one thread per (key, j); run by
//     cmtv_register_keys_secp256k1.
//   k_verify_secp256k1_keyed: one signature per lane by registered key
//     (secp_verify_keyed_one): both scalar multiplications are combs, 33
//     additions from the fixed table and 33 from the key's; no scratch.
//   k_verify_secp256k1_tmpl, k_verify_secp256k1_keyed_tmpl: the same two with
//     each lane's message built by the lane itself: the CanonicalVote of its
//     commit signature written from the commit's template (kernels.h SbFuse,
//     signbytes.h sb_write) into the lane's own LDS slot of kSbFuseMaxMsg
//     bytes and hashed from there, so a commit ships no message buffer.
//   k_verify_secp256k1_keyed_batch<KB>: the keyed templated kernel with KB =
//     4 or 8 signatures per lane sharing one inversion mod n (Montgomery's
//     trick); the lane's running products go through the launch's scratch.
//     Launched for cross-height typed batches only (commits_typed.cpp).
//
// Memory layout: pk n x 33 B and sig n x 64 B (read bytewise: a 33-byte
// stride has no alignment), msg flat bytes + (n+1) u32 offsets as the other
// kernels. The per-lane table (1..8)Q lives in the launch's scratch,
// word-major / lane-minor (word w of entry e for lane l at
// (e * 30 + w) * stride + l), so a wave's access to one word is one 256-byte
// line whenever its lanes pick the same entry. The fixed table's rows are
// 32 words (16-byte aligned): a lane gathers its row with dwordx4 loads.
#include <hip/hip_runtime.h>

#include "kernel_parts.h"
#include "kernels.h"
#include "secp256k1.h"

namespace cmtv {

static_assert(kSecpQtabWordsPerLane == SECP_QTAB_ENTRIES * SECP_PT_WORDS, "scratch per lane");
static_assert(kSecpGtabWords == (uint32_t)SECP_GTAB_ENTRIES * SECP_GTAB_ROW_WORDS, "fixed table size");

struct DevSecpQTab {
  uint32_t* __restrict__ base;
  uint32_t stride;
  uint32_t lane;
  __device__ __forceinline__ void store(int e, const pt256& p) {
    uint32_t* q = base + (size_t)(e * SECP_PT_WORDS) * stride + lane;
#pragma unroll
    for (int i = 0; i < 10; i++) {
      q[(size_t)i * stride] = p.X.v[i];
      q[(size_t)(10 + i) * stride] = p.Y.v[i];
      q[(size_t)(20 + i) * stride] = p.Z.v[i];
    }
  }
  __device__ __forceinline__ void load(int e, pt256& p) const {
    const uint32_t* q = base + (size_t)(e * SECP_PT_WORDS) * stride + lane;
#pragma unroll
    for (int i = 0; i < 10; i++) {
      p.X.v[i] = q[(size_t)i * stride];
      p.Y.v[i] = q[(size_t)(10 + i) * stride];
      p.Z.v[i] = q[(size_t)(20 + i) * stride];
    }
  }
};

__global__ __launch_bounds__(64) void k_secp_gtab_build(uint32_t* __restrict__ rows) {
  const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
  if (gid >= (uint32_t)SECP_GTAB_ENTRIES) return;
  uint32_t row[SECP_GTAB_ROW_WORDS];
  secp_gtab_row(row, (int)(gid / SECP_GTAB_PER_POS), (int)(gid % SECP_GTAB_PER_POS) + 1);
  uint4* out = reinterpret_cast<uint4*>(rows + (size_t)gid * SECP_GTAB_ROW_WORDS);
#pragma unroll
  for (int k = 0; k < 8; k++) out[k] = make_uint4(row[4 * k], row[4 * k + 1], row[4 * k + 2], row[4 * k + 3]);
}

__global__ __launch_bounds__(64, 2) void k_verify_secp256k1(uint32_t n, const uint8_t* __restrict__ pk,
                                                            const uint8_t* __restrict__ sig,
                                                            const uint8_t* __restrict__ msg,
                                                            const uint32_t* __restrict__ off,
                                                            const uint32_t* __restrict__ gtab,
                                                            uint32_t* __restrict__ qtab,
                                                            uint8_t* __restrict__ out_valid,
                                                            uint64_t* __restrict__ out_bitmap) {
  const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
  const bool active = gid < n;
  const uint32_t i = active ? gid : n - 1;
  const uint32_t m0 = off[i], m1 = off[i + 1];
  DevSecpQTab qt{qtab, gridDim.x * 64u, gid};
  DevSecpGTab gt{gtab};
  bool v = secp_verify_one(pk + 33 * (size_t)i, sig + 64 * (size_t)i, msg + m0, m1 - m0, qt, gt);
  lane_verdict_store(gid, active, v, out_valid, out_bitmap);
}

// One thread per (key, position): position-major, so that a wave's lanes
// (nearly always) share j and with it the doubling loop's trip count. The
// thread's 128 rows go straight to the table (16 KiB per thread, written once).
__global__ __launch_bounds__(64) void k_secp_qcomb_build(uint32_t n_keys, const uint8_t* __restrict__ pk,
                                                         uint8_t* __restrict__ ok, uint32_t* __restrict__ tab) {
  const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
  if (gid >= n_keys * (uint32_t)SECP_GTAB_POS) return;
  const uint32_t j = gid / n_keys, key = gid % n_keys;
  uint32_t* rows = tab + (size_t)key * kSecpGtabWords + (size_t)j * (SECP_GTAB_PER_POS * SECP_GTAB_ROW_WORDS);
  const bool v = secp_qcomb_position(rows, pk + 33 * (size_t)key, (int)j);
  if (j == 0) ok[key] = v ? 1 : 0;
}

// One signature per lane by registered key key_idx[i]: no key bytes, no
// scratch. An index >= n_keys reads key 0's table and clears the verdict.
__global__ __launch_bounds__(64) void k_verify_secp256k1_keyed(uint32_t n, uint32_t n_keys,
                                                               const uint32_t* __restrict__ key_idx,
                                                               const uint8_t* __restrict__ key_ok,
                                                               const uint32_t* __restrict__ qtab,
                                                               const uint8_t* __restrict__ sig,
                                                               const uint8_t* __restrict__ msg,
                                                               const uint32_t* __restrict__ off,
                                                               const uint32_t* __restrict__ gtab,
                                                               uint8_t* __restrict__ out_valid,
                                                               uint64_t* __restrict__ out_bitmap) {
  const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
  const bool active = gid < n;
  const uint32_t i = active ? gid : n - 1;
  const uint32_t m0 = off[i], m1 = off[i + 1];
  const uint32_t k = key_idx[i];
  const bool in_set = k < n_keys;
  const uint32_t key = in_set ? k : 0;
  DevSecpGTab qt{qtab + (size_t)key * kSecpGtabWords};
  DevSecpGTab gt{gtab};
  bool v = secp_verify_keyed_one(in_set && key_ok[key] != 0, sig + 64 * (size_t)i, msg + m0, m1 - m0, qt, gt);
  lane_verdict_store(gid, active, v, out_valid, out_bitmap);
}

// The templated kernels' per-lane inputs, after helper_message's precedent
// (kernel_parts.h): signature i's template (tidx null: template 0), flag and
// timestamp, and a byte writer over this lane's LDS slot. A lane hashes only
// bytes it wrote itself, so no barrier is needed; a lane past n rebuilds
// signature n - 1's message in its own slot.
struct SecpLaneMsg {
  SbTemplate tp;
  bool flag;
  int64_t sec;
  int32_t nanos;
  __device__ __forceinline__ SecpLaneMsg(const SbFuse& sb, uint32_t i)
      : tp(static_cast<const SbTemplate*>(sb.tmpls)[sb.tidx ? sb.tidx[i] : 0u]),
        flag(sb.flag[i] != 0),
        sec(sb.sec[i]),
        nanos(sb.nanos[i]) {}
};

// k_verify_secp256k1 with templated sign-bytes (sb.tmpls set)
__global__ __launch_bounds__(64, 2) void k_verify_secp256k1_tmpl(uint32_t n, const uint8_t* __restrict__ pk,
                                                                 const uint8_t* __restrict__ sig, SbFuse sb,
                                                                 const uint32_t* __restrict__ gtab,
                                                                 uint32_t* __restrict__ qtab,
                                                                 uint8_t* __restrict__ out_valid,
                                                                 uint64_t* __restrict__ out_bitmap) {
  __shared__ uint32_t slots[64][kSbFuseMaxMsg / 4];
  const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
  const bool active = gid < n;
  const uint32_t i = active ? gid : n - 1;
  const SecpLaneMsg m(sb, i);
  uint8_t* slot = reinterpret_cast<uint8_t*>(slots[threadIdx.x]);
  LdsBytes out{slot};
  DevSecpQTab qt{qtab, gridDim.x * 64u, gid};
  DevSecpGTab gt{gtab};
  bool v = secp_verify_tmpl_one(pk + 33 * (size_t)i, sig + 64 * (size_t)i, out, slot, m.tp, sb.blob, m.flag, m.sec,
                                m.nanos, qt, gt);
  lane_verdict_store(gid, active, v, out_valid, out_bitmap);
}

// k_verify_secp256k1_keyed with templated sign-bytes
__global__ __launch_bounds__(64) void k_verify_secp256k1_keyed_tmpl(uint32_t n, uint32_t n_keys,
                                                                    const uint32_t* __restrict__ key_idx,
                                                                    const uint8_t* __restrict__ key_ok,
                                                                    const uint32_t* __restrict__ qtab,
                                                                    const uint8_t* __restrict__ sig, SbFuse sb,
                                                                    const uint32_t* __restrict__ gtab,
                                                                    uint8_t* __restrict__ out_valid,
                                                                    uint64_t* __restrict__ out_bitmap) {
  __shared__ uint32_t slots[64][kSbFuseMaxMsg / 4];
  const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
  const bool active = gid < n;
  const uint32_t i = active ? gid : n - 1;
  const SecpLaneMsg m(sb, i);
  uint8_t* slot = reinterpret_cast<uint8_t*>(slots[threadIdx.x]);
  LdsBytes out{slot};
  const uint32_t k = key_idx[i];
  const bool in_set = k < n_keys;
  const uint32_t key = in_set ? k : 0;
  DevSecpGTab qt{qtab + (size_t)key * kSecpGtabWords};
  DevSecpGTab gt{gtab};
  bool v = secp_verify_keyed_tmpl_one(in_set && key_ok[key] != 0, sig + 64 * (size_t)i, out, slot, m.tp, sb.blob,
                                      m.flag, m.sec, m.nanos, qt, gt);
  lane_verdict_store(gid, active, v, out_valid, out_bitmap);
}

// The batch kernel's running products in the launch's scratch, word-major /
// lane-minor like the per-lane table above: word w of round r for lane l at
// (r * 8 + w) * lanes + l, a wave's access to one word is one 256-byte line.
struct DevSecpPre {
  uint32_t* __restrict__ base;
  uint32_t lanes;
  uint32_t lane;
  __device__ __forceinline__ void store(int r, const scn& x) {
    uint32_t* q = base + (size_t)(r * 8) * lanes + lane;
#pragma unroll
    for (int i = 0; i < 8; i++) q[(size_t)i * lanes] = x.v[i];
  }
  __device__ __forceinline__ void load(int r, scn& x) const {
    const uint32_t* q = base + (size_t)(r * 8) * lanes + lane;
#pragma unroll
    for (int i = 0; i < 8; i++) x.v[i] = q[(size_t)i * lanes];
  }
};

// A lane's rounds of k_verify_secp256k1_keyed_batch (secp256k1.h
// secp_verify_keyed_batch_lane Src): round r is signature gid + r * lanes; a
// round past n takes signature n - 1 and writes nothing.
struct DevSecpBatchSrc {
  using QTab = DevSecpGTab;
  uint32_t n, n_keys, lanes, gid;
  const uint32_t* __restrict__ key_idx;
  const uint8_t* __restrict__ key_ok;
  const uint32_t* __restrict__ qtab;
  const uint8_t* __restrict__ sigs;
  const SbFuse& sb;
  uint8_t* slot;
  uint8_t* __restrict__ out_valid;
  uint64_t* __restrict__ out_bitmap;
  __device__ __forceinline__ uint32_t at(int r) const { return gid + (uint32_t)r * lanes; }
  __device__ __forceinline__ bool active(int r) const { return at(r) < n; }
  __device__ __forceinline__ uint32_t index(int r) const { return active(r) ? at(r) : n - 1; }
  __device__ __forceinline__ const uint8_t* sig(int r) const { return sigs + 64 * (size_t)index(r); }
  __device__ __forceinline__ bool key(int r, QTab& qt) const {
    const uint32_t k = key_idx[index(r)];
    const bool in_set = k < n_keys;
    const uint32_t key = in_set ? k : 0;
    qt.rows = qtab + (size_t)key * kSecpGtabWords;
    return in_set && key_ok[key] != 0;
  }
  __device__ __forceinline__ uint32_t message(int r, const uint8_t*& msg) const {
    const SecpLaneMsg m(sb, index(r));
    LdsBytes out{slot};
    msg = slot;
    return sb_write(out, m.tp, sb.blob, m.flag, m.sec, m.nanos);
  }
  __device__ __forceinline__ void verdict(int r, bool v) const {
    // a wave whose 64 signatures of this round are all past n has no bitmap word
    if (at(r) - threadIdx.x < n) lane_verdict_store(at(r), active(r), v, out_valid, out_bitmap);
  }
};

// k_verify_secp256k1_keyed_tmpl with KB signatures per lane sharing one
// inversion mod n (secp256k1.h secp_verify_keyed_batch_lane): signature
// s = gid + r * lanes in round r, so every round of a wave covers 64
// consecutive signatures and one bitmap word; ceil(n / (64 KB)) workgroups.
// pre: lanes x KB x 8 words of scratch. Verdicts equal the per-lane kernel's.
template <int KB>
__global__ __launch_bounds__(64) void k_verify_secp256k1_keyed_batch(uint32_t n, uint32_t n_keys,
                                                                     const uint32_t* __restrict__ key_idx,
                                                                     const uint8_t* __restrict__ key_ok,
                                                                     const uint32_t* __restrict__ qtab,
                                                                     const uint8_t* __restrict__ sig, SbFuse sb,
                                                                     const uint32_t* __restrict__ gtab,
                                                                     uint32_t* __restrict__ pre,
                                                                     uint8_t* __restrict__ out_valid,
                                                                     uint64_t* __restrict__ out_bitmap) {
  __shared__ uint32_t slots[64][kSbFuseMaxMsg / 4];
  const uint32_t lanes = gridDim.x * 64u, gid = blockIdx.x * 64u + threadIdx.x;
  DevSecpBatchSrc src{n,  n_keys, lanes, gid, key_idx, key_ok, qtab, sig, sb, reinterpret_cast<uint8_t*>(slots[threadIdx.x]),
                      out_valid, out_bitmap};
  DevSecpPre pr{pre, lanes, gid};
  DevSecpGTab gt{gtab};
  secp_verify_keyed_batch_lane<KB>(src, pr, gt);
}

hipError_t launch_verify_secp256k1_keyed_batch(uint32_t kb, uint32_t n, uint32_t n_keys, const uint32_t* key_idx,
                                               const uint8_t* key_ok, const uint32_t* qtab, const void* sig,
                                               const SbFuse& sb, const uint32_t* gtab, uint32_t* pre, void* valid,
                                               void* bitmap, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (!sb.tmpls || !pre || (kb != 4 && kb != 8)) return hipErrorInvalidValue;
  const dim3 grid((n + 64 * kb - 1) / (64 * kb)), block(64);
  if (kb == 8)
    hipLaunchKernelGGL(k_verify_secp256k1_keyed_batch<8>, grid, block, 0, s, n, n_keys, key_idx, key_ok, qtab,
                       static_cast<const uint8_t*>(sig), sb, gtab, pre, static_cast<uint8_t*>(valid),
                       static_cast<uint64_t*>(bitmap));
  else
    hipLaunchKernelGGL(k_verify_secp256k1_keyed_batch<4>, grid, block, 0, s, n, n_keys, key_idx, key_ok, qtab,
                       static_cast<const uint8_t*>(sig), sb, gtab, pre, static_cast<uint8_t*>(valid),
                       static_cast<uint64_t*>(bitmap));
  return hipGetLastError();
}

hipError_t launch_verify_secp256k1_tmpl(uint32_t n, const void* pk, const void* sig, const SbFuse& sb,
                                        const uint32_t* gtab, uint32_t* qtab, void* valid, void* bitmap,
                                        hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (!sb.tmpls) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_verify_secp256k1_tmpl, dim3((n + 63) / 64), dim3(64), 0, s, n,
                     static_cast<const uint8_t*>(pk), static_cast<const uint8_t*>(sig), sb, gtab, qtab,
                     static_cast<uint8_t*>(valid), static_cast<uint64_t*>(bitmap));
  return hipGetLastError();
}

hipError_t launch_verify_secp256k1_keyed_tmpl(uint32_t n, uint32_t n_keys, const uint32_t* key_idx,
                                              const uint8_t* key_ok, const uint32_t* qtab, const void* sig,
                                              const SbFuse& sb, const uint32_t* gtab, void* valid, void* bitmap,
                                              hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (!sb.tmpls) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_verify_secp256k1_keyed_tmpl, dim3((n + 63) / 64), dim3(64), 0, s, n, n_keys, key_idx, key_ok,
                     qtab, static_cast<const uint8_t*>(sig), sb, gtab, static_cast<uint8_t*>(valid),
                     static_cast<uint64_t*>(bitmap));
  return hipGetLastError();
}

hipError_t launch_secp_qcomb_build(uint32_t n_keys, const uint8_t* d_pk, uint8_t* d_ok, uint32_t* d_tab,
                                   hipStream_t s) {
  if (n_keys == 0) return hipSuccess;
  const uint32_t threads = n_keys * (uint32_t)SECP_GTAB_POS;
  hipLaunchKernelGGL(k_secp_qcomb_build, dim3((threads + 63) / 64), dim3(64), 0, s, n_keys, d_pk, d_ok, d_tab);
  return hipGetLastError();
}

hipError_t launch_verify_secp256k1_keyed(uint32_t n, uint32_t n_keys, const uint32_t* key_idx, const uint8_t* key_ok,
                                         const uint32_t* qtab, const void* sig, const void* msg, const void* off,
                                         const uint32_t* gtab, void* valid, void* bitmap, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_verify_secp256k1_keyed, dim3((n + 63) / 64), dim3(64), 0, s, n, n_keys, key_idx, key_ok, qtab,
                     static_cast<const uint8_t*>(sig), static_cast<const uint8_t*>(msg),
                     static_cast<const uint32_t*>(off), gtab, static_cast<uint8_t*>(valid),
                     static_cast<uint64_t*>(bitmap));
  return hipGetLastError();
}

hipError_t launch_secp_gtab_build(uint32_t* d_rows, hipStream_t s) {
  hipLaunchKernelGGL(k_secp_gtab_build, dim3((SECP_GTAB_ENTRIES + 63) / 64), dim3(64), 0, s, d_rows);
  return hipGetLastError();
}

hipError_t launch_verify_secp256k1(uint32_t n, const void* pk, const void* sig, const void* msg, const void* off,
                                   const uint32_t* gtab, uint32_t* qtab, void* valid, void* bitmap, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_verify_secp256k1, dim3((n + 63) / 64), dim3(64), 0, s, n, static_cast<const uint8_t*>(pk),
                     static_cast<const uint8_t*>(sig), static_cast<const uint8_t*>(msg),
                     static_cast<const uint32_t*>(off), gtab, qtab, static_cast<uint8_t*>(valid),
                     static_cast<uint64_t*>(bitmap));
  return hipGetLastError();
}

}  // namespace cmtv
