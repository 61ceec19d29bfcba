// sr25519_sign.hip -- gfx950 kernels that make sr25519 test data
// (sr25519_sign.h), the counterpart of keygen.hip's Ed25519 pair and of
// secp256k1_sign.hip:
//
//   k_pubkey_sr25519: one key per lane: SHA-512 of the mini secret, [key]B over
//     the shared fixed-base table, ristretto255 ENCODE (one field power) and,
//     when asked for, the address SHA-256(pk)[:20] (one compression).
//   k_sign_sr25519: one signature per lane: the same key expansion and public
//     key, the witness hash, [r]B and its ENCODE, the verifier's merlin
//     transcript (merlin.h) and s = k key + r.
//
// 64-lane workgroups. The transcript has cross-lane steps (the wave's longest
// message, a vote on the tail's second pass), so k_sign_sr25519's lanes past n
// take the last item's inputs and store nothing, as k_verify_sr25519's do.
// Each lane's current STROBE block (42 words) gathers in LDS lane-interleaved
// exactly as there. Variable time: not for keys that matter.
//
// Memory layout: mini n_keys x 32 B (4-byte aligned), msg flat bytes + (n + 1)
// u32 offsets as the verifying kernels, out_pk n x 32 B, out_addr n x 20 B
// and out_sig n x 64 B as words.
#include <hip/hip_runtime.h>

#include "devtables.h"
#include "kernels.h"
#include "sr25519_sign.h"

namespace cmtv {

// sr25519.hip's: the STROBE block buffer of one lane in LDS
struct LdsStrobeState {
  uint32_t* __restrict__ lds;
  uint32_t lane;
  __device__ __forceinline__ void store(int i, uint32_t x) { lds[i * 64 + lane] = x; }
  __device__ __forceinline__ uint32_t load(int i) const { return lds[i * 64 + lane]; }
};

__global__ __launch_bounds__(64) void k_pubkey_sr25519(uint32_t n, const uint32_t* __restrict__ mini,
                                                       const uint32_t* __restrict__ btab,
                                                       uint32_t* __restrict__ out_pk,
                                                       uint32_t* __restrict__ out_addr) {
  const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
  if (gid >= n) return;
  uint32_t mw[8], pkw[8];
  load_words(mw, mini + 8 * (size_t)gid, 2);
  DevBTab bt{btab};
  sr_pubkey_from_mini(pkw, mw, bt);
#pragma unroll
  for (int q = 0; q < 8; q++) out_pk[8 * (size_t)gid + q] = pkw[q];
  if (out_addr) {
    uint32_t addr[5];
    sr_address(addr, pkw);
#pragma unroll
    for (int q = 0; q < 5; q++) out_addr[5 * (size_t)gid + q] = addr[q];
  }
}

// (64, 2): two waves per SIMD to put one wave's comb-row loads (32 dependent
// additions, each behind a row from a 75 MB table) under the other's hashing.
// The listing: 256 VGPRs and 20 spilled (84 bytes of scratch a lane, around
// the transcript); unbounded it takes 256 + 18 AGPRs, no scratch, one wave.
__global__ __launch_bounds__(64, 2) void k_sign_sr25519(uint32_t n, const uint32_t* __restrict__ mini,
                                                        const uint32_t* __restrict__ key_idx,
                                                        const uint8_t* __restrict__ msg,
                                                        const uint32_t* __restrict__ off,
                                                        const uint32_t* __restrict__ btab,
                                                        const uint32_t* __restrict__ prog, int nops,
                                                        uint32_t* __restrict__ out_sig) {
  __shared__ uint32_t st_lds[STROBE_BLOCK_WORDS * 64];
  const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
  const bool active = gid < n;
  const uint32_t i = active ? gid : n - 1;
  const uint32_t kid = key_idx ? key_idx[i] : i;
  const uint32_t m0 = off[i], m1 = off[i + 1];
  uint32_t mw[8], sg[16];
  load_words(mw, mini + 8 * (size_t)kid, 2);
  DevBTab bt{btab};
  LdsStrobeState st{st_lds, threadIdx.x};
  sr_sign_one(sg, mw, msg + m0, m1 - m0, prog, nops, st, bt);
  if (!active) return;
#pragma unroll
  for (int q = 0; q < 16; q++) out_sig[16 * (size_t)gid + q] = sg[q];
}

hipError_t launch_pubkey_sr25519(uint32_t n, const void* mini, const uint32_t* btab, void* out_pk, void* out_addr,
                                 hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pubkey_sr25519, dim3((n + 63) / 64), dim3(64), 0, s, n, static_cast<const uint32_t*>(mini),
                     btab, static_cast<uint32_t*>(out_pk), static_cast<uint32_t*>(out_addr));
  return hipGetLastError();
}

hipError_t launch_sign_sr25519(uint32_t n, const void* mini, const void* key_idx, const void* msg, const void* off,
                               const uint32_t* btab, const uint32_t* prog, int nops, void* out_sig, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sign_sr25519, dim3((n + 63) / 64), dim3(64), 0, s, n, static_cast<const uint32_t*>(mini),
                     static_cast<const uint32_t*>(key_idx), static_cast<const uint8_t*>(msg),
                     static_cast<const uint32_t*>(off), btab, prog, nops, static_cast<uint32_t*>(out_sig));
  return hipGetLastError();
}

}  // namespace cmtv
