// keygen.hip -- gfx950 kernels that make data rather than check it, and
// their launchers:
//
//   k_btab_init       : builds the shared fixed-base table (affine niels rows;
//                       the layout is at kernels.hip's head)
//   k_pubkey / k_sign : RFC 8032 key generation and signing (synthetic data)
#include <hip/hip_runtime.h>

#include "devtables.h"
#include "kernels.h"
#include "verify_core.h"

namespace cmtv {

// rows 0..127: (1..128)B; 128..255: (1..128)[2^124]B; 256..383: (1..128)[2^128]B;
// then the radix-2^16 blocks (1..2^15)B, (1..2^15)[2^120]B, (1..2^15)[2^128]B
// and the 16-position comb (1..2^15)[2^16j]B (verify_core.h btab_row)
__global__ __launch_bounds__(64) void k_btab_init(uint32_t* __restrict__ rows) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= BTAB_TOTAL_ROWS) return;
  uint32_t row[BTAB_ROW_WORDS];
  btab_row(row, e);
#pragma unroll
  for (int i = 0; i < BTAB_ROW_WORDS; i++) rows[e * BTAB_ROW_WORDS + i] = row[i];
}

__global__ __launch_bounds__(64) void k_pubkey(uint32_t n, const uint32_t* __restrict__ seeds,
                                               const uint32_t* __restrict__ btab, uint32_t* __restrict__ out_pk) {
  const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
  if (gid >= n) return;
  uint32_t sw[8], pkw[8];
  load_words(sw, seeds + 8 * (size_t)gid, 2);
  DevBTab bt{btab};
  pubkey_from_seed(pkw, sw, bt);
#pragma unroll
  for (int q = 0; q < 8; q++) out_pk[8 * (size_t)gid + q] = pkw[q];
}

__global__ __launch_bounds__(64) void k_sign(uint32_t n, const uint32_t* __restrict__ seeds,
                                             const uint32_t* __restrict__ key_idx, const uint8_t* __restrict__ msg,
                                             const uint32_t* __restrict__ off, const uint32_t* __restrict__ btab,
                                             uint32_t* __restrict__ out_sig) {
  const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
  if (gid >= n) return;
  const uint32_t kid = key_idx ? key_idx[gid] : gid;
  uint32_t sw[8], sg[16];
  load_words(sw, seeds + 8 * (size_t)kid, 2);
  DevBTab bt{btab};
  const uint32_t m0 = off[gid], m1 = off[gid + 1];
  sign_one(sg, sw, msg + m0, m1 - m0, bt);
#pragma unroll
  for (int q = 0; q < 16; q++) out_sig[16 * (size_t)gid + q] = sg[q];
}

static inline unsigned blocks_for(uint32_t n) { return (n + 63) / 64; }

hipError_t launch_btab_init(uint32_t* d_rows, hipStream_t s) {
  hipLaunchKernelGGL(k_btab_init, dim3(blocks_for(BTAB_TOTAL_ROWS)), dim3(64), 0, s, d_rows);
  return hipGetLastError();
}

hipError_t launch_pubkey(uint32_t n, const void* seeds, const uint32_t* btab, void* out_pk, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pubkey, dim3(blocks_for(n)), dim3(64), 0, s, n, static_cast<const uint32_t*>(seeds), btab,
                     static_cast<uint32_t*>(out_pk));
  return hipGetLastError();
}

hipError_t launch_sign(uint32_t n, const void* seeds, const void* key_idx, const void* msg, const void* off,
                       const uint32_t* btab, void* out_sig, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sign, dim3(blocks_for(n)), dim3(64), 0, s, n, static_cast<const uint32_t*>(seeds),
                     static_cast<const uint32_t*>(key_idx), static_cast<const uint8_t*>(msg),
                     static_cast<const uint32_t*>(off), btab, static_cast<uint32_t*>(out_sig));
  return hipGetLastError();
}

}  // namespace cmtv
