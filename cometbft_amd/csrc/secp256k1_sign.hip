// secp256k1_sign.hip -- gfx950 kernels that make secp256k1 test data
// (secp256k1_sign.h), the counterpart of keygen.hip's Ed25519 pair:
//
//   k_secp_pubkey: one key per lane: [d]G by the comb over the fixed table the
//     verifier builds (secp256k1.hip k_secp_gtab_build), one inversion mod p,
//     the 33-byte compressed key and, when asked for, its 20-byte address
//     (SHA-256 then RIPEMD-160, one block each).
//   k_secp_sign: one signature per lane: SHA-256 of the lane's message, the
//     RFC 6979 nonce (22 compressions of HMAC-SHA-256), [k]G by the same comb,
//     one inversion mod p and one mod n.
//
// 64-lane workgroups, no LDS, no barrier, nothing handed between workgroups.
// Variable time: not for keys that matter.
//
// Memory layout: priv n_keys x 32 B big-endian (read bytewise), msg flat bytes
// + (n + 1) u32 offsets as the verifying kernels, out_pk n x 33 B (written
// bytewise: a 33-byte stride has no alignment), out_addr n x 20 B and out_sig
// n x 64 B as words.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "secp256k1_sign.h"

namespace cmtv {

__device__ __forceinline__ void load_privkey(scn& d, const uint8_t* priv) {
  uint32_t w[8];
  words_from_be32(w, priv);
  scn_from_words(d, w);
}

__global__ __launch_bounds__(64) void k_secp_pubkey(uint32_t n, const uint8_t* __restrict__ priv,
                                                    const uint32_t* __restrict__ gtab,
                                                    uint8_t* __restrict__ out_pk, uint32_t* __restrict__ out_addr) {
  const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
  if (gid >= n) return;
  scn d;
  load_privkey(d, priv + 32 * (size_t)gid);
  DevSecpGTab gt{gtab};
  uint32_t pkw[9], addr[5];
  secp_pubkey_one(pkw, addr, out_addr != nullptr, d, gt);
  uint8_t* pk = out_pk + 33 * (size_t)gid;
#pragma unroll
  for (int i = 0; i < 33; i++) pk[i] = (uint8_t)(pkw[i / 4] >> (24 - 8 * (i % 4)));
  if (out_addr) {
#pragma unroll
    for (int q = 0; q < 5; q++) out_addr[5 * (size_t)gid + q] = addr[q];
  }
}

__global__ __launch_bounds__(64) void k_secp_sign(uint32_t n, const uint8_t* __restrict__ priv,
                                                  const uint32_t* __restrict__ key_idx,
                                                  const uint8_t* __restrict__ msg, const uint32_t* __restrict__ off,
                                                  const uint32_t* __restrict__ gtab, uint32_t* __restrict__ out_sig) {
  const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
  if (gid >= n) return;
  const uint32_t kid = key_idx ? key_idx[gid] : gid;
  scn d;
  load_privkey(d, priv + 32 * (size_t)kid);
  DevSecpGTab gt{gtab};
  const uint32_t m0 = off[gid], m1 = off[gid + 1];
  uint32_t sg[16];
  (void)secp_sign_one(sg, d, msg + m0, m1 - m0, gt);
#pragma unroll
  for (int q = 0; q < 16; q++) out_sig[16 * (size_t)gid + q] = __builtin_bswap32(sg[q]);
}

hipError_t launch_secp_pubkey(uint32_t n, const void* priv, const uint32_t* gtab, void* out_pk, void* out_addr,
                              hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_secp_pubkey, dim3((n + 63) / 64), dim3(64), 0, s, n, static_cast<const uint8_t*>(priv), gtab,
                     static_cast<uint8_t*>(out_pk), static_cast<uint32_t*>(out_addr));
  return hipGetLastError();
}

hipError_t launch_secp_sign(uint32_t n, const void* priv, const void* key_idx, const void* msg, const void* off,
                            const uint32_t* gtab, void* out_sig, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_secp_sign, dim3((n + 63) / 64), dim3(64), 0, s, n, static_cast<const uint8_t*>(priv),
                     static_cast<const uint32_t*>(key_idx), static_cast<const uint8_t*>(msg),
                     static_cast<const uint32_t*>(off), gtab, static_cast<uint32_t*>(out_sig));
  return hipGetLastError();
}

}  // namespace cmtv
