// header.hip -- k_header_hash: Header.Hash() of many headers in one launch
// (header.h; types/block.go:440-475). A row of 16 lanes owns a header: lanes
// 0..13 build one leaf each in registers from the staged struct-of-arrays
// fields and hash it, then the row reduces 14 -> 7 -> 4 -> 2 -> 1 in place
// with DPP row moves, every lane of the wave running the same compressions
// (two for the leaf, two per level). No LDS, no barrier, nothing handed
// between workgroups, one launch; the row's first lane writes the root.
#include <hip/hip_runtime.h>

#include "header.h"
#include "kernels.h"

namespace cmtv {

constexpr uint32_t kHeaderThreads = kHeadersPerWg * kHeaderGroup;
static_assert(kHeaderThreads == 256 && kHeaderGroup == 16, "whole waves of four DPP rows");

// The group policy of header.h on the device: lane i reads lane i + S of its
// row (v_mov_b32_dpp row_shl:S, bound_ctrl: a lane with no such neighbour
// reads zero and does not use it)
struct DevGroup {
  template <int S>
  __device__ __forceinline__ void down(uint32_t out[8], const uint32_t in[8]) const {
#pragma unroll
    for (int k = 0; k < 8; k++) out[k] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)in[k], 0x100 + S, 0xF, 0xF, true);
  }
};

__global__ __launch_bounds__(kHeaderThreads) void k_header_hash(MerkleLeaves a, uint32_t n, uint32_t* __restrict__ out) {
  const uint32_t t = blockIdx.x * kHeaderThreads + threadIdx.x;
  const uint32_t h = t / kHeaderGroup, lane = t % kHeaderGroup;
  uint32_t w[32], d[8];
  uint32_t nb = 1;
  if (h < n && lane < kHeaderLeaves) {
    const HeaderFields F{a.var, a.off, reinterpret_cast<const uint64_t*>(a.i64),
                         reinterpret_cast<const uint32_t*>(a.i32), n};
    nb = header_leaf(w, F, h, lane);
  } else {  // an idle lane hashes along: its node is never a child that counts
#pragma unroll
    for (int k = 0; k < 32; k++) w[k] = 0u;
  }
  sha256_blocks(d, w, nb);
  header_reduce(DevGroup{}, lane, d);
  if (h < n && lane == 0) {
    uint4* o = reinterpret_cast<uint4*>(out + 8 * (size_t)h);
    o[0] = make_uint4(d[0], d[1], d[2], d[3]);
    o[1] = make_uint4(d[4], d[5], d[6], d[7]);
  }
}

hipError_t launch_header_hash(const MerkleLeaves& fields, uint32_t n, uint32_t* out, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const dim3 grid((n + kHeadersPerWg - 1) / kHeadersPerWg), block(kHeaderThreads);
  hipLaunchKernelGGL(k_header_hash, grid, block, 0, s, fields, n, out);
  return hipGetLastError();
}

}  // namespace cmtv
