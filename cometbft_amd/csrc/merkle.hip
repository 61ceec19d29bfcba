// merkle.hip -- k_merkle_pass: RFC 6962 merkle roots of many trees per launch
// (merkle.h; crypto/merkle/tree.go:9, types/validator_set.go:347 Hash,
// types/block.go:894 Commit.Hash). One lane hashes one leaf -- an item in
// global memory, a transaction (Txs.Hash(): hashed, then hashed as an item), a
// validator or a CommitSig encoded in registers from the
// struct-of-arrays fields, or a node of the previous pass -- and the
// workgroup reduces its aligned block of kMerkleB leaves to one node in LDS,
// one barrier per level, two word-planar level buffers (16 KiB).
//
// Workgroups never hand anything to each other inside a launch: no flags, no
// counters, no grid barrier. A tree of more than kMerkleB leaves takes
// another launch on the same stream over its block nodes, and the kernel
// boundary orders the two.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "merkle.h"

namespace cmtv {

struct ItemLeaf {
  MerkleLeaves a;
  __device__ __forceinline__ void operator()(uint32_t g, uint32_t h[8]) const {
    const uint32_t o = a.off[g];
    merkle_leaf_hash(h, a.var + o, a.off[g + 1] - o);
  }
};

struct TxLeaf {
  MerkleLeaves a;
  __device__ __forceinline__ void operator()(uint32_t g, uint32_t h[8]) const {
    const uint32_t o = a.off[g];
    merkle_tx_leaf_hash(h, a.var + o, a.off[g + 1] - o);
  }
};

struct ValidatorLeaf {
  MerkleLeaves a;
  __device__ __forceinline__ void operator()(uint32_t g, uint32_t h[8]) const {
    const uint32_t o = a.off[g], klen = a.off[g + 1] - o;
    uint32_t kw[16], w[32];
    load_be_words<16>(kw, a.var + o, klen);
    const uint32_t nb = merkle_validator_leaf(w, kw, klen, a.u8 ? a.u8[g] : kMerkleKeyEd25519, a.i64[g]);
    sha256_blocks(h, w, nb);
  }
};

struct CommitSigLeaf {
  MerkleLeaves a;
  __device__ __forceinline__ void operator()(uint32_t g, uint32_t h[8]) const {
    const uint32_t o = a.off[g], slen = a.off[g + 1] - o;
    uint32_t sw[16], addr[5], w[32];
    load_be_words<16>(sw, a.var + o, slen);
    // the address array starts 16-byte aligned: 20 g is a word boundary
    const uint32_t* ap = reinterpret_cast<const uint32_t*>(a.addr + 20 * (size_t)g);
#pragma unroll
    for (int k = 0; k < 5; k++) addr[k] = __builtin_bswap32(ap[k]);
    const uint32_t nb = merkle_commit_sig_leaf(w, a.u8[g], addr, a.i64[g], a.i32[g], sw, slen);
    sha256_blocks(h, w, nb);
  }
};

struct NodeLeaf {
  MerkleLeaves a;
  __device__ __forceinline__ void operator()(uint32_t g, uint32_t h[8]) const {
    const uint4* p = reinterpret_cast<const uint4*>(a.nodes + 8 * (size_t)g);
    const uint4 lo = p[0], hi = p[1];
    h[0] = lo.x; h[1] = lo.y; h[2] = lo.z; h[3] = lo.w;
    h[4] = hi.x; h[5] = hi.y; h[6] = hi.z; h[7] = hi.w;
  }
};

template <class Leaf>
__global__ __launch_bounds__(kMerkleB) void k_merkle_pass(Leaf leaf, const uint32_t* __restrict__ wg_off,
                                                          const uint32_t* __restrict__ leaf_off, uint32_t n_trees,
                                                          uint32_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint32_t lv[2][8 * kMerkleB];
  const uint32_t tid = threadIdx.x;
  const MerkleBlock b = merkle_block_of(blockIdx.x, wg_off, leaf_off, n_trees);
  uint32_t h[8];
  if (b.m == 0) {  // an empty tree (the whole workgroup: b is uniform)
    if (tid == 0) {
      merkle_empty(h);
#pragma unroll
      for (int k = 0; k < 8; k++) out[8 * (size_t)blockIdx.x + k] = h[k];
    }
    return;
  }
  if (tid < b.m) {
    leaf(b.first + tid, h);
#pragma unroll
    for (int k = 0; k < 8; k++) lv[0][k * kMerkleB + tid] = h[k];
  }
  __syncthreads();
  uint32_t cur = 0;
  for (uint32_t c = b.m; c > 1; c = (c + 1) >> 1) {
    merkle_level_lane(tid, c, lv[cur], lv[cur ^ 1]);
    __syncthreads();
    cur ^= 1;
  }
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 8; k++) out[8 * (size_t)blockIdx.x + k] = lv[cur][k * kMerkleB];
  }
}

hipError_t launch_merkle_pass(MerkleLeafKind kind, const MerkleLeaves& leaves, const uint32_t* wg_off,
                              const uint32_t* leaf_off, uint32_t n_trees, uint32_t n_wg, uint32_t* out,
                              hipStream_t s) {
  if (n_wg == 0) return hipSuccess;
  const dim3 grid(n_wg), block(kMerkleB);
  switch (kind) {
    case kMerkleItems:
      hipLaunchKernelGGL(k_merkle_pass<ItemLeaf>, grid, block, 0, s, ItemLeaf{leaves}, wg_off, leaf_off, n_trees, out);
      break;
    case kMerkleValidators:
      hipLaunchKernelGGL(k_merkle_pass<ValidatorLeaf>, grid, block, 0, s, ValidatorLeaf{leaves}, wg_off, leaf_off,
                         n_trees, out);
      break;
    case kMerkleCommitSigs:
      hipLaunchKernelGGL(k_merkle_pass<CommitSigLeaf>, grid, block, 0, s, CommitSigLeaf{leaves}, wg_off, leaf_off,
                         n_trees, out);
      break;
    case kMerkleTxs:
      hipLaunchKernelGGL(k_merkle_pass<TxLeaf>, grid, block, 0, s, TxLeaf{leaves}, wg_off, leaf_off, n_trees, out);
      break;
    case kMerkleNodes:
      hipLaunchKernelGGL(k_merkle_pass<NodeLeaf>, grid, block, 0, s, NodeLeaf{leaves}, wg_off, leaf_off, n_trees, out);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace cmtv
