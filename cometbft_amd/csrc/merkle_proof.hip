// merkle_proof.hip -- merkle inclusion proofs (merkle_proof.h;
// crypto/merkle/proof.go ProofsFromByteSlices, Proof.Verify).
//
// k_merkle_proof_pass is k_merkle_pass's reduction with the nodes kept: every
// node of every tree is still hashed once. The first pass also writes every
// leaf hash. Before a level of the block is reduced, lane t (it owns leaf
// first + t) copies its sibling node of that level, when there is one, from
// the level buffer in LDS to the next free slot of its own proof: two 16-byte
// stores at aunt_off[first + t] + (aunts so far), 32-byte aligned. A tree of
// more than kMerkleB leaves takes further passes over its block nodes; the
// aunts a block node collects there are written once per node to a side
// buffer, and k_merkle_proof_spread appends them to the proof of every leaf
// below it.
//
// Workgroups hand nothing to each other inside a launch: the kernel boundary
// orders the passes and the spreading.
//
// k_merkle_proofs_verify: one lane per proof (merkle_proof_verify_lane).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "merkle_proof.h"

namespace cmtv {

namespace {

struct ProofItemLeaf {
  MerkleLeaves a;
  __device__ __forceinline__ void operator()(uint32_t g, uint32_t h[8]) const {
    const uint32_t o = a.off[g];
    merkle_leaf_hash(h, a.var + o, a.off[g + 1] - o);
  }
};

struct ProofTxLeaf {
  MerkleLeaves a;
  __device__ __forceinline__ void operator()(uint32_t g, uint32_t h[8]) const {
    const uint32_t o = a.off[g];
    merkle_tx_leaf_hash(h, a.var + o, a.off[g + 1] - o);
  }
};

struct ProofNodeLeaf {
  MerkleLeaves a;
  __device__ __forceinline__ void operator()(uint32_t g, uint32_t h[8]) const {
    merkle_load_node(h, a.nodes + 8 * (size_t)g);
  }
};

}  // namespace

// leaf_hashes: the first pass's, 8 words a leaf, or null. aunt_off: per leaf
// of this pass, in nodes of `aunts`.
template <class Leaf>
__global__ __launch_bounds__(kMerkleB) void k_merkle_proof_pass(Leaf leaf, const uint32_t* __restrict__ wg_off,
                                                                const uint32_t* __restrict__ leaf_off,
                                                                uint32_t n_trees, uint32_t* __restrict__ out,
                                                                uint32_t* __restrict__ leaf_hashes,
                                                                const uint32_t* __restrict__ aunt_off,
                                                                uint32_t* __restrict__ aunts) {
  __shared__ __attribute__((aligned(16))) uint32_t lv[2][8 * kMerkleB];
  const uint32_t tid = threadIdx.x;
  const MerkleBlock b = merkle_block_of(blockIdx.x, wg_off, leaf_off, n_trees);
  uint32_t h[8];
  if (b.m == 0) {  // an empty tree (the whole workgroup: b is uniform): the constant, no proof
    if (tid == 0) {
      merkle_empty(h);
      merkle_store_node(out + 8 * (size_t)blockIdx.x, h);
    }
    return;
  }
  const bool mine = tid < b.m;
  uint32_t* dst = nullptr;
  if (mine) {
    leaf(b.first + tid, h);
#pragma unroll
    for (int k = 0; k < 8; k++) lv[0][k * kMerkleB + tid] = h[k];
    if (leaf_hashes) merkle_store_node(leaf_hashes + 8 * (size_t)(b.first + tid), h);
    dst = aunts + 8 * (size_t)aunt_off[b.first + tid];
  }
  __syncthreads();
  uint32_t cur = 0, l = 0;
  for (uint32_t c = b.m; c > 1; c = (c + 1) >> 1, l++) {
    if (mine && merkle_aunt_lane(tid, l, c, lv[cur], h)) {
      merkle_store_node(dst, h);
      dst += 8;
    }
    merkle_level_lane(tid, c, lv[cur], lv[cur ^ 1]);
    __syncthreads();
    cur ^= 1;
  }
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 8; k++) h[k] = lv[cur][k * kMerkleB];
    merkle_store_node(out + 8 * (size_t)blockIdx.x, h);
  }
}

__global__ __launch_bounds__(256) void k_merkle_proof_spread(ProofSpread S) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g < S.n_leaves) merkle_proof_spread_lane(S, g);
}

__global__ __launch_bounds__(256) void k_merkle_proofs_verify(ProofBatch P, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) merkle_proof_verify_lane(P, i);
}

hipError_t launch_merkle_proof_pass(MerkleLeafKind kind, const MerkleLeaves& leaves, const uint32_t* wg_off,
                                    const uint32_t* leaf_off, uint32_t n_trees, uint32_t n_wg, uint32_t* out,
                                    uint32_t* leaf_hashes, const uint32_t* aunt_off, uint32_t* aunts, hipStream_t s) {
  if (n_wg == 0) return hipSuccess;
  const dim3 grid(n_wg), block(kMerkleB);
  switch (kind) {
    case kMerkleItems:
      hipLaunchKernelGGL(k_merkle_proof_pass<ProofItemLeaf>, grid, block, 0, s, ProofItemLeaf{leaves}, wg_off,
                         leaf_off, n_trees, out, leaf_hashes, aunt_off, aunts);
      break;
    case kMerkleTxs:
      hipLaunchKernelGGL(k_merkle_proof_pass<ProofTxLeaf>, grid, block, 0, s, ProofTxLeaf{leaves}, wg_off, leaf_off,
                         n_trees, out, leaf_hashes, aunt_off, aunts);
      break;
    case kMerkleNodes:
      hipLaunchKernelGGL(k_merkle_proof_pass<ProofNodeLeaf>, grid, block, 0, s, ProofNodeLeaf{leaves}, wg_off,
                         leaf_off, n_trees, out, leaf_hashes, aunt_off, aunts);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_merkle_proof_spread(const ProofSpread& S, hipStream_t s) {
  if (S.n_leaves == 0 || S.n_pass < 2) return hipSuccess;
  hipLaunchKernelGGL(k_merkle_proof_spread, dim3((S.n_leaves + 255) / 256), dim3(256), 0, s, S);
  return hipGetLastError();
}

hipError_t launch_merkle_proofs_verify(const ProofBatch& P, uint32_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_merkle_proofs_verify, dim3((n + 255) / 256), dim3(256), 0, s, P, n);
  return hipGetLastError();
}

}  // namespace cmtv
