// kernels.h -- host-side launchers for the gfx950 kernels (kernels.hip,
// keyed_forms.hip, keyed_lane.hip, keygen.hip, sr25519.hip, secp256k1.hip,
// signbytes.hip, merkle.hip, header.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cmtv {

// (1..128)B, [2^124]B, [2^128]B multiples, then (1..2^15)B, [2^120]B, [2^128]B
// multiples, then the 16-position comb (1..2^15)[2^16j]B (verify_core.h
// BTAB_TOTAL_ROWS); 36 words per row, 89.7 MB
constexpr uint32_t kBtabWords = (3 * 128 + 3 * 32768 + 16 * 32768) * 36;
constexpr uint32_t kAtabWordsPerLane = 320; // (1..8)(-A), 40 words per point
constexpr uint32_t kCombWords = 32 * 128 * 32;     // one registered-key comb (keyed.h), 512 KiB
constexpr uint32_t kCombScratchWordsPerKey = 128 * 320;  // prefix products while building

// The verification forms (launch_verify / launch_verify_sr25519 kflags bits
// 0..7; the runtime picks one per batch size, runtime_state.h ed_form / sr_form):
//   kFormLane : one signature per lane (k_verify, k_verify_sr25519)
//   kFormQuad : four lanes per signature, three quad waves + a helper wave
//               that hashes and sums each window's table entries
//               (k_verify_quad_hs_fold with a fifth wave for [s]B, or
//               k_verify_quad_hs; k_verify_sr25519_quad_hs)
//   kFormOct2 : eight lanes per signature in two waves (k_verify_oct_split)
//   kFormRow  : one wave per signature, three per workgroup + a helper
//               (k_verify_row_split)
//   kFormRow4 : four waves per signature (k_verify_row4_split)
// sr25519 has the lane and quad forms. kLaunchForceWide: the CMTV_FORCE_WIDE
// test knob (every quad-family verifier takes the 64-window schedule); bits
// 16..31: the helper-summed forms' tuning (hs_tune: CMTV_HS_PRE in its bits
// 0..7, CMTV_HS_FOLD_TUNE in bits 8..10, kHsTune* above them). kLaunchHsFold: the Ed25519 quad form
// runs k_verify_quad_hs_fold ([s]B folded into R by a fifth wave) instead of
// k_verify_quad_hs.
constexpr uint32_t kFormLane = 0, kFormQuad = 1, kFormOct2 = 2, kFormRow = 3, kFormRow4 = 4;
constexpr uint32_t kFormMask = 0xFF, kLaunchForceWide = 0x100, kLaunchHsFold = 0x200;
// hs_tune bits 11 and 12, k_verify_quad_hs_fold only: the window sums are
// split over the hash helper and the comb wave (CMTV_HS_SUM_SPLIT); the comb
// wave's half never arrives (the CMTV_FORCE_FG_LATE test knob)
constexpr uint32_t kHsTuneSumSplit = 1u << 11, kHsTuneFgLate = 1u << 12;
// hs_tune bit 13, the same kernel: the window sums are software-pipelined over
// those two waves, each sum whole on one wave (CMTV_HS_SUM_PIPE); without
// effect under kHsTuneSumSplit
constexpr uint32_t kHsTunePipe = 1u << 13;
// registered-key forms (launch_verify_keyed): the keyed row kernel
// (k_verify_keyed_row_split, one signature per workgroup), the keyed quad
// kernel with two helper waves (k_verify_keyed_quad_split), the lane kernels
// (keyed_lane.hip)
constexpr uint32_t kKeyedRow = 0, kKeyedQuad = 1, kKeyedLane = 2;

// Row kernel bitmap assembly: each launch takes the next of kRowSlots slots
// of a per-device ring (kRowSlotWords words, read as 64-bit words of 32
// two-bit verdict fields: kernel_parts.h row_bitmap_add); the wave that fills a
// word's last field writes that word's 32 bitmap bits and zeroes it. A slot is
// reused after kRowSlots further row launches on the device; the runtime
// fences a reuse against the slot's previous launch (launch.cpp
// row_slot_acquire). kRowMaxCap bounds a row launch.
constexpr uint32_t kRowSlots = 256, kRowSlotWords = 1024, kRowMaxCap = 4 * (kRowSlotWords - 16);
// A row launch's ring slot and, optionally, its tagged bitmap: with tagged
// set (a device pointer to mapped host memory, one entry per 32 signatures),
// the wave that completes word j stores (seq << 32 | the word's 32 bits) into
// tagged[j] with ONE 64-bit system-scope atomic store instead of writing the
// bitmap, so the host knows the bitmap is complete when every entry carries
// seq -- without waiting for the kernel to retire, and without any ordering
// between the waves' stores (host_batch.cpp wait_row_tags). The slot word is zero
// again before its entry is stored.
struct RowSlot {
  uint32_t* words = nullptr;
  uint64_t* tagged = nullptr;
  uint32_t seq = 0;
};

// Templated sign-bytes (signbytes.h) written by the helper waves of the
// helper-wave kernels themselves (every Ed25519 form but the lane kernels;
// the secp256k1 templated kernels, where every lane is its own helper): each
// helper lane builds its signature's CanonicalVote into an LDS slot of
// kSbFuseMaxMsg bytes and hashes it from there, so a templated commit needs
// no k_sign_bytes launch (and no global message buffer). Device pointers;
// tmpls == nullptr means the messages are in `msg`.
struct SbFuse {
  const void* tmpls = nullptr;
  const uint8_t* blob = nullptr;
  const uint32_t* tidx = nullptr;
  const uint8_t* flag = nullptr;
  const int64_t* sec = nullptr;
  const int32_t* nanos = nullptr;
};
constexpr uint32_t kSbFuseMaxMsg = 192;

// Per-device diagnostic counters the kernels bump with vector atomics
// (CmtvDev::d_diag, read by cmtv_stats_get): kDiagLateK = quad waves of
// k_verify_keyed_quad_split that stopped waiting for the hash helper and
// hashed their own signatures. kKeyedWaitDefault = the polls before that.
// kDiagLatePs = quad waves of k_verify_quad_hs_fold that stopped waiting for
// the comb wave's [s]B and added the comb rows themselves, after kPsWaitDefault
// polls. kDiagLateSum = workgroups of that kernel whose hash helper stopped
// waiting for the comb wave's half of a window sum at least once and formed
// the sum alone (at most one count per workgroup and launch).
constexpr uint32_t kDiagLateK = 0, kDiagLatePs = 1, kDiagLateSum = 2, kDiagWords = 4;
constexpr uint32_t kKeyedWaitDefault = 1u << 22, kPsWaitDefault = 1u << 22;

hipError_t launch_btab_init(uint32_t* d_rows, hipStream_t s);
// sb (may be null) is honoured by the forms whose helper wave hashes (every
// form but kFormLane); the caller launches k_sign_bytes otherwise. The row
// forms need row_slot (one slot of the device's ring) when bitmap is set.
// ps_wait, diag: the folded quad form's polls for [s]B and the device's
// diagnostic counters (may be null).
hipError_t launch_verify(uint32_t mode, uint32_t n, const void* pk, const void* sig, const void* msg,
                         const void* off, const uint32_t* btab, uint32_t* atab, void* valid, void* bitmap,
                         uint32_t kflags, hipStream_t s, const SbFuse* sb = nullptr, const RowSlot* row_slot = nullptr,
                         uint32_t ps_wait = kPsWaitDefault, uint32_t* diag = nullptr);
hipError_t launch_comb_build(uint32_t n_keys, const void* keys_pk, uint8_t* keys_ok, uint32_t* tabs,
                             uint32_t* scratch, bool negate, hipStream_t s);
// form: kKeyedRow (row_slot: a slot of the device's bitmap ring when bitmap
// is set), kKeyedQuad, kKeyedLane. sb (may be null) is honoured by the row and
// quad forms only (their helper waves hash; hipErrorInvalidValue otherwise).
// key_idx null: signature i is by key i (row and quad forms).
hipError_t launch_verify_keyed(uint32_t mode, uint32_t n, uint32_t n_keys, const void* key_idx, const void* sig,
                               const void* msg, const void* off, const uint32_t* keys_pk, const uint8_t* keys_ok,
                               const uint32_t* ktabs, void* valid, void* bitmap, uint32_t form, uint32_t k_wait,
                               uint32_t* diag, uint32_t batch_kb, uint32_t* scr, const uint32_t* wtabs,
                               const uint32_t* btab, hipStream_t s, const RowSlot* row_slot = nullptr,
                               const SbFuse* sb = nullptr);
// the one-signature-per-lane part of launch_verify_keyed (keyed_lane.hip):
// over the wide combs wtabs (rows staged by LDS-DMA) or, with wtabs null, the
// radix-256 key combs ktabs with B over btab's radix-2^16 comb
hipError_t launch_verify_keyed_lane(uint32_t mode, uint32_t n, uint32_t n_keys, const uint32_t* ki,
                                    const uint32_t* sgp, const uint8_t* mp, const uint32_t* op,
                                    const uint32_t* keys_pk, const uint8_t* keys_ok, const uint32_t* ktabs,
                                    uint8_t* vp, uint64_t* bp, uint32_t batch_kb, uint32_t* scr,
                                    const uint32_t* wtabs, const uint32_t* btab, hipStream_t s);
// Wide (radix-2^16) combs of n_keys keys (keyed.h): bases = n_keys x 16 x 40
// words, scratch = n_keys x kWideScratchWordsPerKey words.
constexpr size_t kWideTableWords = (size_t)16 * 32768 * 32;  // 64 MiB per key
constexpr size_t kWideScratchWordsPerKey = (size_t)16 * (32768 / 64) * 64 * 10;
constexpr size_t kWideBaseWordsPerKey = 16 * 40;
hipError_t launch_wide_build(uint32_t n_keys, const void* keys_pk, uint32_t* tabs, uint32_t* bases,
                             uint32_t* scratch, hipStream_t s);
// k_verify_keyed_batch: signatures per lane, and its scratch per lane
// (kb x 40 words: R'.X and R'.Y (Go) or the coset x numerator (ZIP-215), Z,
// and the running product of the Z's)
constexpr uint32_t kKeyedBatchScratchWordsPerSig = 40;
hipError_t launch_verify_sr25519(uint32_t n, const void* pk, const void* sig, const void* msg, const void* off,
                                 const uint32_t* btab, uint32_t* atab, const uint32_t* prog, int nops, void* valid,
                                 void* bitmap, uint32_t kflags, hipStream_t s);
// secp256k1 ECDSA (secp256k1.hip): the fixed table (1..128)[256^j]G, j = 0..32,
// rows of 32 words (528 KiB), built by launch_secp_gtab_build; the lane
// kernel's scratch, (1..8)Q at 30 words per point
constexpr uint32_t kSecpGtabWords = 33 * 128 * 32;
constexpr uint32_t kSecpQtabWordsPerLane = 240;
hipError_t launch_secp_gtab_build(uint32_t* d_rows, hipStream_t s);
// pk n x 33 bytes; qtab: n rounded up to 64, times kSecpQtabWordsPerLane words
hipError_t launch_verify_secp256k1(uint32_t n, const void* pk, const void* sig, const void* msg, const void* off,
                                   const uint32_t* gtab, uint32_t* qtab, void* valid, void* bitmap, hipStream_t s);
// registered secp256k1 keys: per key a table in the fixed table's layout,
// (1..128)[256^j]Q (kSecpGtabWords words, keys back to back), and an ok byte
// (0: the key is rejected, its rows are the point at infinity); pk n_keys x 33
hipError_t launch_secp_qcomb_build(uint32_t n_keys, const uint8_t* d_pk, uint8_t* d_ok, uint32_t* d_tab,
                                   hipStream_t s);
// key_idx: n words; an entry >= n_keys gives an invalid verdict. No scratch.
hipError_t launch_verify_secp256k1_keyed(uint32_t n, uint32_t n_keys, const uint32_t* key_idx, const uint8_t* key_ok,
                                         const uint32_t* qtab, const void* sig, const void* msg, const void* off,
                                         const uint32_t* gtab, void* valid, void* bitmap, hipStream_t s);
// the two with each lane's message built by the lane from its commit's
// template (sb.tmpls set; every message at most kSbFuseMaxMsg bytes; a chunk
// passes sb with flag / sec / nanos / tidx advanced to its first signature)
hipError_t launch_verify_secp256k1_tmpl(uint32_t n, const void* pk, const void* sig, const SbFuse& sb,
                                        const uint32_t* gtab, uint32_t* qtab, void* valid, void* bitmap,
                                        hipStream_t s);
hipError_t launch_verify_secp256k1_keyed_tmpl(uint32_t n, uint32_t n_keys, const uint32_t* key_idx,
                                              const uint8_t* key_ok, const uint32_t* qtab, const void* sig,
                                              const SbFuse& sb, const uint32_t* gtab, void* valid, void* bitmap,
                                              hipStream_t s);
// the keyed templated kernel with kb = 4 or 8 signatures per lane sharing one
// inversion mod n (k_verify_secp256k1_keyed_batch): ceil(n / (64 kb))
// workgroups; pre: that many x 64 lanes x kb x kSecpBatchScratchWordsPerSig
// words of scratch (each lane's running products)
constexpr uint32_t kSecpBatchScratchWordsPerSig = 8;
hipError_t launch_verify_secp256k1_keyed_batch(uint32_t kb, uint32_t n, uint32_t n_keys, const uint32_t* key_idx,
                                               const uint8_t* key_ok, const uint32_t* qtab, const void* sig,
                                               const SbFuse& sb, const uint32_t* gtab, uint32_t* pre, void* valid,
                                               void* bitmap, hipStream_t s);
hipError_t launch_sign_bytes(uint32_t n, const void* tmpls, const uint8_t* blob, const uint32_t* tidx,
                             const uint8_t* commit_flag, const int64_t* sec, const int32_t* nanos,
                             const uint32_t* off, uint8_t* msg, hipStream_t s);
// direct cross-height chunks (signbytes.hip): n_c commits (BulkDesc, their
// templates) whose arrays sit in `arena` (the chunk's device copy of the
// caller's pinned memory) -> the per-signature chunk layout of m planned
// signatures and their message offsets (off[0..m]); ctot / cbase: n_c words
// each of scratch
hipError_t launch_bulk_gather(uint32_t n_c, uint32_t m, const void* desc, const void* tmpls, const uint8_t* arena,
                              uint32_t* kidx, uint8_t* sig, uint32_t* off, uint32_t* tidx, uint8_t* flag,
                              int64_t* sec, int32_t* nanos, uint32_t* ctot, uint32_t* cbase, hipStream_t s);
hipError_t launch_pubkey(uint32_t n, const void* seeds, const uint32_t* btab, void* out_pk, hipStream_t s);
hipError_t launch_sign(uint32_t n, const void* seeds, const void* key_idx, const void* msg, const void* off,
                       const uint32_t* btab, void* out_sig, hipStream_t s);
// secp256k1 test data (secp256k1_sign.hip): priv n x 32 bytes big-endian, every
// key in [1, n - 1] (the caller checked); gtab the verifier's fixed table.
// out_pk n x 33 bytes, out_addr n x 20 bytes (4-byte aligned) or null.
hipError_t launch_secp_pubkey(uint32_t n, const void* priv, const uint32_t* gtab, void* out_pk, void* out_addr,
                              hipStream_t s);
// signature i by key key_idx[i] (null: key i) over msg[off[i] .. off[i + 1]); out_sig n x 64 bytes (4-byte aligned)
hipError_t launch_secp_sign(uint32_t n, const void* priv, const void* key_idx, const void* msg, const void* off,
                            const uint32_t* gtab, void* out_sig, hipStream_t s);
// sr25519 test data (sr25519_sign.hip): mini n x 32 bytes (16-byte aligned);
// btab the shared fixed-base table; out_pk n x 32 bytes, out_addr n x 20 bytes
// (4-byte aligned) or null.
hipError_t launch_pubkey_sr25519(uint32_t n, const void* mini, const uint32_t* btab, void* out_pk, void* out_addr,
                                 hipStream_t s);
// signature i by key key_idx[i] (null: key i) over msg[off[i] .. off[i + 1]); prog / nops the transcript's prefix
// sponge (merlin.h sr_prefix_state); out_sig n x 64 bytes (4-byte aligned)
hipError_t launch_sign_sr25519(uint32_t n, const void* mini, const void* key_idx, const void* msg, const void* off,
                               const uint32_t* btab, const uint32_t* prog, int nops, void* out_sig, hipStream_t s);

// One pass of the merkle engine (merkle.hip, merkle.h): n_wg workgroups, each
// an aligned block of one tree's leaves reduced to node g of `out` (8 words a
// node). wg_off / leaf_off: n_trees + 1 words each. What a leaf is:
//   kMerkleItems      item g = var[off[g] .. off[g + 1])
//   kMerkleValidators key g = var[off[g] .. off[g + 1]), power i64[g], key
//                     type u8[g] (u8 null: every key Ed25519)
//   kMerkleCommitSigs flag u8[g], seconds i64[g], nanos i32[g], address
//                     addr[20 g ..), signature var[off[g] .. off[g + 1])
//   kMerkleNodes      node g of `nodes`, the previous pass's output
//   kMerkleTxs        transaction g = var[off[g] .. off[g + 1]) (Txs.Hash())
// kMerkleHeaders is no pass of that kernel: a "leaf" is a whole header, hashed
// to its root by launch_header_hash below.
enum MerkleLeafKind {
  kMerkleItems = 0,
  kMerkleValidators = 1,
  kMerkleCommitSigs = 2,
  kMerkleNodes = 3,
  kMerkleTxs = 4,
  kMerkleHeaders = 5
};
struct MerkleLeaves {
  const uint8_t* var = nullptr;
  const uint32_t* off = nullptr;
  const int64_t* i64 = nullptr;
  const int32_t* i32 = nullptr;
  const uint8_t* u8 = nullptr;
  const uint8_t* addr = nullptr;
  const uint32_t* nodes = nullptr;
};
hipError_t launch_merkle_pass(MerkleLeafKind kind, const MerkleLeaves& leaves, const uint32_t* wg_off,
                              const uint32_t* leaf_off, uint32_t n_trees, uint32_t n_wg, uint32_t* out,
                              hipStream_t s);

// Header.Hash() of n headers (header.hip, header.h): root h into out[8 h ..).
// The fields, header h of n (the constants are header.h's):
//   off[12 h + f]  where byte field f starts in var (12 n + 1 offsets): the
//                  chain id, LastBlockID's hash and part-set hash, the nine
//                  hashes and the proposer address in struct order
//   i64[k n + h]   version.block, version.app, height, seconds (k = 0..3)
//   i32[k n + h]   nanos, LastBlockID's part-set total (k = 0, 1)
hipError_t launch_header_hash(const MerkleLeaves& fields, uint32_t n, uint32_t* out, hipStream_t s);

// Merkle inclusion proofs (merkle_proof.hip, merkle_proof.h). A proof pass is
// launch_merkle_pass's (kMerkleItems, kMerkleTxs or kMerkleNodes) that also
// writes each leaf's hash (leaf_hashes, 8 words a leaf; null after the first
// pass) and, per leaf g of the pass, its aunts inside its block from node
// aunt_off[g] of `aunts` on. The spreading launch appends the aunts of the
// passes after the first to every leaf's proof; the verify launch is
// Proof.Verify of n proofs, one lane each.
struct ProofSpread;
struct ProofBatch;
hipError_t launch_merkle_proof_pass(MerkleLeafKind kind, const MerkleLeaves& leaves, const uint32_t* wg_off,
                                    const uint32_t* leaf_off, uint32_t n_trees, uint32_t n_wg, uint32_t* out,
                                    uint32_t* leaf_hashes, const uint32_t* aunt_off, uint32_t* aunts, hipStream_t s);
hipError_t launch_merkle_proof_spread(const ProofSpread& S, hipStream_t s);
hipError_t launch_merkle_proofs_verify(const ProofBatch& P, uint32_t n, hipStream_t s);

}  // namespace cmtv
