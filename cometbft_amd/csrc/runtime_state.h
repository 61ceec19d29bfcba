// runtime_state.h -- the state of a context and its devices, the constants of
// the verification forms and the small helpers every launch path inlines.
// Private to the runtime's own files (runtime.cpp, launch.cpp, host_batch.cpp,
// gather.cpp, keyset.cpp, bulk_lane.cpp, merkle.cpp, header.cpp): the commit and pipeline layers see
// runtime_internal.h only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <random>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/cmtverify.h"
#include "host_pool.h"
#include "kernels.h"
#include "runtime_internal.h"

namespace cmtv {

constexpr uint32_t kChunk = 1u << 18;  // signatures per launch (A-table scratch = kChunk * 1280 B)
// registered-key lane launches take up to this many signatures, KB per lane
// (k_verify_keyed_batch, both modes: one field inversion per
// KB signatures; KB = 8 keeps 2,048 waves = two per SIMD); scratch 160 B per
// signature, in the lane kernels' scratch buffer
constexpr uint32_t kKeyedBatchChunk = 1u << 20;
constexpr uint32_t kKeyedBatchMinWaves = 2048;
// KB of a batched registered-key launch of cn signatures (4 or 8, the
// instantiated forms, else 1: one signature per lane): the widest KB up to
// max_kb that still launches min_waves waves (the last one may be partial: a
// commit-aligned 1,048,500-signature chunk takes KB = 8 in 2,048 waves).
// Shared by k_verify_keyed_batch and k_verify_secp256k1_keyed_batch.
inline uint32_t keyed_batch_kb(size_t cn, uint32_t min_waves, uint32_t max_kb = 8) {
  uint32_t kb = 1;
  while (kb < max_kb && cn > ((size_t)min_waves - 1) * 64 * (kb * 2)) kb *= 2;
  return kb >= 4 ? kb : 1;
}
// The same threshold for k_verify_secp256k1_keyed_batch (the cross-height
// typed batches, launch.cpp enqueue_verify_secp_keyed), measured apart
// (tools/bench_typed_commits.py): KB = 4 from 209,921 signatures
// per launch (820 x 256; 105,000 lost, 210,000 gained), and never KB = 8 by
// default: at every measured size KB = 4 took less kernel time than KB = 8.
// CMTV_KEYED_BATCH_MIN_WAVES sets the threshold and allows KB = 8.
constexpr uint32_t kSecpBatchMinWaves = 821;
constexpr uint32_t kSecpBatchMaxKb = 4;
// The batch-size bands of the verification forms (kernels.h kForm*, picked
// by ed_form / sr_form / keyed_form below), measured on MI355X in round 4 and
// frozen since (no more single-band tuning). CMTV_FORM forces one
// form at every size it can take (tools/*_ab.py use it for A/B runs).
// Ed25519, per call:
//   <= 256     kFormRow4  four waves per signature, one round on 256 CUs
//   <= 1,536   kFormRow   one wave per signature, two workgroups of 3 per CU
//              (profiles/r04_row_max_ab.txt: 1,024 0.215 vs oct2 0.235 ms;
//              2,048: 0.29 vs 0.24 ms)
//   <= 2,048   kFormOct2  eight lanes per signature in two waves
//              (profiles/r04_oct_hs_crossover.txt: 2,048 0.209 vs quad 0.218;
//              3,072 0.272 vs 0.221 ms)
//   <= 49,152  kFormQuad  four rounds of the helper-summed quad kernel
//              (profiles/r04_quad_max_ab.txt: 49,152 0.96 vs lane 1.15 ms;
//              65,536 1.39 vs 1.25 ms)
//   above      kFormLane
// sr25519: the same bands since the round-5 transcript (profiles/
// r05_sr_quad_max_ab.txt: 49,152 0.94 vs lane 1.15 ms; 65,536 1.37 vs 1.25;
// round 4, with the byte-code transcript, crossed at 40,000).
// Registered keys:
//   <= 512     kKeyedRow   (profiles/r04_keyed_row_max_ab.txt: 320-512
//              0.058-0.062 vs quad 0.076 ms; 640-768 lose)
//   <= 36,864  kKeyedQuad  (profiles/r02_keyed_sweep.json: 12,288 per round,
//              0.088/0.164/0.242 ms for 1-3 rounds vs the lane kernel's flat
//              0.28-0.30 ms up to 49k)
//   above      kKeyedLane
constexpr size_t kRow4Max = 256, kRowMax = 1536, kOct2Max = 2048, kQuadMax = 49152, kSrQuadMax = 49152;
constexpr size_t kKeyedRowMax = 512, kKeyedQuadMax = 36864;
constexpr uint32_t kNoForm = 0xFF;
// signatures per device below which a batch is not sharded (env CMTV_SHARD_MIN)
constexpr size_t kShardMinDefault = 8192;
// single-device host batches up to this size return their bitmap through
// mapped host memory (no D2H copy; the writes are a few PCIe transactions),
// and fused commit batches read their staging there (no H2D copy). Measured
// on MI355X (round 4, profiles/r04_zc_max_ab.txt, tools/mid_ab.py, the then knob
// 4,096 vs 16,384): VerifyCommit at 8,192 0.329-0.330 -> 0.320 ms, at 10,000
// 0.349 -> 0.341-0.343 ms; the host API unchanged. 4,096 before.
constexpr size_t kZeroCopyMax = 12288;
// tagged bitmap entries of a polled host batch (CmtvDev::h_tags): a row
// launch's 32-signature words or a keyed quad launch's 16-signature slices
constexpr size_t kTagEntries = std::max<size_t>(cmtv::kRowMaxCap / 32 + 1, 4 * ((kZeroCopyMax + 63) / 64));
constexpr int kMaxDevices = 64;

// A device (DevBuf) or pinned host (HostBuf; flags: hipHostMalloc's) buffer
// that grows a quarter past the request and never shrinks.
template <bool kHost>
struct GrowBuf {
  void* p = nullptr;
  size_t cap = 0;
  unsigned flags = hipHostMallocDefault;
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    size_t want = std::max<size_t>(bytes, 4096);
    want = want + want / 4;
    const hipError_t e = kHost ? hipHostMalloc(&p, want, flags) : hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)(kHost ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
  }
};
using DevBuf = GrowBuf<false>;
using HostBuf = GrowBuf<true>;

// Lane-kernel scratch (the generic kernel's A tables, the batched keyed
// kernel's R' and Z products) and the event of its last user: a launch on
// another stream waits for that user (acquire_scratch), growing it first
// waits for it to finish.
struct Scratch {
  DevBuf buf;
  hipEvent_t done = nullptr;
  bool used = false;
};

// The per-process key of the verdict cache's index hash (host_batch.cpp siphash24)
struct SipKey {
  uint64_t k0, k1;
  SipKey() {
    std::random_device rd;
    k0 = ((uint64_t)rd() << 32) ^ rd();
    k1 = ((uint64_t)rd() << 32) ^ rd();
  }
};

// Verdict cache (cmtv_verdict_cache): a ring of the last `cap` verdicts,
// indexed by a keyed hash of the full key (scheme + mode, pk, sig, msg); a hit
// also compares the key bytes, so it returns exactly the device verdict.
struct VerdictCache {
  struct Entry {
    std::string key;
    uint64_t h = 0;
    uint8_t verdict = 0;
    bool used = false;
  };
  SipKey sk;
  size_t cap = 0;
  size_t next = 0;
  std::vector<Entry> ring;
  std::unordered_multimap<uint64_t, size_t> index;

  uint64_t hash(const std::string& k) const;  // host_batch.cpp
  static void make_key(std::string& k, uint32_t mode, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg,
                       size_t mlen) {
    k.resize(1 + 32 + 64 + mlen);
    k[0] = (char)(mode == cmtv::kModeSr25519 ? 0x80 : mode);  // scheme + verdict mode
    std::memcpy(&k[1], pk, 32);
    std::memcpy(&k[33], sig, 64);
    if (mlen) std::memcpy(&k[97], msg, mlen);
  }
  void reset(size_t c) {
    cap = c;
    next = 0;
    ring.clear();
    ring.resize(c);
    index.clear();
  }
  // verdict or -1
  int find(uint64_t h, const std::string& k) const {
    auto r = index.equal_range(h);
    for (auto it = r.first; it != r.second; ++it)
      if (ring[it->second].key == k) return ring[it->second].verdict;
    return -1;
  }
  void insert(uint64_t h, std::string&& k, uint8_t v) {
    if (!cap) return;
    Entry& e = ring[next];
    if (e.used) {
      auto r = index.equal_range(e.h);
      for (auto it = r.first; it != r.second; ++it)
        if (it->second == next) {
          index.erase(it);
          break;
        }
    }
    e.key = std::move(k);
    e.h = h;
    e.verdict = v;
    e.used = true;
    index.emplace(h, next);
    next = (next + 1) % cap;
  }
  size_t size() const { return index.size(); }
};

// ---------------------------------------------------------------- RCCL (dlopen)
// Resolved at run time with RTLD_LOCAL so the library loads (and a context
// falls back to peer copies) where librccl is absent, and so RCCL's symbols
// never interpose on a host process that carries its own copy.
typedef void* ncclComm_t;
typedef int ncclResult_t;
constexpr int kNcclUint64 = 5;  // ncclDataType_t ncclUint64 (rccl.h)

struct Rccl {
  bool ok = false;
  ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;  // optional (a failed group's stuck ranks)
};

// Kernel timing: HIP event pairs recorded around each verification on its
// stream, harvested without blocking once complete (so device-resident calls
// stay asynchronous).
struct Timing {
  struct Pair {
    hipEvent_t a = nullptr, b = nullptr;
  };
  std::vector<Pair> free_;
  std::deque<Pair> pending;
  // pairs in flight beyond this are not timed (begin hands out a null pair)
  static constexpr size_t kMaxPending = 1u << 16;
  hipError_t begin(Pair& p, hipStream_t s) {
    if (pending.size() >= kMaxPending) {
      p = Pair();
      return hipSuccess;
    }
    if (free_.empty()) {
      Pair q;
      hipError_t e = hipEventCreate(&q.a);
      if (e == hipSuccess) e = hipEventCreate(&q.b);
      if (e != hipSuccess) return e;
      free_.push_back(q);
    }
    p = free_.back();
    free_.pop_back();
    hipError_t e = hipEventRecord(p.a, s);
    if (e != hipSuccess) free_.push_back(p);
    return e;
  }
  hipError_t end(const Pair& p, hipStream_t s) {
    if (!p.a) return hipSuccess;  // untimed (kMaxPending)
    hipError_t e = hipEventRecord(p.b, s);
    if (e != hipSuccess) {
      free_.push_back(p);
      return e;
    }
    pending.push_back(p);
    return hipSuccess;
  }
  void abandon(const Pair& p) {
    if (p.a) free_.push_back(p);
  }
  // completed pairs -> stats (context-wide and this device's); blocking
  // waits for all of them
  void harvest(cmtv_stats& st, double& dev_ms, uint64_t& dev_timed, bool blocking) {
    while (!pending.empty()) {
      Pair p = pending.front();
      // never blocks unless asked (cmtv_stats_get): a device-resident call
      // must not wait for launches parked on other streams
      if (blocking) {
        if (hipEventSynchronize(p.b) != hipSuccess) break;
      } else if (hipEventQuery(p.b) != hipSuccess) {
        break;
      }
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
        st.last_kernel_ms = ms;
        st.device_ms += ms;
        st.timed_calls++;
        dev_ms += ms;
        dev_timed++;
      }
      pending.pop_front();
      free_.push_back(p);
    }
  }
  void release() {
    for (auto& p : pending) free_.push_back(p);
    pending.clear();
    for (auto& p : free_) {
      if (p.a) (void)hipEventDestroy(p.a);
      if (p.b) (void)hipEventDestroy(p.b);
    }
    free_.clear();
  }
};

// A device's bulk lane (runtime_internal.h): staging slots and streams of
// the cross-height pipeline.
struct BulkSlot {
  HostBuf h_in;   // pinned staging, packed by the host workers
  // verdict bitmap: D2H'd into it, or (registered-key chunks) written there
  // by the kernel itself (coherent, mapped)
  HostBuf h_bm{nullptr, 0, hipHostMallocCoherent | hipHostMallocMapped};
  DevBuf d_in;    // the staging on the device, then the sign-bytes
  DevBuf d_bm;    // verdict bitmap
  hipEvent_t h2d = nullptr, done = nullptr;
  hipEvent_t prep = nullptr;  // the chunk's gather + sign-bytes done (bulk_prep_stream)
  bool pending = false;  // submitted, not yet waited for
};
struct BulkLane {
  hipStream_t copy = nullptr, exec = nullptr;
  // the exec stream of chunks submitted near a latency call: every CU but
  // the reserved ones (its own hardware queue, cu_mask), and the waves one
  // round of it holds at two per SIMD (the keyed batch kernel's occupancy)
  hipStream_t exec_masked = nullptr;
  // (no prep stream: a fifth hardware queue per lane cost the latency calls
  // beside a pipeline ~70 us of p99 -- round 6, profiles/r06_prep_queue_ab.txt;
  // an unmasked chunk's prep runs on exec_masked instead, bulk_prep_stream)
  // ... and the device's latency stream while a pipeline call is in flight
  // (LatencyStreams): the reserved CUs only, so a 150-validator commit's
  // workgroups never share a CU -- its SIMDs, its instruction cache (one per
  // CU pair) -- with the bulk launch's waves; lat_in / lat_out order it
  // after / before the device's normal stream
  hipStream_t lat = nullptr;
  hipEvent_t lat_in = nullptr, lat_out = nullptr;
  uint32_t cus = 0, masked_waves = 0;
  BulkSlot slot[cmtv::kBulkSlotsMax];
  Scratch scratch;
};

// A staging slot of the merkle engine (merkle.cpp): a run's pinned staging
// block and its copy on the device, the passes' nodes, the roots back, and
// the event after them. Two per device: one run is packed while the other
// is hashed. d_out: what a proof run writes besides its roots (merkle_proof.cpp).
struct MerkleSlot {
  HostBuf h_in, h_out;
  DevBuf d_in, d_nodes, d_out;
  hipEvent_t done = nullptr;
};

// Per-device state of a context.
struct CmtvDev {
  int ordinal = 0;
  hipStream_t stream = nullptr;
  uint32_t* d_btab = nullptr;
  uint32_t* d_srprog = nullptr;  // sr25519 transcript: the sponge after the constant prefix (merlin.h)
  // secp256k1: the fixed table (kernels.h kSecpGtabWords), built by the first
  // secp256k1 batch of the context (ensure_secp_gtab), and the host-buffer
  // call's own staging (no other entry point touches them)
  uint32_t* d_secp_gtab = nullptr;
  DevBuf secp_in, secp_out;
  std::vector<uint8_t> secp_stage;  // verify_secp_templated_locked's staging block, kept between calls
  MerkleSlot merkle[2];  // the merkle calls' own staging (devs[0] only)
  DevBuf d_in, d_out, d_all;
  HostBuf h_in, h_out;
  // small single-device host batches: the kernel writes the verdict bitmap
  // straight into this coherent, device-mapped host buffer (no D2H copy)
  HostBuf h_zc{nullptr, 0, hipHostMallocCoherent | hipHostMallocMapped};
  // ... and, with fused sign-bytes, reads its inputs straight from this one
  // (no H2D copy, no copy-engine -> compute dependency before the kernel)
  HostBuf h_zin{nullptr, 0, hipHostMallocCoherent | hipHostMallocMapped};
  // The lane kernels' A-table scratch is shared by every launch on this
  // device, whatever stream it is enqueued on: each lane launch waits for the
  // previous one (Scratch::done) so calls on different streams cannot
  // overwrite each other's tables. (The bulk lane has its own.)
  Scratch scratch;
  hipEvent_t done = nullptr;  // cross-device ordering for peer-copy gathers
  Timing timing;
  ncclComm_t comm = nullptr;
  // kernel diagnostic counters (kernels.h kDiagWords, vector atomics)
  uint32_t* d_diag = nullptr;
  // the row kernel's bitmap ring (kernels.h kRowSlots x kRowSlotWords)
  uint32_t* d_rowslots = nullptr;
  uint32_t row_seq = 0;
  // per ring slot: an event recorded after the device-resident launch that
  // last took it (row_pending), waited on before the slot is handed out again
  // (row_slot_acquire), so a slot is never shared by two launches in flight
  hipEvent_t row_ev[cmtv::kRowSlots] = {};
  bool row_pending[cmtv::kRowSlots] = {};
  // the row kernels' tagged bitmap (kernels.h RowSlot) for small host
  // batches: run_host_batch_ arms tag_arm (h_tags' device pointer) and a fresh
  // tag_seq around its launch; a row launch that takes them sets tag_used, and
  // the call polls the entries (wait_row_tags) instead of synchronising the
  // stream
  HostBuf h_tags{nullptr, 0, hipHostMallocCoherent | hipHostMallocMapped};
  uint64_t* d_tags = nullptr;
  uint64_t* tag_arm = nullptr;
  uint32_t tag_seq = 0;
  bool tag_used = false;
  // signatures per tagged entry of the launch that took the tags: 32 (row
  // kernels' words) or 16 (the keyed quad kernel's per-wave slices)
  uint32_t tag_width = 32;
  // A polled host call returns once its tags are in, while the row launch
  // may still be retiring (its last waves zero their ring words). poll_ev is
  // recorded after that launch; the next host call on the device -- before it
  // writes the mapped staging (h_zin) the launch read -- and the next row-slot
  // acquisition wait for it (settle_polled), so neither the staging nor a ring
  // slot is ever shared with a launch still in flight.
  hipEvent_t poll_ev = nullptr;
  bool poll_pending = false;
  // signatures a single-commit call copied to h_in / d_in (offset 0) before
  // planning (stage_sigs_early_locked): the source and count, and the keys
  // copied after them (generic kernels; null when none); the next staging of
  // those bytes skips them
  const uint8_t* early_src = nullptr;
  const uint8_t* early_pk = nullptr;
  size_t early_n = 0;
  // a device that returned a HIP error is taken out of the context's
  // rotation: host batches are re-planned over the others (host_batch.cpp
  // run_host_batch); CMTV_FAULT_DEV=g makes device g's first launch fail
  bool failed = false;
  bool inject_fault = false;
  // this device's share of cmtv_stats (cmtv_device_stats_get)
  uint64_t calls = 0, signatures = 0, launches = 0, timed_calls = 0;
  double device_ms = 0;
  // verification calls on this device (CMTV_TIMING samples one in timing_every)
  uint64_t timing_seq = 0;
  BulkLane bulk;  // the pipeline's lane on this device (created on first use)
};

}  // namespace cmtv

struct cmtv_ctx {
  std::vector<cmtv::CmtvDev> devs;  // devs[0]: single-device and device-resident calls
  bool rccl = false;          // gathers over an RCCL communicator
  uint32_t default_mode = CMTV_MODE_GO_STDLIB;
  std::mutex mu;
  cmtv_stats stats{};
  // CMTV_FORM: a form forced at every size it can take (kNoForm: the bands)
  uint32_t force_form = cmtv::kNoForm, force_keyed = cmtv::kNoForm;
  // CMTV_HS_PRE + 1 (bits 0..7; 0: the kernel's default), CMTV_HS_FOLD_TUNE (bits 8..10)
  uint32_t hs_tune = 0;
  // the Ed25519 quad form folds [s]B into R on a fifth wave
  // (k_verify_quad_hs_fold; CMTV_HS_FOLD=0: k_verify_quad_hs), and its quads'
  // polls for that wave's [s]B before they add the comb rows themselves
  // (CMTV_FORCE_PS_LATE=1: 0, every quad wave does)
  bool hs_fold = true;
  uint32_t ps_wait = cmtv::kPsWaitDefault;
  // CMTV_HS_SUM_SPLIT=1: that kernel's hash helper and comb wave share every
  // window's sum (off by default: measured a tie);
  // CMTV_FORCE_FG_LATE=1: the comb wave's half never arrives and the helper
  // falls back on every window (it turns the split on unless the other knob
  // says 0)
  bool hs_sum_split = false, fg_late = false;
  // CMTV_HS_SUM_PIPE: the two waves form every second window's sum each, half
  // a sum per window (hs_helper.h hs_helper_sums_pipe); 0 = the hash helper
  // forms them alone. The split above, where it is on, takes precedence
  bool hs_sum_pipe = true;
  // diag[kDiagLateSum] of every device, summed by read_diag (cmtv_late_sum_waves)
  uint64_t late_sum_waves = 0;
  size_t lane_chunk = cmtv::kChunk;         // signatures per lane-kernel launch (env CMTV_LANE_CHUNK)
  size_t shard_min = cmtv::kShardMinDefault;
  int sr_nops = 0;
  cmtv::VerdictCache cache;                 // cmtv_verdict_cache (off by default)
  // cmtv_keyset_cache: validator sets (their concatenated keys) -> registered
  // key sets, used by cmtv_verify_commit(s); FIFO of at most keyset_cap
  size_t keyset_cap = 0;
  std::vector<std::pair<std::string, cmtv_keyset*>> keysets;
  // ... and the registered secp256k1 sets of typed commits (commit_typed.cpp;
  // keyset.cpp secp_keyset_for_locked): a list of its own under the same cap,
  // oldest out, compared by key bytes (n x 33), never pinned
  std::vector<cmtv_secp_keyset*> secp_keysets;
  // CMTV_FAULT_AT: 1-based index of the verification launch that fails
  uint64_t fault_at = 0, launch_seq = 0;
  bool fault_pending = false;  // the last failure was CMTV_FAULT_AT's
  // RCCL options read at open (CMTV_FORCE_RCCL, CMTV_NO_RCCL) and the
  // library to load (CMTV_RCCL_LIB; empty: the system librccl)
  bool force_rccl = false, no_rccl = false, no_rccl_fallback = false;
  std::string rccl_lib;
  // a gather failed inside RCCL: the context never builds a communicator
  // again (rebuild_comm after a device retirement included); gathers use
  // peer copies. rccl_drain_ms bounds the wait for the failed group's
  // streams (CMTV_RCCL_DRAIN_MS): a rank whose collective was enqueued before
  // the group failed never completes without its peers.
  bool rccl_broken = false;
  uint32_t rccl_drain_ms = 2000;
  // CMTV_FORCE_WIDE: quad kernels take the 64-window half-scalar fallback
  bool force_wide = false;
  // templated sign-bytes in the split kernels' helper waves (CMTV_NO_SB_FUSE=1: off)
  bool sb_fuse = true;
  // polls of the keyed split kernel's quads for the hash helper's k before
  // they hash themselves (CMTV_FORCE_K_LATE=1: 0, every quad wave hashes)
  uint32_t keyed_wait = cmtv::kKeyedWaitDefault;
  // waves a batched launch must keep (CMTV_KEYED_BATCH_MIN_WAVES; 1 batches
  // any size, the test knob that puts the corpus through the batched kernels)
  uint32_t keyed_batch_min_waves = cmtv::kKeyedBatchMinWaves;
  // the same for the secp256k1 batched kernel, and its widest KB
  // (CMTV_KEYED_BATCH_MIN_WAVES sets both thresholds and lifts the KB to 8;
  // a threshold of 0: off)
  uint32_t secp_batch_min_waves = cmtv::kSecpBatchMinWaves;
  uint32_t secp_batch_max_kb = cmtv::kSecpBatchMaxKb;
  // devices (indices into devs) that take host batches, in shard order; the
  // RCCL communicator (when rccl) spans exactly these, rank = position
  std::vector<size_t> live;
  // fused small host batches read their inputs from mapped host memory (CMTV_NO_ZC_IN=1: off)
  bool zc_in = true;
  bool zc_host_in = true;  // CMTV_ZC_HOST_IN=0: host-API batches copy their staging to HBM
  bool early_sigs = true;  // CMTV_EARLY_SIGS=0: a commit's signatures are staged after its plan
  // single-device host batches up to this size take the mapped-memory path
  size_t zc_max = cmtv::kZeroCopyMax;
  // small host batches on a row kernel poll its tagged bitmap words
  // (run_host_batch_); CMTV_HOST_POLL=0 synchronises the stream
  bool host_poll = true;
  // set while a host-buffer call runs (run_host_batch): its launches finish
  // before the call returns, so their row-ring slots need no fence event
  bool host_sync = false;
  // CMTV_ROW_FENCE=0: no row-ring fence (only for the test that shows the race)
  bool row_fence = true;
  // kernel timing by HIP event pairs on one call in timing_every per device
  // (cmtv_stats device_ms / timed_calls; CMTV_TIMING=N, 0: off). The pair's
  // marker packets cost ~4 us of a 150-validator call and ~8 us between
  // back-to-back 10k launches (tools/step_gap.py), so not every call pays.
  uint32_t timing_every = 16;
  // CMTV_HOST_PHASES=1: host phase clock (runtime_internal.h HostPhase)
  bool phases_on = false;
  uint64_t phase_ns[cmtv::kPhCount] = {};
  uint64_t phase_calls = 0;
  // CMTV_FAULT_SYNC_DEV=g: device g's stream synchronisation in a host batch
  // reports a HIP error (a fault found after the launch; re-shard test knob)
  long fault_sync_dev = -1;
  // the cross-height pipeline (pipeline.cpp): its bulk lanes and worker pool
  // belong to the holder of bulk_mu; cmtv_verify_commits calls of at least
  // pipe_min signatures take it (CMTV_PIPE_MIN; CMTV_PIPELINE=0: never),
  // in chunks of about pipe_chunk signatures (CMTV_PIPE_CHUNK) over
  // pipe_slots staging slots per device (CMTV_PIPE_SLOTS), on host_threads
  // threads (CMTV_HOST_THREADS; default: the CPUs this process may use, less
  // 3 when more than 8, at most 16: host_pool)
  std::mutex bulk_mu;
  std::unique_ptr<cmtv::HostPool> pool;
  unsigned host_threads = 0;
  size_t pipe_min = 32768, pipe_chunk = 1u << 20;
  int pipe_slots = 3;
  bool pipe_on = true;
  bool pipe_direct = true;  // CMTV_PIPE_DIRECT=0: pinned arguments are packed too
  // Latency calls beside a pipeline (a 150-validator
  // VerifyCommit from consensus while blocksync replays): a pipeline chunk
  // submitted within lat_window_ns of such a call (cmtv_verify_commit, a
  // small one-batch cmtv_verify_commits or host batch: note_latency) runs on
  // the lane's CU-masked exec stream, which leaves lat_reserve_cus CUs (one
  // per 32) to the device's normal stream, and is cut to what the other CUs
  // hold in one round; while a pipeline call is in flight (bulk_busy) the
  // latency call takes a form that fits those CUs (under_load, snapshotted at
  // each lock hold). CMTV_LAT_WINDOW_MS (default 10,000; 0: never masked),
  // CMTV_LAT_RESERVE_CUS (default 16); CMTV_LOAD_FORM=0 keeps the latency
  // call's idle form under load.
  std::atomic<uint64_t> last_latency_ns{0};
  bool load_form = true;
  // a pipeline call is in flight (snapshotted with under_load): a registered-
  // key latency batch then reads its staging in place (mapped host memory)
  // rather than queue its H2D copy on the copy engines behind the pipeline's
  // chunk DMAs; CMTV_LOAD_ZC=0 copies it as when idle
  bool bulk_now = false, load_zc = true;
  // ... and waits for its stream rather than polling its kernel's tagged
  // bitmap (run_host_batch_; CMTV_LOAD_POLL=1 polls as when idle)
  bool load_nopoll = true;
  // the quad kernels' tagged slices (CMTV_QUAD_POLL=1): polling a 10k commit
  // was slower than waiting for its stream on MI355X (round 6,
  // tools/gpu_r6p.sh, three alternating rounds: keyset pinned p50 0.112-0.119
  // polled vs 0.108-0.110 ms, generic 0.269-0.279 vs 0.267 ms), so off
  bool quad_poll = false;
  // registered-key small batches read their staging in place -- signatures in
  // the caller's cmtv_alloc_pinned memory straight from there -- instead of
  // an early signature DMA + the split staging (CMTV_KEYED_ZC=0). Measured
  // on MI355X (round 6, tools/gpu_r6x.sh, three alternating rounds):
  // verify_commit_10k_keyset pinned p50 0.105 / 0.1085 / 0.1051 against
  // 0.1118 / 0.1074 / 0.108 ms, heap 0.114-0.117 against 0.117-0.123 ms
  bool keyed_zc = true;
  bool spin_wait = false;  // CMTV_SPIN_WAIT (wait_stream)
  bool prep_stream = true;  // CMTV_PREP_STREAM (BulkLane::prep)
  bool one_exec = false;    // CMTV_ONE_EXEC (bulk_lane_init)
  // CMTV_BULK_BM_DIRECT=1 (bulk_submit_locked): off -- two alternating rounds
  // (profiles/r06_bm_direct_ab.txt) gave VerifyCommit -0.13 ms but
  // VerifyCommitLight +0.5-0.7 ms per pass
  bool bulk_bm_direct = false;
  bool split_submit = true;  // CMTV_SPLIT_SUBMIT (PipeConfig::split_submit)
  // CMTV_CALL_TRACE=1 (diagnostics): per single-commit call, the time to the
  // context lock, to the launch, to the verdicts and to the return; their
  // percentiles printed on stderr at cmtv_close
  bool call_trace = false, call_trace_loaded_only = false;
  uint64_t trace_launch = 0, trace_wait = 0;  // this hold's marks (lock held)
  uint64_t trace_dev_ns = 0;
  hipEvent_t trace_ev[2] = {nullptr, nullptr};
  std::mutex trace_mu;
  std::vector<std::array<uint64_t, 5>> trace_rows;
  uint64_t lat_window_ns = 10'000'000'000ull;
  uint32_t lat_reserve_cus = 16;
  // latency calls beside a pipeline run on the reserved CUs only
  // (LatencyStreams; CMTV_LAT_ISOLATE=0: on the whole device, beside the
  // bulk waves)
  bool lat_isolate = true;
  std::atomic<int> bulk_busy{0};
  // threads blocked in ctx_lock: a pipeline re-taking the lock for its next
  // chunk lets them in first (bulk_relock)
  std::atomic<int> lock_waiters{0};
  bool under_load = false;
  uint32_t cus = 0;  // CUs per device (the smallest of the context's)
  // the caller's pinned blocks (cmtv_alloc_pinned): base -> bytes; chunks
  // whose arrays lie in one are DMA'd from it (pipeline.cpp direct chunks)
  std::map<uintptr_t, size_t> pinned;
  // the last key set keyset_for_locked returned, by the caller's key array
  // (commit.cpp's speculative VerifyCommit launches with it, and checks the
  // keys' bytes while the kernel runs); cleared when that set is evicted
  uint32_t spec_min = 2048;  // CMTV_SPEC_MIN; CMTV_SPEC=0: 0 (off)
  const uint8_t* guess_pk = nullptr;
  size_t guess_n = 0;
  const cmtv_keyset* guess_ks = nullptr;
  // cached key sets evicted while a pipeline call had them pinned
  std::vector<cmtv_keyset*> zombies;
  cmtv::PipeWorkspace* pipe_ws = nullptr;
};

struct cmtv_keyset {
  struct PerDev {
    uint32_t* d_pk = nullptr;   // n x 8 words, the keys' original bytes
    uint8_t* d_ok = nullptr;    // n decode flags
    uint32_t* d_tab = nullptr;  // n x kCombWords
    uint32_t* d_wide = nullptr; // n x kWideTableWords (CMTV_KEYS_WIDE), else null
  };
  cmtv_ctx* ctx = nullptr;
  size_t n = 0;
  int pins = 0;               // pipeline calls using this cached set
  bool evicted = false;       // left the keyset cache while pinned
  std::vector<PerDev> dev;    // one per device of the context
  std::vector<uint8_t> pk;    // host copy (n x 32)
};

// Registered secp256k1 keys: on devs[0] only, as every secp256k1 launch.
struct cmtv_secp_keyset {
  cmtv_ctx* ctx = nullptr;
  size_t n = 0;
  std::vector<uint8_t> pk;    // host copy (n x 33)
  uint8_t* d_pk = nullptr;    // n x 33, what the build kernel parsed
  uint8_t* d_ok = nullptr;    // n flags: 0 = rejected key
  uint32_t* d_tab = nullptr;  // n x kSecpGtabWords
};

namespace cmtv {

inline int hip_fail(hipError_t e) {
  if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) return CMTV_ENOMEM;
  return CMTV_EHIP;
}

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

inline uint64_t now_ns_steady() {
  return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
             std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

// phase_now (runtime_internal.h) for the runtime's own launch paths
inline uint64_t phase_clock(const cmtv_ctx* ctx) { return ctx->phases_on ? now_ns_steady() : 0; }

// A lane launch's scratch (Scratch: a device's, shared by every stream, or
// the bulk lane's): the launch waits for the previous user, growing it first
// waits for that user to finish.
inline hipError_t acquire_scratch(Scratch& S, size_t bytes, hipStream_t s) {
  hipError_t e;
  if (bytes > S.buf.cap) {
    // growing frees the old scratch: every earlier user must be done
    if (S.used && (e = hipEventSynchronize(S.done)) != hipSuccess) return e;
    if ((e = S.buf.ensure(bytes)) != hipSuccess) return e;
  }
  if (S.used && (e = hipStreamWaitEvent(s, S.done, 0)) != hipSuccess) return e;
  return hipSuccess;
}

inline hipError_t release_scratch(Scratch& S, hipStream_t s) {
  const hipError_t e = hipEventRecord(S.done, s);
  if (e == hipSuccess) S.used = true;
  return e;
}

// Waits for the last polled host launch on D (CmtvDev::poll_ev); it has
// normally retired by then, so this is one event query.
inline hipError_t settle_polled(CmtvDev& D) {
  if (!D.poll_pending) return hipSuccess;
  hipError_t e = hipEventQuery(D.poll_ev);
  if (e == hipErrorNotReady) e = hipEventSynchronize(D.poll_ev);
  if (e == hipSuccess) D.poll_pending = false;
  return e;
}

// The form of a batch of n Ed25519 signatures (the bands above, or CMTV_FORM
// where the forced form can take n: a row form at most kRowMaxCap in one launch)
inline uint32_t ed_form(const cmtv_ctx* ctx, size_t n) {
  const uint32_t f = ctx->force_form;
  if (f != kNoForm && !((f == kFormRow || f == kFormRow4) && n > kRowMaxCap)) return f;
  // beside a running pipeline only its reserved CUs are free: 48 signatures
  // per workgroup (quad) rather than one (row) or eight (oct)
  if (ctx->under_load && n <= kQuadMax) return kFormQuad;
  return n <= kRow4Max ? kFormRow4 : n <= kRowMax ? kFormRow : n <= kOct2Max ? kFormOct2 : n <= kQuadMax ? kFormQuad
                                                                                                       : kFormLane;
}

// ... of sr25519 signatures (the quad and lane forms)
inline uint32_t sr_form(const cmtv_ctx* ctx, size_t n) {
  const uint32_t f = ctx->force_form;
  if (f == kFormQuad || f == kFormLane) return f;
  return n <= kSrQuadMax ? kFormQuad : kFormLane;
}

// ... and of registered-key signatures
inline uint32_t keyed_form(const cmtv_ctx* ctx, size_t n) {
  const uint32_t f = ctx->force_keyed;
  if (f != kNoForm && !(f == kKeyedRow && n > kRowMaxCap)) return f;
  if (ctx->under_load && n <= kKeyedQuadMax) return kKeyedQuad;  // as ed_form
  return n <= kKeyedRowMax ? kKeyedRow : n <= kKeyedQuadMax ? kKeyedQuad : kKeyedLane;
}

// The forms whose helper wave can write templated sign-bytes itself
// (kernels.h SbFuse) when they run in one launch (enqueue_verify rejects a
// fused batch of more than kChunk): every form but the lane kernels. The one
// predicate enqueue_shard and the enqueue functions use.
inline bool fuse_ok(const cmtv_ctx* ctx, size_t n) { return ed_form(ctx, n) != kFormLane && n <= kChunk; }
inline bool keyed_fuse_ok(const cmtv_ctx* ctx, size_t n) { return keyed_form(ctx, n) != kKeyedLane && n <= kChunk; }

// ---------------------------------------------------------------- across files
// runtime.cpp: completed timing pairs of every usable device -> stats
void harvest(cmtv_ctx* ctx, bool blocking);

// launch.cpp: CMTV_FAULT_AT -- counts a launch, true when it is the one to fail
bool fault_hit(cmtv_ctx* ctx);

// launch.cpp: enqueue verification of n signatures whose inputs are in device
// memory of device D (current on this thread), on stream s
int enqueue_verify(cmtv_ctx* ctx, CmtvDev& D, size_t n, const uint8_t* d_pk, const uint8_t* d_sig,
                   const uint8_t* d_msg, const uint32_t* d_off, uint32_t mode, uint8_t* d_valid, uint64_t* d_bitmap,
                   hipStream_t s, const SbFuse* sb = nullptr, Scratch* scr = nullptr);
int enqueue_verify_keyed(cmtv_ctx* ctx, CmtvDev& D, const cmtv_keyset::PerDev& K, size_t n_keys, size_t n,
                         const uint32_t* d_idx, const uint8_t* d_sig, const uint8_t* d_msg, const uint32_t* d_off,
                         uint32_t mode, uint8_t* d_valid, uint64_t* d_bitmap, hipStream_t s, Scratch* scr = nullptr,
                         const SbFuse* sb = nullptr, uint32_t min_waves = 0);
int enqueue_verify_secp(cmtv_ctx* ctx, CmtvDev& D, size_t n, const uint8_t* d_pk, const uint8_t* d_sig,
                        const uint8_t* d_msg, const uint32_t* d_off, uint8_t* d_valid, uint64_t* d_bitmap,
                        hipStream_t s, const SbFuse* sb = nullptr);
int enqueue_verify_secp_keyed(cmtv_ctx* ctx, CmtvDev& D, const cmtv_secp_keyset* ks, size_t n, const uint32_t* d_idx,
                              const uint8_t* d_sig, const uint8_t* d_msg, const uint32_t* d_off, uint8_t* d_valid,
                              uint64_t* d_bitmap, hipStream_t s, const SbFuse* sb = nullptr, bool batch = false);
// commit signatures, sign-bytes from templates: fused (max_len <= kSbFuseMaxMsg)
// or through k_sign_bytes into d_msg at d_off
int enqueue_verify_secp_templated(cmtv_ctx* ctx, CmtvDev& D, size_t n, const uint8_t* d_pk,
                                  const cmtv_secp_keyset* ks, const uint32_t* d_idx, const uint8_t* d_sig,
                                  const SbFuse& sb, uint32_t max_len, const uint32_t* d_off, uint8_t* d_msg,
                                  uint8_t* d_valid, uint64_t* d_bitmap, hipStream_t s, bool batch = false);
// secp256k1 test data (secp256k1_sign.hip) from host buffers, on device D
// (current on this thread), blocking, in launches of kChunk; the arguments
// checked by the caller (runtime.cpp). Lock held.
int secp_pubkeys_host_locked(cmtv_ctx* ctx, CmtvDev& D, size_t n, const uint8_t* priv, uint8_t* out_pk,
                             uint8_t* out_addr);
int secp_sign_host_locked(cmtv_ctx* ctx, CmtvDev& D, size_t n_keys, const uint8_t* priv, size_t n,
                          const uint32_t* key_idx, const uint8_t* msg, const uint32_t* msg_off, uint8_t* out_sig);
// the same for sr25519 (sr25519_sign.hip): mini secrets, any 32 bytes each
int sr_pubkeys_host_locked(cmtv_ctx* ctx, CmtvDev& D, size_t n, const uint8_t* mini, uint8_t* out_pk,
                           uint8_t* out_addr);
int sr_sign_host_locked(cmtv_ctx* ctx, CmtvDev& D, size_t n_keys, const uint8_t* mini, size_t n,
                        const uint32_t* key_idx, const uint8_t* msg, const uint32_t* msg_off, uint8_t* out_sig);

// host_batch.cpp: a host batch straight to the devices (no verdict cache),
// generic keys or (ks) registered ones; secp256k1 on devs[0]. Lock held.
int verify_host_device(cmtv_ctx* ctx, size_t n, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg,
                       const uint32_t* msg_off, uint32_t mode, uint8_t* out_valid, uint64_t* out_bitmap,
                       const cmtv_keyset* ks = nullptr, const uint32_t* key_idx = nullptr);
// (keys: n x 33 key bytes, or with ks n u32 indices of its registered keys)
int verify_secp_host_locked(cmtv_ctx* ctx, const cmtv_secp_keyset* ks, size_t n, const void* keys, const uint8_t* sig,
                            const uint8_t* msg, const uint32_t* msg_off, uint8_t* out_valid, uint64_t* out_bitmap);

// gather.cpp
int gather_bitmaps(cmtv_ctx* ctx, const size_t* dev, size_t G, size_t W, uint64_t* const* bufs);
void drop_comms(cmtv_ctx* ctx, bool abort);
void rebuild_comm(cmtv_ctx* ctx);
void retire_device(cmtv_ctx* ctx, size_t d);

// bulk_lane.cpp
void bulk_lane_release(CmtvDev& D);

}  // namespace cmtv
