// pipeline.cpp -- cmtv_verify_commits for large cross-height batches
// (blocksync and light-client replay: blockchain/v0/reactor.go:349-400,
// light/client.go:613-689; BASELINE configs[2], 100k commits x 150).
//
// The one-batch path (commit.cpp) plans, stages and replays a call on one
// thread with the context lock held throughout, and stages the whole batch
// before the first kernel starts. Here a call is cut into chunks of about
// CMTV_PIPE_CHUNK planned signatures (commit-aligned, one registered key set
// per chunk) that flow through the per-device bulk lanes (bulk_lane.cpp).
// One call is one PipeRun; its stages are its members:
//
//   plan     plan_window, plan_direct: every commit's preamble and plan (the
//            signatures the reference loop can reach:
//            types/validator_set.go:685-707, 740-762, 793-823), its template
//            and sign-bytes lengths -- host workers
//   cut      cut_chunk (size_chunks, scan, pin_keyset, demote, layout_spans):
//            the next chunk's commits, key set and layout -- calling thread
//   pack     pack, pack_direct: a chunk's keys / indices, signatures,
//            timestamps, flags and templates into its slot's pinned staging
//            -- host workers
//   submit   submit: H2D on the lane's copy stream, k_sign_bytes + the verify
//            kernel + the bitmap D2H on its exec stream -- context lock held
//   replay   retire, replay: each commit's reference loop over the chunk's
//            verdict bits (commit_internal.h job_replay) -- host workers
//
// Chunk c+1 is packed while the device verifies chunk c, and chunk c-k is
// replayed while it does: with S slots per device and G devices, G x S
// chunks are in flight (attempt). Chunks go round-robin over the live
// devices, each with its own lane; a device that fails with a HIP error is
// retired and the chunks not yet replayed are run again on the others (run).
// Verdicts, errors and early exits are exactly the one-batch path's (the same
// plan and replay code, the same kernels).
#include <emmintrin.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "commit_internal.h"
#include "host_pool.h"
#include "runtime_internal.h"
#include "signbytes.h"

namespace cmtv {

namespace {

uint64_t now_ns() {
  return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
             std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

// The caller's arrays a direct chunk reads (BulkLayout), by class: the
// signatures, ts_seconds, ts_nanos and flags of its commits' plans. Each
// class's [lo, hi) over the chunk's commits; the DMA copies their union
// (classes closer than kSpanGap merged into one span).
constexpr int kClsSig = 0, kClsSec = 1, kClsNanos = 2, kClsFlags = 3, kClasses = 4;
constexpr uintptr_t kSpanGap = 64 * 1024;
struct SpanAcc {
  uintptr_t lo[kClasses], hi[kClasses];
  uint64_t need = 0;  // bytes the plans read
  SpanAcc() {
    for (int k = 0; k < kClasses; k++) {
      lo[k] = UINTPTR_MAX;
      hi[k] = 0;
    }
  }
  static void ranges(const cmtv_commit* cm, size_t m, uintptr_t* a, size_t* len) {
    a[kClsSig] = reinterpret_cast<uintptr_t>(cm->sigs + cm->sig_off[0]);
    len[kClsSig] = 64 * m;
    a[kClsSec] = reinterpret_cast<uintptr_t>(cm->ts_seconds);
    len[kClsSec] = 8 * m;
    a[kClsNanos] = reinterpret_cast<uintptr_t>(cm->ts_nanos);
    len[kClsNanos] = 4 * m;
    a[kClsFlags] = reinterpret_cast<uintptr_t>(cm->flags);
    len[kClsFlags] = m;
  }
  // a commit's m signatures, from the class starts ranges() gave (lengths:
  // 64, 8, 4, 1 per signature)
  void add(const uintptr_t* a, size_t m) {
    static constexpr size_t w[kClasses] = {64, 8, 4, 1};
    for (int k = 0; k < kClasses; k++) {
      lo[k] = std::min(lo[k], a[k]);
      hi[k] = std::max(hi[k], a[k] + w[k] * m);
    }
    need += 77 * m;
  }
  // the merged spans (sorted by address): count, and [slo, shi) of each
  int merge(uintptr_t* slo, uintptr_t* shi, int* cls_span) const {
    int order[kClasses] = {0, 1, 2, 3};
    std::sort(order, order + kClasses, [&](int x, int y) { return lo[x] < lo[y]; });
    int ns = 0;
    for (int j = 0; j < kClasses; j++) {
      const int k = order[j];
      if (lo[k] >= hi[k]) {  // nothing of this class (m == 0 everywhere)
        cls_span[k] = -1;
        continue;
      }
      if (ns && lo[k] <= shi[ns - 1] + kSpanGap) {
        shi[ns - 1] = std::max(shi[ns - 1], hi[k]);
      } else {
        slo[ns] = lo[k];
        shi[ns] = hi[k];
        ns++;
      }
      cls_span[k] = ns - 1;
    }
    return ns;
  }
  // the classes' extents summed (>= merged_bytes when they do not overlap)
  uint64_t sum_bytes() const {
    uint64_t b = 0;
    for (int k = 0; k < kClasses; k++) b += lo[k] < hi[k] ? hi[k] - lo[k] : 0;
    return b;
  }
  uint64_t merged_bytes() const {
    uintptr_t slo[kClasses], shi[kClasses];
    int cs[kClasses];
    const int ns = merge(slo, shi, cs);
    uint64_t b = 0;
    for (int j = 0; j < ns; j++) b += shi[j] - slo[j];
    return b;
  }
  // the DMA would copy far more than the plans read (a caller's arrays
  // scattered over its pinned block): PipeConfig span_factor, span_slack
  bool over(const PipeConfig& pc) const {
    const uint64_t cap = pc.span_factor * need + pc.span_slack;
    return sum_bytes() > cap && merged_bytes() > cap;
  }
};

struct Chunk {
  size_t c0 = 0, c1 = 0;              // commits [c0, c1)
  const cmtv_valset* vs = nullptr;    // the key class of its signatures
  const cmtv_keyset* ks = nullptr;    // registered keys, or null (generic kernel)
  size_t dev = 0;                     // where it was submitted
  int slot = 0;
  bool direct = false;                // DMA'd from the caller's pinned block (BulkLayout)
  SpanAcc acc;                        // direct: the classes' extents ...
  uintptr_t cls_lo[kClasses] = {};    // ... and where each class starts, host
  uint64_t cls_dev[kClasses] = {};    // and device (from o_arena)
  BulkLayout L;
};

// The first invalid verdict among batch bits [i0, i0 + m) as a plan index
// (m: all valid).
size_t first_invalid(const uint64_t* bm, size_t i0, size_t m) {
  const size_t end = i0 + m;
  for (size_t i = i0; i < end;) {
    const size_t b = i & 63, lim = std::min<size_t>(64 - b, end - i);
    uint64_t x = ~bm[i >> 6] >> b;
    if (lim < 64) x &= (1ull << lim) - 1;
    if (x) return i + (size_t)__builtin_ctzll(x) - i0;
    i += lim;
  }
  return m;
}

// The valid verdicts among batch bits [0, m).
uint64_t count_valid(const uint64_t* bm, size_t m) {
  uint64_t valid = 0;
  for (size_t w = 0; w < m / 64; w++) valid += (uint64_t)__builtin_popcountll(bm[w]);
  if (m & 63) valid += (uint64_t)__builtin_popcountll(bm[m / 64] & ((1ull << (m & 63)) - 1));
  return valid;
}

// The pinned block holding [p, p + len), or -1.
long find_block(const std::vector<PinnedRange>& pins, const void* p, size_t len) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  auto it = std::upper_bound(pins.begin(), pins.end(), a,
                             [](uintptr_t x, const PinnedRange& r) { return x < r.base; });
  if (it == pins.begin()) return -1;
  --it;
  if (a + len < a || a + len > it->base + it->bytes) return -1;
  return (long)(it - pins.begin());
}

// Copy into the pinned staging with non-temporal stores: the staging is
// written once by the host and read once by the H2D copy, so its lines need
// not be read for ownership or kept in the cache (the pack is bound by host
// memory traffic: ~165 B per signature instead of ~250). The writer calls
// nt_fence before its block's bytes may be read.
inline void nt_copy(uint8_t* dst, const uint8_t* src, size_t n) {
  const size_t head = std::min(n, (size_t)((16 - ((uintptr_t)dst & 15)) & 15));
  std::memcpy(dst, src, head);
  dst += head;
  src += head;
  n -= head;
  for (; n >= 64; n -= 64, dst += 64, src += 64) {
    const __m128i a = _mm_loadu_si128(reinterpret_cast<const __m128i*>(src));
    const __m128i b = _mm_loadu_si128(reinterpret_cast<const __m128i*>(src + 16));
    const __m128i c = _mm_loadu_si128(reinterpret_cast<const __m128i*>(src + 32));
    const __m128i d = _mm_loadu_si128(reinterpret_cast<const __m128i*>(src + 48));
    _mm_stream_si128(reinterpret_cast<__m128i*>(dst), a);
    _mm_stream_si128(reinterpret_cast<__m128i*>(dst + 16), b);
    _mm_stream_si128(reinterpret_cast<__m128i*>(dst + 32), c);
    _mm_stream_si128(reinterpret_cast<__m128i*>(dst + 48), d);
  }
  for (; n >= 16; n -= 16, dst += 16, src += 16)
    _mm_stream_si128(reinterpret_cast<__m128i*>(dst), _mm_loadu_si128(reinterpret_cast<const __m128i*>(src)));
  std::memcpy(dst, src, n);
}

inline void nt_fence() { _mm_sfence(); }

// Two validator-set structs over the same arrays (a caller typically hands
// one struct per commit, all pointing at its set's arrays): one evaluation
// of the set serves both within a call.
inline bool same_arrays(const cmtv_valset* a, const cmtv_valset* b) {
  return a == b || (a->n_vals == b->n_vals && a->pubkeys == b->pubkeys && a->pk_off == b->pk_off &&
                    a->voting_power == b->voting_power);
}

// keys of vals are all 32 bytes and packed (what a registered key set needs)
bool packed_keys(const cmtv_valset* v) {
  if (!v->n_vals) return false;
  for (uint32_t i = 0; i <= v->n_vals; i++)
    if (v->pk_off[i] != 32 * i) return false;
  return true;
}

// every flag of fl[0, k) is BlockIDFlagCommit (eight at a time)
inline bool all_commit(const uint8_t* fl, uint32_t k) {
  uint64_t bad = 0;
  uint32_t i = 0;
  for (; i + 8 <= k; i += 8) {
    uint64_t w;
    std::memcpy(&w, fl + i, 8);
    bad |= w ^ 0x0202020202020202ull;
  }
  for (; i < k; i++) bad |= fl[i] ^ kFlagCommit;
  return bad == 0;
}

// the exact sign-bytes of a planned commit (pi: its plan, m > 0 long)
uint64_t exact_mbytes(const cmtv_commit* cm, const uint32_t* pi, size_t m, const TplLens& tlz) {
  const uint8_t* fl = cm->flags;
  const int64_t* se = cm->ts_seconds;
  const int32_t* na = cm->ts_nanos;
  uint64_t mb = 0;
  if (pi[m - 1] - pi[0] == m - 1) {  // a contiguous plan (the common case)
    const uint32_t a = pi[0];
    for (size_t k = 0; k < m; k++) mb += msg_len(tlz, fl[a + k] == kFlagCommit, se[a + k], na[a + k]);
  } else {
    for (size_t k = 0; k < m; k++) {
      const uint32_t idx = pi[k];
      mb += msg_len(tlz, fl[idx] == kFlagCommit, se[idx], na[idx]);
    }
  }
  return mb;
}

}  // namespace

// The pipeline's per-call arrays, kept by the context between calls
// (runtime_internal.h pipe_workspace).
struct PipeWorkspace {
  std::unique_ptr<uint32_t[]> pidx, pval;  // plan: commit / validator index per signature
  size_t cap_idx = 0, cap_val = 0;
  // base: each commit's first signature in the call; sp, mp, tp: chunk-local
  // offsets of its first planned signature / sign-byte / template byte
  std::vector<uint64_t> base, mbytes, sp, mp, tp;
  std::vector<uint32_t> plen, tlen;
  // each commit's preamble outcome, kept from the plan to the replay
  std::vector<int32_t> early;
  std::vector<int64_t> needed;
  std::vector<const AddrIndex*> addr;  // LightTrusting
  // direct commits: their prefix plan's tally and the pinned block of their
  // arrays (direct[c] = 1)
  std::vector<uint8_t> direct;
  std::vector<int64_t> ptally;
  std::vector<uint32_t> pblock;
  // ... and where each of their array classes starts (SpanAcc::ranges, kept
  // by the parallel plan so the serial cut reads one sequential array)
  std::vector<std::array<uintptr_t, kClasses>> dspan;
  bool grow(size_t n, bool with_val) {
    if (cap_idx < n) {
      pidx.reset(new (std::nothrow) uint32_t[n]);
      cap_idx = pidx ? n : 0;
      if (!pidx) return false;
    }
    if (with_val && cap_val < n) {
      pval.reset(new (std::nothrow) uint32_t[n]);
      cap_val = pval ? n : 0;
      if (!pval) return false;
    }
    return true;
  }
};

void pipe_workspace_free(PipeWorkspace* w) { delete w; }

// The staging layout of one chunk (runtime_internal.h BulkLayout): the
// pipeline writes it, the bulk lane copies and launches on it.
void BulkLayout::compute() {
  auto up = [](size_t x) { return (x + 255) / 256 * 256; };
  if (direct) {
    // host part: templates, their bytes, descriptors; the rest device-only
    o_tmpl = 0;
    o_blob = up(n_tmpls * sizeof(SbTemplate));
    o_desc = up(o_blob + blob_len + 16);
    in_bytes = up(o_desc + n_tmpls * sizeof(BulkDesc));
    o_key = in_bytes;
    o_sig = up(o_key + 4 * m);
    o_off = up(o_sig + 64 * m);
    o_tidx = up(o_off + 4 * (m + 1));
    o_flag = up(o_tidx + 4 * m);
    o_sec = up(o_flag + m);
    o_nanos = up(o_sec + 8 * m);
    o_cbase = up(o_nanos + 4 * m);  // ctot, then cbase: n_tmpls words each
    o_arena = up(o_cbase + 8 * n_tmpls);
    o_msg = up(o_arena + arena_bytes);
    dev_bytes = up(o_msg + msg_bytes + 16);
    return;
  }
  o_key = 0;
  o_sig = up(keyed ? 4 * m : 32 * m);
  o_off = up(o_sig + 64 * m);
  o_tidx = up(o_off + 4 * (m + 1));
  o_flag = up(o_tidx + 4 * m);
  o_sec = up(o_flag + m);
  o_nanos = up(o_sec + 8 * m);
  o_tmpl = up(o_nanos + 4 * m);
  o_blob = up(o_tmpl + n_tmpls * sizeof(SbTemplate));
  in_bytes = up(o_blob + blob_len + 16);
  o_msg = in_bytes;  // device only: k_sign_bytes writes the messages here
  dev_bytes = up(o_msg + msg_bytes + 16);
}

bool pipeline_wanted(const cmtv_ctx* ctx, uint64_t n_sigs) {
  const PipeConfig pc = pipe_config(ctx);
  if (!pc.enabled || n_sigs < pc.min_sigs || cache_enabled(ctx)) return false;
  const char* v = std::getenv("CMTV_HOST_SIGNBYTES");  // host-encoded sign-bytes: one-batch path only
  return !(v && v[0] == '1');
}

namespace {

// The context lock re-taken for one step of the pipeline (bulk_relock: a
// waiting latency call goes first), released at scope end.
struct Relock {
  std::unique_lock<std::mutex>& lk;
  Relock(cmtv_ctx* c, std::unique_lock<std::mutex>& l) : lk(l) { bulk_relock(c, lk); }
  ~Relock() { lk.unlock(); }
  Relock(const Relock&) = delete;
  Relock& operator=(const Relock&) = delete;
};

// What plan_direct keeps per distinct validator set of a call (the call's id
// keeps a set freed and reallocated at the same address between calls from
// hitting): whether its keys are packed, its total power, and --
// VerifyCommitLight -- the prefix an all-Commit commit of it reaches (the
// plan then depends on the set alone).
struct SetInfo {
  const cmtv_valset* v = nullptr;
  uint64_t call = 0;
  bool packed = false;
  int64_t total = 0;
  uint32_t light_m = 0;
  int64_t light_tally = 0;
};

// What one scan of cut_chunk found: the chunk's commits and totals.
struct Scan {
  static constexpr long kUnset = -2;
  size_t c1 = 0;                    // its commits end here
  uint64_t s = 0, mb = 0, tb = 0;   // planned signatures, sign-bytes, template bytes
  const cmtv_valset* vs = nullptr;  // key class: the set of its packed keys, or null
  // direct class: the pinned block of a direct chunk's commits, -1 for a
  // packed chunk (a chunk is one or the other), kUnset: nothing planned
  long dcls = kUnset;
  SpanAcc acc;  // the extents of its direct commits (a per-commit-capped scan)
  bool direct() const { return dcls >= 0; }
};

// A packed chunk's columns in its slot's pinned staging (BulkLayout offsets).
struct Staging {
  uint32_t* kidx;  // keyed: validator indices; else pk, the keys themselves
  uint8_t *pk, *sg;
  uint32_t *off, *tidx;
  uint8_t* flag;
  int64_t* sec;
  int32_t* nanos;
  SbTemplate* tmpls;
  uint8_t* blob;
  Staging(uint8_t* h, const BulkLayout& L)
      : kidx(reinterpret_cast<uint32_t*>(h + L.o_key)),
        pk(h + L.o_key),
        sg(h + L.o_sig),
        off(reinterpret_cast<uint32_t*>(h + L.o_off)),
        tidx(reinterpret_cast<uint32_t*>(h + L.o_tidx)),
        flag(h + L.o_flag),
        sec(reinterpret_cast<int64_t*>(h + L.o_sec)),
        nanos(reinterpret_cast<int32_t*>(h + L.o_nanos)),
        tmpls(reinterpret_cast<SbTemplate*>(h + L.o_tmpl)),
        blob(h + L.o_blob) {}
};

// One planned commit of a packed chunk, as its pack loops need it.
struct PackItem {
  const cmtv_commit* cm;
  const cmtv_valset* vals;
  const uint32_t *pi, *pv;  // its plan: commit and validator indices
  size_t m, i0;             // the plan's length; its first signature in the chunk
  uint64_t mo;              // its first sign-byte in the chunk
  uint32_t tl;              // its template in the chunk
  TplLens tlz;
  bool keyed;
};

// The common case, column by column: a contiguous plan whose validators are
// the commit's indices and whose signatures are all 64 bytes, back to back.
// (Staging by value: the byte stores below cannot alias the caller's copy.)
inline void pack_run(const Staging st, const PackItem& it) {
  const cmtv_commit* cm = it.cm;
  const cmtv_valset* vals = it.vals;
  const size_t m = it.m, i0 = it.i0;
  const uint32_t a = it.pi[0], tl = it.tl;
  nt_copy(st.sg + 64 * i0, cm->sigs + cm->sig_off[a], 64 * m);
  nt_copy(reinterpret_cast<uint8_t*>(st.sec + i0), reinterpret_cast<const uint8_t*>(cm->ts_seconds + a), 8 * m);
  nt_copy(reinterpret_cast<uint8_t*>(st.nanos + i0), reinterpret_cast<const uint8_t*>(cm->ts_nanos + a), 4 * m);
  const uint8_t* fl = cm->flags + a;
  for (size_t k = 0; k < m; k++) st.flag[i0 + k] = fl[k] == kFlagCommit;
  for (size_t k = 0; k < m; k++) st.tidx[i0 + k] = tl;
  if (it.keyed) {
    for (size_t k = 0; k < m; k++) st.kidx[i0 + k] = a + (uint32_t)k;
  } else if (vals->pk_off[a + m] - vals->pk_off[a] == 32 * m) {
    std::memcpy(st.pk + 32 * i0, vals->pubkeys + vals->pk_off[a], 32 * m);  // planned keys are 32 bytes
  } else {
    for (size_t k = 0; k < m; k++) std::memcpy(st.pk + 32 * (i0 + k), vals->pubkeys + vals->pk_off[a + k], 32);
  }
  const int64_t* se = cm->ts_seconds + a;
  const int32_t* na = cm->ts_nanos + a;
  uint64_t mo = it.mo;
  for (size_t k = 0; k < m; k++) {
    st.off[i0 + k] = (uint32_t)mo;
    mo += msg_len(it.tlz, fl[k] == kFlagCommit, se[k], na[k]);
  }
}

// Any plan, one signature at a time.
inline void pack_general(const Staging st, const PackItem& it) {
  const cmtv_commit* cm = it.cm;
  const cmtv_valset* vals = it.vals;
  uint64_t mo = it.mo;
  for (size_t k = 0; k < it.m; k++) {
    const size_t i = it.i0 + k;
    const uint32_t idx = it.pi[k], vi = it.pv[k];
    if (it.keyed)
      st.kidx[i] = vi;
    else
      std::memcpy(st.pk + 32 * i, vals->pubkeys + vals->pk_off[vi], 32);
    const uint32_t s0 = cm->sig_off[idx];
    if (cm->sig_off[idx + 1] - s0 == 64)
      std::memcpy(st.sg + 64 * i, cm->sigs + s0, 64);
    else
      std::memset(st.sg + 64 * i, 0, 64);  // invalid whatever the device says (job_replay)
    const bool fb = cm->flags[idx] == kFlagCommit;
    const int64_t se = cm->ts_seconds[idx];
    const int32_t na = cm->ts_nanos[idx];
    st.flag[i] = fb ? 1 : 0;
    st.sec[i] = se;
    st.nanos[i] = na;
    st.tidx[i] = it.tl;
    st.off[i] = (uint32_t)mo;
    mo += msg_len(it.tlz, fb, se, na);
  }
}

// One cmtv_verify_commits call through the pipeline: its state, and one
// member per stage. The caller holds the bulk lock throughout; the context
// lock is taken by the members that say so and never held across
// pool.parallel_for, bulk_stage, pack or (split_submit) bulk_prepare.
class PipeRun {
 public:
  PipeRun(cmtv_ctx* ctx, const CommitsArgs& args, int* rcs, std::vector<const cmtv_keyset*>& pinned)
      : ctx(ctx),
        args(args),
        rcs(rcs),
        n(args.n),
        trusting(args.kind == CMTV_VERIFY_COMMIT_LIGHT_TRUSTING),
        pc(pipe_config(ctx)),
        pool(host_pool(ctx)),
        pinned(pinned) {}
  // The workspace sized for the call, the address indices, the snapshot of
  // devices and pinned blocks. Takes the context lock for the snapshot.
  int init();
  // The attempt / retry loop and the phase flush. Takes the context lock
  // after a failure and for the flush.
  int run();

 private:
  // ---- call state: set by init, constant over the call unless noted
  cmtv_ctx* const ctx;
  const CommitsArgs& args;
  int* const rcs;
  const size_t n;
  const bool trusting;
  const PipeConfig pc;
  HostPool& pool;
  // the registered key sets pinned so far: the caller's, which unpins them
  // (also after an exception)
  std::vector<const cmtv_keyset*>& pinned;
  // per-call arrays in the context's workspace: reused across calls, so a
  // pass over 15M signatures does not fault in 100+ MB of fresh pages
  PipeWorkspace* W = nullptr;
  uint64_t call_id = 0;
  // LightTrusting: one address index per distinct (address array, size)
  std::map<std::pair<const uint8_t*, uint32_t>, AddrIndex> addr_index;
  bool keyed_mode = false;
  // direct chunks (BulkLayout): on when the caller's arguments can be in
  // pinned blocks of this context and the registered-key cache is on
  std::vector<PinnedRange> pins;
  bool direct_on = false;
  std::vector<size_t> live;  // refreshed after a device is retired
  // the context lock, held only inside a Relock scope
  std::unique_lock<std::mutex> lk;
  // the phase clock, flushed to the context once at the end of run
  struct {
    uint64_t plan = 0, cut = 0, pack = 0, submit = 0, wait = 0, replay = 0;
  } ph;

  // ---- cutter state: chunks are cut on the fly, commit-aligned, about
  // `per` planned signatures each (at least the kernels' full-rate size,
  // pc.chunk, and at least two per device when the call is large enough to
  // split), one key class per chunk when the keyset cache can serve it
  std::vector<Chunk> chunks;
  size_t cursor = 0;        // next commit to put in a chunk
  size_t planned_upto = 0;  // commits [0, planned_upto) are planned
  uint64_t per = 0;         // 0: not sized yet (size_chunks)
  bool ramp = false;
  const cmtv_valset* last_vs = nullptr;  // the scan's last set and whether
  bool last_packed = false;              // its keys are packed
  const uint64_t max_mb = max_batch_msg_bytes();

  // ---- attempt state, reset by each pass of the retry loop ...
  std::deque<size_t> inflight;  // chunks submitted (or empty), not yet replayed
  size_t rr = 0;                // round-robin count over (device, slot)
  long bad_dev = -1;            // the device whose error ended the attempt
  // ... and what survives it: chunks are replayed in submission (= chunk)
  // order, so the replayed ones are exactly [0, retired)
  size_t retired = 0;

  // a commit's job as the plan needs it, and with its preamble's outcome
  // restored once planned
  CommitJob job(size_t c) const {
    CommitJob J = args.job(c);
    if (trusting) J.addr = W->addr[c];
    return J;
  }
  CommitJob planned_job(size_t c) const {
    CommitJob J = job(c);
    J.early = W->early[c];
    J.needed = W->needed[c];
    return J;
  }
  uint32_t* plan_idx(size_t c) const { return W->pidx.get() + W->base[c]; }
  uint32_t* plan_val(size_t c) const { return trusting ? W->pval.get() + W->base[c] : nullptr; }

  // The stages. Each is entered with the context lock free and leaves it
  // free; the note says whether it takes the lock meanwhile ("workers": it
  // runs a parallel_for, or on a worker inside one, where the lock must be free).
  void plan_window(uint64_t want_sigs);                            // never; workers
  bool plan_direct(size_t c, const CommitJob& J);                  // never; workers
  const SetInfo& set_info(const CommitJob& J) const;               // never; workers
  long pinned_block(const uintptr_t* a, const size_t* len) const;  // never; workers (pins is a snapshot)
  int cut_chunk();                                                 // in pin_keyset only
  void size_chunks();                                              // never; workers
  Scan scan(uint64_t want, bool per_commit_cap);                   // never; workers
  void pin_keyset(Chunk& ch);                                      // takes it: keyset_for / keyset_pin
  void demote(Chunk& ch);                                          // never; workers
  void layout_spans(Chunk& ch) const;                              // never
  void pack(const Chunk& ch, uint8_t* h);                          // never; workers
  void pack_direct(const Chunk& ch, uint8_t* h);                   // never; workers
  int submit(Chunk& ch);                                           // takes it for the launch, after the pack
  void replay(const Chunk& ch, const uint64_t* bm);                // never; workers
  int retire(size_t c);                                            // takes it for the invalid count, after the replay
  int retire_until(size_t keep);                                   // as retire
  int attempt();                                                   // as cut_chunk, submit, retire
};

int PipeRun::init() {
  PipeWorkspace*& wsp = pipe_workspace(ctx);
  if (!wsp) wsp = new (std::nothrow) PipeWorkspace();
  if (!wsp) return CMTV_ENOMEM;
  W = wsp;
  W->base.resize(n + 1);
  W->base[0] = 0;
  for (size_t c = 0; c < n; c++) W->base[c + 1] = W->base[c] + args.commits[c].n_sigs;
  if (!W->grow(W->base[n] + 1, trusting)) return CMTV_ENOMEM;
  W->plen.resize(n);
  W->tlen.resize(n);
  W->mbytes.resize(n);
  W->early.resize(n);
  W->needed.resize(n);
  W->direct.resize(n);
  W->ptally.resize(n);
  W->pblock.resize(n);
  W->dspan.resize(n);
  W->sp.resize(n);
  W->mp.resize(n);
  W->tp.resize(n);
  static std::atomic<uint64_t> calls{0};
  call_id = ++calls;
  if (trusting) {
    W->addr.resize(n);
    const AddrIndex* last = nullptr;
    std::pair<const uint8_t*, uint32_t> last_key{nullptr, 0};
    for (size_t c = 0; c < n; c++) {
      const cmtv_valset& v = args.vals[c];
      const auto key = std::make_pair(v.addrs, v.n_vals);
      if (!last || key != last_key) {
        auto it = addr_index.find(key);
        if (it == addr_index.end()) {
          it = addr_index.emplace(key, AddrIndex()).first;
          it->second.build(v.addrs, v.n_vals);
        }
        last = &it->second;
        last_key = key;
      }
      W->addr[c] = last;
    }
  }
  const int rc = ctx_lock(ctx, lk);
  if (rc != CMTV_OK) return rc;
  keyed_mode = keyset_cache_enabled(ctx);
  live_devices_locked(ctx, live);
  pinned_ranges_locked(ctx, pins);
  direct_on = pc.direct && keyed_mode && !trusting && !pins.empty();
  lk.unlock();
  return CMTV_OK;
}

// ---- plan: each commit's preamble and plan, its template and sign-bytes
// lengths -- window by window (about want_sigs signatures from
// planned_upto), just ahead of the chunk being cut, so the planning of
// later commits overlaps the device's work on earlier chunks
void PipeRun::plan_window(uint64_t want_sigs) {
  const uint64_t t0 = now_ns();
  size_t b = planned_upto;
  while (b < n && W->base[b] - W->base[planned_upto] < want_sigs) b++;
  if (b == planned_upto) b++;
  const size_t a = planned_upto;
  pool.parallel_for(b - a, 64, [this, a](size_t lo, size_t hi) {
    thread_local Seen seen;
    // each distinct validator set's total power once (job_preamble)
    const cmtv_valset* tot_vs = nullptr;
    int64_t tot = 0;
    for (size_t c = a + lo; c < a + hi; c++) {
      CommitJob J = job(c);
      if (!tot_vs || !same_arrays(J.vals, tot_vs)) {
        tot_vs = J.vals;
        tot = 0;
        for (uint32_t i = 0; i < tot_vs->n_vals; i++) tot += tot_vs->voting_power[i];
      }
      J.has_total = true;
      J.total = tot;
      job_preamble(J);
      W->early[c] = J.early;
      W->needed[c] = J.needed;
      W->direct[c] = 0;
      W->plen[c] = W->tlen[c] = 0;
      W->mbytes[c] = 0;
      if (J.early != 1) continue;
      if (direct_on && plan_direct(c, J)) continue;
      uint32_t* pi = plan_idx(c);
      const size_t m = job_plan(J, pi, plan_val(c), seen);
      W->plen[c] = (uint32_t)m;
      if (!m) continue;
      TplLens tl;
      W->tlen[c] = (uint32_t)commit_template_lens(J.chain_id_len, J.commit, &tl.pre_commit, &tl.pre_nil, &tl.post);
      W->mbytes[c] = exact_mbytes(J.commit, pi, m, tl);
    }
  });
  planned_upto = b;
  ph.plan += now_ns() - t0;
}

// This thread's SetInfo of J's validator set (J past its preamble: J.total
// is the set's power as plan_window summed it, J.needed its 2/3).
const SetInfo& PipeRun::set_info(const CommitJob& J) const {
  const cmtv_valset* v = J.vals;
  thread_local SetInfo si;
  if (!si.v || si.call != call_id || !same_arrays(v, si.v)) {
    si.v = v;
    si.call = call_id;
    si.packed = packed_keys(v);
    si.total = J.total;
    int64_t t = 0;
    uint32_t m = 0;
    for (uint32_t i = 0; i < v->n_vals; i++) {
      t += v->voting_power[i];
      m = i + 1;
      if (t > J.needed) break;
    }
    si.light_m = m;
    si.light_tally = t;
  }
  return si;
}

// The one pinned block holding all four classes [a[k], a[k] + len[k]), or -1
// (this thread's last block first).
long PipeRun::pinned_block(const uintptr_t* a, const size_t* len) const {
  thread_local long hint = -1;
  long blk = -1;
  for (int k = 0; k < kClasses; k++) {
    const PinnedRange* h = hint >= 0 && (size_t)hint < pins.size() ? &pins[(size_t)hint] : nullptr;
    long b;
    if (h && a[k] >= h->base && a[k] + len[k] >= a[k] && a[k] + len[k] <= h->base + h->bytes)
      b = hint;
    else
      b = hint = find_block(pins, reinterpret_cast<const void*>(a[k]), len[k]);
    if (b < 0 || (blk >= 0 && b != blk)) return -1;
    blk = b;
  }
  return blk;
}

// A direct commit (BulkLayout): its plan is its signatures [0, m) --
// VerifyCommit: every flag Commit or Nil; VerifyCommitLight: Commit flags
// up to the +2/3 threshold -- from a set of packed 32-byte keys, 64-byte
// signatures back to back, and its four arrays aligned and inside ONE of the
// caller's pinned blocks. Nothing per signature is then packed on the host:
// the plan costs one pass over the flags (and powers) and the signature
// offsets. Sets plen, tlen, mbytes (an upper bound: every message at its
// template's longest) and the direct fields; false: the general plan.
bool PipeRun::plan_direct(size_t c, const CommitJob& J) {
  const cmtv_commit* cm = J.commit;
  const cmtv_valset* v = J.vals;
  const uint32_t n_s = cm->n_sigs;
  if (n_s != v->n_vals) return false;
  const SetInfo& si = set_info(J);
  if (!si.packed) return false;
  const uint8_t* fl = cm->flags;
  int64_t tally = 0;
  uint32_t m = 0;
  if (J.kind == CMTV_VERIFY_COMMIT) {
    m = n_s;
    if (all_commit(fl, n_s)) {
      tally = si.total;
    } else {
      const int64_t* vp = v->voting_power;
      uint32_t bad = 0;
      for (uint32_t i = 0; i < n_s; i++) {  // branch-free: the compiler vectorises it
        const uint8_t f = fl[i];
        const bool fb = f == kFlagCommit;
        bad |= (uint32_t)(!fb & (f != kFlagNil));
        tally += fb ? vp[i] : 0;
      }
      if (bad) return false;
    }
  } else {
    // J.needed is the set's (total * 2 / 3, as when si was filled)
    m = si.light_m;
    tally = si.light_tally;
    if (!all_commit(fl, m)) return false;
  }
  uint32_t blk = UINT32_MAX;
  if (m) {
    const uint32_t* so = cm->sig_off;
    const uint32_t s0 = so[0];
    if ((uint64_t)s0 + 64ull * m > UINT32_MAX) return false;
    uint32_t bad = 0;
    for (uint32_t i = 1; i <= m; i++) bad |= so[i] ^ (s0 + 64u * i);  // vectorised
    if (bad) return false;
    uintptr_t* a = W->dspan[c].data();
    size_t len[kClasses];
    SpanAcc::ranges(cm, m, a, len);
    if ((a[kClsSig] & 7) || (a[kClsSec] & 7) || (a[kClsNanos] & 3)) return false;
    const long b = pinned_block(a, len);
    if (b < 0) return false;
    blk = (uint32_t)b;
    TplLens tl;
    W->tlen[c] = (uint32_t)commit_template_lens(J.chain_id_len, cm, &tl.pre_commit, &tl.pre_nil, &tl.post);
    W->mbytes[c] = (uint64_t)m * msg_len_bound(tl);
  }
  W->plen[c] = m;
  W->direct[c] = 1;
  W->ptally[c] = tally;
  W->pblock[c] = blk;
  return true;
}

// ---- cut: the first window sets the chunk size from its plan ratio
void PipeRun::size_chunks() {
  plan_window(std::max<uint64_t>(pc.chunk, 1));
  const uint64_t ws = W->base[planned_upto];
  uint64_t wp = 0;
  for (size_t c = 0; c < planned_upto; c++) wp += W->plen[c];
  const uint64_t est = ws ? (uint64_t)((double)W->base[n] * ((double)wp / (double)ws)) : 0;
  uint64_t nc = std::max<uint64_t>(1, est / pc.chunk);
  const uint64_t spread = std::min<uint64_t>(2 * live.size(), est / std::max<size_t>(pc.min_sigs, 1));
  nc = std::max(nc, spread);
  per = std::max<uint64_t>(1, (est + nc - 1) / nc);
  const bool long_call = est / pc.chunk >= 4;
  // a long call runs chunks of pc.chunk planned signatures at most (the
  // default, 2^20, is one full round of the batched registered-key lane
  // kernel: 2,048 waves of 64 lanes x 8 signatures; a chunk just past it
  // would start a second, nearly empty round), and ramps up: its first
  // chunks are 1/16, 1/4 and 1/2 of that, so the device starts after a
  // fraction of a chunk's pack instead of a whole one
  if (long_call) {
    ramp = true;
    per = pc.chunk;
  }
}

// The commits of the chunk that starts at cursor, about `want` planned
// signatures; with per_commit_cap a direct chunk also ends where its DMA
// extents outgrow its plans. The common case runs without it and checks the
// extents once, for the whole chunk, from the plan's per-commit class starts
// (W->dspan, cut_chunk); only a chunk that fails that check is cut again
// commit by commit (round 6: the per-commit extents were ~40% of the serial
// cut, tests/host/pipebench's pipe_cut phase). Plans ahead as it goes and
// writes the commits' chunk-local offsets (sp, mp, tp).
Scan PipeRun::scan(uint64_t want, bool per_commit_cap) {
  Scan r;
  bool cls_set = false;
  uint64_t s = 0, mb = 0, tb = 0;
  size_t c = cursor;
  for (; c < n; c++) {
    // plan a chunk's worth at a time: each window is one parallel_for (a
    // wake-up of every worker), so windows of 64k signatures cost ~230
    // wake-ups per 15M-signature call
    if (c == planned_upto)
      plan_window(std::max<uint64_t>(want - std::min(want, s), std::max<uint64_t>(pc.chunk, 65536)));
    const uint32_t pl = W->plen[c];
    const bool dir = pl && W->direct[c];
    if (pl) {
      const long dc = dir ? (long)W->pblock[c] : -1;
      if (r.dcls != Scan::kUnset && dc != r.dcls) break;
      r.dcls = dc;
    }
    if (pl && keyed_mode) {
      const cmtv_valset* v = &args.vals[c];
      if (!last_vs || !same_arrays(v, last_vs)) {
        last_vs = v;
        last_packed = packed_keys(v);
      }
      const cmtv_valset* cls = last_packed ? v : nullptr;
      if (cls_set &&
          !((cls == nullptr) == (r.vs == nullptr) && (!cls || same_arrays(r.vs, cls) || same_keys(r.vs, cls))))
        break;
      if (!cls_set) {
        r.vs = cls;
        cls_set = true;
      }
    }
    // cut below the target (a commit that would cross it opens the next
    // chunk), unless the chunk would be empty
    if (s && s + pl > want) break;
    // ... and below the one-batch path's sign-bytes span per launch (its
    // message offsets are 32-bit): a commit that would cross it opens the
    // next chunk
    if (s && mb + W->mbytes[c] >= max_mb) break;
    W->sp[c] = s;
    W->mp[c] = mb;
    W->tp[c] = tb;
    s += pl;
    mb += W->mbytes[c];
    tb += W->tlen[c];
    if (dir && per_commit_cap) r.acc.add(W->dspan[c].data(), pl);
    // a direct chunk's DMA covers its classes' extents: it ends at a commit
    // past which it would copy far more than its plans read
    if (s >= want || (dir && per_commit_cap && r.acc.over(pc))) {
      c++;
      break;
    }
  }
  r.c1 = c;
  r.s = s;
  r.mb = mb;
  r.tb = tb;
  return r;
}

// The chunk's registered key set, pinned for the call. Takes the context lock.
void PipeRun::pin_keyset(Chunk& ch) {
  Relock g(ctx, lk);
  ch.ks = keyset_for_locked(ctx, ch.vs->pubkeys, ch.vs->n_vals);
  if (ch.ks && std::find(pinned.begin(), pinned.end(), ch.ks) == pinned.end()) {
    keyset_pin_locked(ch.ks);
    pinned.push_back(ch.ks);
  }
}

// A direct chunk without a registered key set (registration failed) is
// packed after all: the same prefix plans, written out, with exact sign-bytes.
void PipeRun::demote(Chunk& ch) {
  pool.parallel_for(ch.c1 - ch.c0, 64, [this, &ch](size_t lo, size_t hi) {
    thread_local Seen seen;
    for (size_t k = ch.c0 + lo; k < ch.c0 + hi; k++) {
      if (!W->direct[k]) continue;
      W->direct[k] = 0;
      if (!W->plen[k]) continue;
      const CommitJob J = planned_job(k);
      uint32_t* pi = plan_idx(k);
      (void)job_plan(J, pi, nullptr, seen);  // == the prefix [0, plen)
      SbTemplate tpl;
      put_commit_template(nullptr, 0, J.chain_id, J.chain_id_len, J.commit, &tpl);
      W->mbytes[k] =
          exact_mbytes(J.commit, pi, W->plen[k], TplLens{tpl.pre_commit_len, tpl.pre_nil_len, tpl.post_len});
    }
  });
  uint64_t x = 0;
  for (size_t k = ch.c0; k < ch.c1; k++) {
    W->mp[k] = x;
    x += W->mbytes[k];
  }
  ch.L.msg_bytes = x;
  ch.direct = false;
}

// A direct chunk's DMA spans: the classes' extents, merged, each landing at
// a device offset congruent to its host address mod 256 (so the caller's
// 8-byte alignment holds on the device).
void PipeRun::layout_spans(Chunk& ch) const {
  uintptr_t slo[kClasses], shi[kClasses];
  int cs[kClasses];
  const int ns = ch.acc.merge(slo, shi, cs);
  size_t at = 0;
  for (int j = 0; j < ns; j++) {
    at = (at + 255) / 256 * 256 + (slo[j] & 255);
    ch.L.spans[j] = BulkSpan{reinterpret_cast<const uint8_t*>(slo[j]), (size_t)(shi[j] - slo[j]), at};
    at += shi[j] - slo[j];
  }
  ch.L.n_spans = ns;
  ch.L.arena_bytes = at;
  for (int k = 0; k < kClasses; k++) {
    ch.cls_lo[k] = ch.acc.lo[k];
    ch.cls_dev[k] = cs[k] < 0 ? 0 : ch.L.spans[cs[k]].dev_off + (ch.acc.lo[k] - slo[cs[k]]);
  }
  ch.L.direct = true;
}

// Appends the next chunk; CMTV_OK or an error.
int PipeRun::cut_chunk() {
  struct CutClock {  // ph.cut: this cut's time, its plan windows apart
    uint64_t &cut, &plan, t0, plan0;
    ~CutClock() { cut += (now_ns() - t0) - (plan - plan0); }
  } cut_clock{ph.cut, ph.plan, now_ns(), ph.plan};
  if (per == 0) size_chunks();
  uint64_t want = per;
  // the ramp: 1/16, 1/4, 1/2 of a chunk (2^16 signatures take the one-
  // signature-per-lane keyed kernel at two waves per SIMD, 2^18 and 2^19
  // the KB = 4 batch); measured on MI355X (tools/ramp_ab.sh, 100k x 150,
  // two alternating rounds): 40.9-41.1 ms per pass against 41.3-41.6 with
  // 1/8, 1/4, 1/2 and 42.3 without a ramp
  static constexpr int ramp_sh[] = {4, 2, 1};
  if (ramp && chunks.size() < 3) want = std::max<uint64_t>(per >> ramp_sh[chunks.size()], 1);
  Chunk ch;
  ch.c0 = cursor;
  // near a latency call the chunk runs on the CU-masked lane: no more than
  // one round of the CUs it keeps
  ch.L.masked = latency_recent(ctx);
  if (ch.L.masked) want = std::min<uint64_t>(want, pc.chunk_masked);
  Scan sc = scan(want, false);
  if (sc.direct()) {
    // a direct chunk (every planned commit of it direct): its extents
    for (size_t k = cursor; k < sc.c1; k++)
      if (W->plen[k]) sc.acc.add(W->dspan[k].data(), W->plen[k]);
    if (sc.acc.over(pc)) sc = scan(want, true);
  }
  ch.c1 = cursor = sc.c1;
  ch.vs = sc.vs;
  ch.acc = sc.acc;
  ch.L.m = sc.s;
  ch.L.n_tmpls = ch.c1 - ch.c0;
  ch.L.blob_len = sc.tb;
  ch.L.msg_bytes = sc.mb;
  if (sc.mb >= max_mb) return CMTV_EINVAL;  // one commit's sign-bytes alone reach the span
  if (keyed_mode && ch.vs && ch.L.m) pin_keyset(ch);
  ch.L.keyed = ch.ks != nullptr;
  ch.direct = sc.direct() && ch.L.m;
  if (ch.direct && !ch.ks) demote(ch);
  if (ch.direct) layout_spans(ch);
  ch.L.compute();
  chunks.push_back(ch);
  return CMTV_OK;
}

// ---- pack. A direct chunk's host part: each commit's template and descriptor
void PipeRun::pack_direct(const Chunk& ch, uint8_t* h) {
  const BulkLayout& L = ch.L;
  auto* tmpls = reinterpret_cast<SbTemplate*>(h + L.o_tmpl);
  uint8_t* blob = h + L.o_blob;
  auto* desc = reinterpret_cast<BulkDesc*>(h + L.o_desc);
  pool.parallel_for(ch.c1 - ch.c0, 64, [this, &ch, tmpls, blob, desc](size_t b, size_t e) {
    for (size_t c = ch.c0 + b; c < ch.c0 + e; c++) {
      const size_t tl = c - ch.c0;
      const uint32_t m = W->plen[c];
      if (!m) {
        tmpls[tl] = SbTemplate{};
        desc[tl] = BulkDesc{};
        continue;
      }
      const cmtv_commit* cm = &args.commits[c];
      put_commit_template(blob, W->tp[c], args.chain_id, args.chain_id_len, cm, &tmpls[tl]);
      uintptr_t a[kClasses];
      size_t len[kClasses];
      SpanAcc::ranges(cm, m, a, len);
      BulkDesc d;
      d.sig = ch.cls_dev[kClsSig] + (a[kClsSig] - ch.cls_lo[kClsSig]);
      d.sec = ch.cls_dev[kClsSec] + (a[kClsSec] - ch.cls_lo[kClsSec]);
      d.nanos = ch.cls_dev[kClsNanos] + (a[kClsNanos] - ch.cls_lo[kClsNanos]);
      d.flags = ch.cls_dev[kClsFlags] + (a[kClsFlags] - ch.cls_lo[kClsFlags]);
      d.sp = (uint32_t)W->sp[c];
      d.m = m;
      desc[tl] = d;
    }
  });
}

// A chunk into its slot's pinned staging h (bulk_stage).
void PipeRun::pack(const Chunk& ch, uint8_t* h) {
  if (ch.direct) return pack_direct(ch, h);
  const BulkLayout& L = ch.L;
  const Staging st(h, L);
  pool.parallel_for(ch.c1 - ch.c0, 16, [this, &ch, st](size_t b, size_t e) {
    for (size_t c = ch.c0 + b; c < ch.c0 + e; c++) {
      const size_t m = W->plen[c];
      if (!m) continue;
      const cmtv_commit* cm = &args.commits[c];
      const uint32_t tl = (uint32_t)(c - ch.c0);
      SbTemplate t;
      put_commit_template(st.blob, W->tp[c], args.chain_id, args.chain_id_len, cm, &t);
      st.tmpls[tl] = t;
      const uint32_t* pi = plan_idx(c);
      const TplLens tlz{t.pre_commit_len, t.pre_nil_len, t.post_len};
      const PackItem it{cm, &args.vals[c], pi, trusting ? plan_val(c) : pi, m, W->sp[c], W->mp[c], tl, tlz, ch.L.keyed};
      const uint32_t a = pi[0];
      bool run = !trusting && pi[m - 1] - a == m - 1 && cm->sig_off[a + m] - cm->sig_off[a] == 64 * m;
      for (size_t k = 0; run && k < m; k++) run = cm->sig_off[a + k + 1] - cm->sig_off[a + k] == 64;
      if (run)
        pack_run(st, it);
      else
        pack_general(st, it);
    }
    nt_fence();  // this block's streaming stores are visible before the H2D reads them
  });
  st.off[L.m] = (uint32_t)L.msg_bytes;
}

// ---- submit: a chunk with signatures onto the next (device, slot): stage,
// pack, prepare, launch. Takes the context lock for the launch only.
int PipeRun::submit(Chunk& ch) {
  const size_t G = live.size(), S = (size_t)pc.slots;
  ch.dev = live[rr % G];
  ch.slot = (int)((rr / G) % S);
  rr++;
  uint8_t* h = nullptr;
  const uint64_t tk = now_ns();
  int rc = bulk_stage(ctx, ch.dev, ch.slot, ch.L, &h);
  if (rc != CMTV_OK) return rc;
  pack(ch, h);
  const uint64_t ts = now_ns();
  ph.pack += ts - tk;
  // the lane-only part first, outside the context lock (a latency call
  // on the context never waits behind it), then the launch under it
  if (pc.split_submit) rc = bulk_prepare(ctx, ch.dev, ch.slot, ch.L, ch.ks);
  if (rc == CMTV_OK) {
    Relock g(ctx, lk);
    if (!pc.split_submit) rc = bulk_prepare(ctx, ch.dev, ch.slot, ch.L, ch.ks);
    if (rc == CMTV_OK) rc = bulk_submit_locked(ctx, ch.dev, ch.slot, ch.L, ch.ks, args.mode);
    if (rc == CMTV_OK && ch.direct) count_direct_locked(ctx);
  }
  ph.submit += now_ns() - ts;
  return rc;
}

// ---- replay: every commit of the chunk over its verdict bits bm
void PipeRun::replay(const Chunk& ch, const uint64_t* bm) {
  pool.parallel_for(ch.c1 - ch.c0, 32, [this, &ch, bm](size_t b, size_t e) {
    thread_local Seen seen;
    for (size_t c = ch.c0 + b; c < ch.c0 + e; c++) {
      const size_t i0 = W->sp[c];
      CommitJob J = planned_job(c);
      if (W->direct[c]) {  // a prefix plan: its first invalid bit decides
        const size_t m = W->plen[c];
        rcs[c] = replay_prefix(J, m, W->ptally[c], m ? first_invalid(bm, i0, m) : 0);
        continue;
      }
      rcs[c] = job_replay(J, plan_idx(c), W->plen[c],
                          [bm, i0](size_t j) {
                            const size_t i = i0 + j;
                            return ((bm[i >> 6] >> (i & 63)) & 1) != 0;
                          },
                          seen);
    }
  });
}

// Chunk c, the oldest in flight: wait for its verdicts, replay it, count its
// invalid signatures (context lock taken for the count).
int PipeRun::retire(size_t c) {
  const Chunk& ch = chunks[c];
  const uint64_t* bm = nullptr;
  if (ch.L.m) {
    const uint64_t tw = now_ns();
    const int r = bulk_wait(ctx, ch.dev, ch.slot, &bm);
    ph.wait += now_ns() - tw;
    if (r != CMTV_OK) {
      bad_dev = (long)ch.dev;
      return r;
    }
  }
  const uint64_t tr = now_ns();
  replay(ch, bm);
  if (ch.L.m) {
    const uint64_t valid = count_valid(bm, ch.L.m);
    Relock g(ctx, lk);
    count_invalid_locked(ctx, ch.L.m - valid);
  }
  ph.replay += now_ns() - tr;
  retired = c + 1;  // chunks retire in order
  return CMTV_OK;
}

// Retires from the front of inflight until at most `keep` chunks are left.
int PipeRun::retire_until(size_t keep) {
  int rc = CMTV_OK;
  while (rc == CMTV_OK && inflight.size() > keep) {
    rc = retire(inflight.front());
    inflight.pop_front();
  }
  return rc;
}

// One pass over the chunks not yet replayed, cutting new ones as it goes:
// CMTV_OK when every commit is replayed, else the first error (bad_dev: the
// device it came from, if any).
int PipeRun::attempt() {
  const size_t slots = live.size() * (size_t)pc.slots;
  inflight.clear();
  rr = 0;
  bad_dev = -1;
  int rc = CMTV_OK;
  for (size_t c = retired; rc == CMTV_OK; c++) {
    if (c == chunks.size()) {
      if (cursor == n) break;
      if ((rc = cut_chunk()) != CMTV_OK) break;
    }
    if ((rc = retire_until(slots - 1)) != CMTV_OK) break;
    Chunk& ch = chunks[c];
    // (nothing to verify: replayed in order with the others)
    if (ch.L.m && (rc = submit(ch)) != CMTV_OK) {
      bad_dev = (long)ch.dev;
      break;
    }
    inflight.push_back(c);
  }
  return rc == CMTV_OK ? retire_until(0) : rc;
}

int PipeRun::run() {
  int rc;
  for (;;) {
    if (live.empty()) {
      rc = CMTV_ENODEV;
      break;
    }
    rc = attempt();
    if (rc == CMTV_OK) break;
    // a failure: nothing of this attempt stays in flight; a device's own HIP
    // error retires it and the chunks not yet replayed run on the others
    bulk_drain(ctx);
    Relock g(ctx, lk);
    if (rc != CMTV_EHIP || bad_dev < 0 || !retire_device_locked(ctx, (size_t)bad_dev)) break;
    live_devices_locked(ctx, live);
  }
  Relock g(ctx, lk);
  phase_add_ns(ctx, kPhPipePlan, ph.plan);
  phase_add_ns(ctx, kPhPipeCut, ph.cut);
  phase_add_ns(ctx, kPhPipePack, ph.pack);
  phase_add_ns(ctx, kPhPipeSubmit, ph.submit);
  phase_add_ns(ctx, kPhPipeWait, ph.wait);
  phase_add_ns(ctx, kPhPipeReplay, ph.replay);
  return rc;
}

}  // namespace

int verify_commits_pipeline(cmtv_ctx* ctx, const CommitsArgs& args, int* rcs) {
  std::unique_lock<std::mutex> bulk(bulk_mutex(ctx));
  const BulkBusy busy(ctx);
  // the registered key sets the call pins, released below (also after an
  // exception)
  std::vector<const cmtv_keyset*> pinned;
  pinned.reserve(8);
  int rc;
  bool threw = false;
  // no C++ exception crosses the C ABI: a failed allocation (std::bad_alloc)
  // or thread creation (std::system_error) is the call's error code, after
  // everything the call enqueued has drained
  try {
    PipeRun p(ctx, args, rcs, pinned);
    rc = p.init();
    if (rc == CMTV_OK) rc = p.run();
  } catch (const std::bad_alloc&) {
    rc = CMTV_ENOMEM;
    threw = true;
  } catch (...) {
    rc = CMTV_EINVAL;
    threw = true;
  }
  if (threw) bulk_drain(ctx);
  if (!pinned.empty()) {
    std::unique_lock<std::mutex> lk;
    (void)ctx_lock(ctx, lk);
    for (auto* ks : pinned) keyset_unpin_locked(ctx, ks);
  }
  return rc;
}

}  // namespace cmtv
