// runtime.cpp -- libcmtverify host runtime: a context's lifecycle (open,
// environment knobs, close), its lock, statistics, the caller's pinned
// blocks, key generation and signing, and the plain verification entry
// points of include/cmtverify.h. The rest of the runtime: launch.cpp (the
// kernel launchers), host_batch.cpp (host-buffer batches, the verdict
// cache), gather.cpp (sharding, RCCL), keyset.cpp (registered keys) and
// bulk_lane.cpp (the pipeline's lanes); runtime_state.h is their shared state.
//
// A context = one or more devices, each with its own HIP stream, fixed-base
// tables, growable device / pinned buffers and lane-kernel scratch. Calls on a
// context are serialised by its mutex and set the device they touch (cgo
// callers migrate threads). Host-buffer batches are split into contiguous
// 64-aligned shards, one per device, and the shards' verdict bitmaps are
// all-gathered over RCCL (xGMI) when the context has several devices
// (SURVEY.md 8e). There is no CPU verification path: if a device is unusable
// every call fails with a negative code and the caller decides what to do.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <thread>

#include "runtime_state.h"
// (after the HIP runtime's header)
#include "merlin.h"
#include "secp256k1_sign.h"

namespace cmtv {

uint64_t phase_now(const cmtv_ctx* ctx) { return phase_clock(ctx); }

void phase_add(cmtv_ctx* ctx, int phase, uint64_t t0) {
  if (!ctx->phases_on || !t0) return;
  ctx->phase_ns[phase] += phase_clock(ctx) - t0;
  if (phase == kPhPrepare) ctx->phase_calls++;
}

void phase_add_ns(cmtv_ctx* ctx, int phase, uint64_t ns) {
  if (!ctx->phases_on) return;
  ctx->phase_ns[phase] += ns;
  if (phase == kPhPipePlan) ctx->phase_calls++;
}

void harvest(cmtv_ctx* ctx, bool blocking) {
  for (auto& d : ctx->devs) {
    if (d.failed) continue;
    (void)hipSetDevice(d.ordinal);
    d.timing.harvest(ctx->stats, d.device_ms, d.timed_calls, blocking);
  }
}

// The single-device _device entry points run on devs[0] (their inputs are
// its memory): once it is retired they return CMTV_ENODEV rather than launch
// on a device that returned a HIP error. (Key generation and signing take
// host buffers and run on the first live device.)
// CMTV_FAULT_AT's failure belongs to that call only, so the flag that marks
// it is cleared with the call's result (run_host_batch and sharded_device
// clear it on their own paths).
template <class F>
static int on_dev0(cmtv_ctx* ctx, F&& call) {
  std::unique_lock<std::mutex> lk;
  if (ctx_lock(ctx, lk) != CMTV_OK) return CMTV_ENODEV;
  if (ctx->devs[0].failed) return CMTV_ENODEV;
  const int rc = call(ctx->devs[0]);
  ctx->fault_pending = false;
  return rc;
}

// The verify entry points' argument checks, in their order: the context,
// the mode and n's range; nothing more for an empty batch (the caller
// returns CMTV_OK for it before any pointer is looked at); then the
// pointers and, for host buffers, monotone message offsets.
static bool host_args_ok(const cmtv_ctx* ctx, uint32_t mode, size_t n, const void* keys, const uint8_t* sig,
                         const uint8_t* msg, const uint32_t* msg_off, const void* out_valid, const void* out_bitmap) {
  if (!ctx || mode > CMTV_MODE_ZIP215 || n > (1ull << 31)) return false;
  if (n == 0) return true;
  if (!keys || !sig || !msg_off || (!msg && msg_off[n] != 0) || (!out_valid && !out_bitmap)) return false;
  for (size_t i = 0; i < n; i++)
    if (msg_off[i + 1] < msg_off[i]) return false;
  return true;
}

static bool device_args_ok(const cmtv_ctx* ctx, uint32_t mode, size_t n, const void* d_keys, const void* d_sig,
                           const void* d_msg, const void* d_msg_off, const void* d_valid, const void* d_bitmap) {
  if (!ctx || mode > CMTV_MODE_ZIP215 || n > (1ull << 31)) return false;
  return n == 0 || (d_keys && d_sig && d_msg && d_msg_off && (d_valid || d_bitmap));
}

// A device-resident call's untyped arguments as the launchers take them
// (a null stream is the HIP null stream).
struct DeviceArgs {
  const uint8_t *keys, *sig, *msg;
  const uint32_t* off;
  uint8_t* valid;
  uint64_t* bitmap;
  hipStream_t s;
  DeviceArgs(const void* d_keys, const void* d_sig, const void* d_msg, const void* d_msg_off, void* d_valid,
             void* d_bitmap, void* stream)
      : keys(static_cast<const uint8_t*>(d_keys)), sig(static_cast<const uint8_t*>(d_sig)),
        msg(static_cast<const uint8_t*>(d_msg)), off(static_cast<const uint32_t*>(d_msg_off)),
        valid(static_cast<uint8_t*>(d_valid)), bitmap(static_cast<uint64_t*>(d_bitmap)),
        s(static_cast<hipStream_t>(stream)) {}
};

// Early-staged signatures (stage_sigs_early_locked) are valid only inside the
// lock hold of the cmtv_verify_commit call that staged them: every new hold
// forgets them, so a later call can never take stale device bytes for its own
// (the caller may refill the same buffer, and d_in / h_in may have been
// rewritten by another entry point meanwhile).
void clear_early_locked(cmtv_ctx* ctx) {
  for (auto& D : ctx->devs) {
    D.early_src = D.early_pk = nullptr;
    D.early_n = 0;
  }
}

int ctx_lock(cmtv_ctx* ctx, std::unique_lock<std::mutex>& lk) {
  ctx->lock_waiters.fetch_add(1, std::memory_order_relaxed);
  lk = std::unique_lock<std::mutex>(ctx->mu);
  ctx->lock_waiters.fetch_sub(1, std::memory_order_relaxed);
  clear_early_locked(ctx);
  // the forms of this hold's launches see one answer (keyed_form, ed_form)
  ctx->bulk_now = ctx->bulk_busy.load(std::memory_order_relaxed) > 0;
  ctx->under_load = ctx->bulk_now && ctx->lat_window_ns && ctx->load_form;
  return hipSetDevice(ctx->devs[0].ordinal) == hipSuccess ? CMTV_OK : CMTV_ENODEV;
}

void bulk_relock(cmtv_ctx* ctx, std::unique_lock<std::mutex>& lk) {
  // std::mutex is not fair: a pipeline thread that re-locks right after each
  // release can hold a 150-validator call off for several of its chunk
  // submissions (round 6: the under-load call's p99 was its wait before the
  // launch). Waiters go first, for at most 200 us.
  if (ctx->lock_waiters.load(std::memory_order_relaxed) > 0) {
    const auto t0 = std::chrono::steady_clock::now();
    while (ctx->lock_waiters.load(std::memory_order_relaxed) > 0 &&
           std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(200))
      std::this_thread::yield();
  }
  lk.lock();
}

uint32_t ctx_default_mode(const cmtv_ctx* ctx) { return ctx->default_mode; }

// ---------------------------------------------------------------- lifecycle

static int init_device(cmtv_ctx* ctx, CmtvDev& D) {
  if (hipSetDevice(D.ordinal) != hipSuccess) return CMTV_ENODEV;
  hipError_t e = hipStreamCreateWithFlags(&D.stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&D.scratch.done, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&D.done, hipEventDisableTiming);
  if (e == hipSuccess) e = hipMalloc(&D.d_diag, kDiagWords * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemsetAsync(D.d_diag, 0, kDiagWords * sizeof(uint32_t), D.stream);
  if (e == hipSuccess) e = hipMalloc(&D.d_rowslots, (size_t)kRowSlots * kRowSlotWords * sizeof(uint32_t));
  if (e == hipSuccess)
    e = hipMemsetAsync(D.d_rowslots, 0, (size_t)kRowSlots * kRowSlotWords * sizeof(uint32_t), D.stream);
  if (e == hipSuccess) e = hipMalloc(&D.d_btab, kBtabWords * sizeof(uint32_t));
  if (e == hipSuccess) e = launch_btab_init(D.d_btab, D.stream);
  uint32_t prog[SR_PREFIX_WORDS];
  ctx->sr_nops = sr_prefix_state(prog);
  if (ctx->sr_nops <= 0 && e == hipSuccess) e = hipErrorInvalidValue;
  if (e == hipSuccess) e = hipMalloc(&D.d_srprog, sizeof(prog));
  if (e == hipSuccess) e = hipMemcpyAsync(D.d_srprog, prog, sizeof(prog), hipMemcpyHostToDevice, D.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(D.stream);
  return e == hipSuccess ? CMTV_OK : hip_fail(e);
}

static void release_device(CmtvDev& D) {
  (void)hipSetDevice(D.ordinal);
  if (D.stream) (void)hipStreamSynchronize(D.stream);
  bulk_lane_release(D);
  for (DevBuf* b : {&D.scratch.buf, &D.d_in, &D.d_out, &D.d_all, &D.secp_in, &D.secp_out}) b->release();
  for (HostBuf* b : {&D.h_in, &D.h_out, &D.h_zc, &D.h_tags, &D.h_zin}) b->release();
  D.d_tags = nullptr;  // h_tags' device pointer
  for (MerkleSlot& M : D.merkle) {
    for (DevBuf* b : {&M.d_in, &M.d_nodes, &M.d_out}) b->release();
    for (HostBuf* b : {&M.h_in, &M.h_out}) b->release();
    if (M.done) (void)hipEventDestroy(M.done);
    M.done = nullptr;
  }
  for (uint32_t** p : {&D.d_btab, &D.d_srprog, &D.d_secp_gtab, &D.d_diag, &D.d_rowslots}) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
  D.timing.release();
  for (uint32_t k = 0; k < kRowSlots; k++) {
    if (D.row_ev[k]) (void)hipEventDestroy(D.row_ev[k]);
    D.row_ev[k] = nullptr;
    D.row_pending[k] = false;
  }
  if (D.scratch.done) (void)hipEventDestroy(D.scratch.done);
  if (D.done) (void)hipEventDestroy(D.done);
  if (D.poll_ev) (void)hipEventDestroy(D.poll_ev);
  D.poll_ev = nullptr;
  D.poll_pending = false;
  if (D.stream) (void)hipStreamDestroy(D.stream);
  D.scratch.done = D.done = nullptr;
  D.scratch.used = false;
  D.stream = nullptr;
}

// CMTV_FORM: comma-separated form names, a debug knob for tests and A/B runs
// (every other size keeps its band): row4 | row | oct2 | quad | lane (Ed25519;
// quad and lane also sr25519) and krow | kquad | klane (registered keys). An
// unknown name is reported once on stderr and ignored.
static void parse_forms(cmtv_ctx* ctx, const char* v) {
  static const struct {
    const char* name;
    bool keyed;
    uint32_t form;
  } kNames[] = {{"row4", false, kFormRow4}, {"row", false, kFormRow},   {"oct2", false, kFormOct2},
                {"quad", false, kFormQuad}, {"lane", false, kFormLane}, {"krow", true, kKeyedRow},
                {"kquad", true, kKeyedQuad}, {"klane", true, kKeyedLane}};
  std::string list(v);
  size_t p = 0;
  while (p <= list.size()) {
    size_t q = list.find(',', p);
    if (q == std::string::npos) q = list.size();
    const std::string tok = list.substr(p, q - p);
    p = q + 1;
    if (tok.empty()) continue;
    bool known = false;
    for (const auto& k : kNames)
      if (tok == k.name) {
        (k.keyed ? ctx->force_keyed : ctx->force_form) = k.form;
        known = true;
      }
    if (!known) std::fprintf(stderr, "cmtverify: CMTV_FORM: unknown form '%s' ignored\n", tok.c_str());
  }
}

// The knobs' shapes: a flag that is (env_is) or is not (env_not) one
// character -- an unset variable keeps the default -- and an integer taken
// only inside [lo, hi].
static void env_is(const char* name, char c, bool& flag) {
  if (const char* v = std::getenv(name)) flag = v[0] == c;
}
static void env_not(const char* name, char c, bool& flag) {
  if (const char* v = std::getenv(name)) flag = v[0] != c;
}
template <class T>
static void env_int(const char* name, long lo, long hi, T& field) {
  const char* v = std::getenv(name);
  if (!v) return;
  const long x = std::strtol(v, nullptr, 10);
  if (x >= lo && x <= hi) field = (T)x;
}

static void read_env(cmtv_ctx* ctx) {
  if (const char* f = std::getenv("CMTV_FORM")) parse_forms(ctx, f);
  if (const char* hp = std::getenv("CMTV_HS_PRE")) {
    // 0..16 comb positions; anything else keeps the kernel's default
    char* end = nullptr;
    const long v = std::strtol(hp, &end, 10);
    if (end != hp && *end == 0 && v >= 0 && v <= 16) ctx->hs_tune = (uint32_t)(v + 1);
  }
  if (const char* lc = std::getenv("CMTV_LANE_CHUNK")) {
    const size_t v = (size_t)std::strtoull(lc, nullptr, 10) / 64 * 64;
    if (v >= 64 && v <= kChunk) ctx->lane_chunk = v;
  }
  if (const char* sm = std::getenv("CMTV_SHARD_MIN")) ctx->shard_min = (size_t)std::strtoull(sm, nullptr, 10);
  if (const char* fa = std::getenv("CMTV_FAULT_AT")) ctx->fault_at = (uint64_t)std::strtoull(fa, nullptr, 10);
  env_is("CMTV_FORCE_WIDE", '1', ctx->force_wide);
  env_not("CMTV_NO_SB_FUSE", '1', ctx->sb_fuse);
  env_not("CMTV_NO_ZC_IN", '1', ctx->zc_in);
  env_not("CMTV_ZC_HOST_IN", '0', ctx->zc_host_in);
  env_not("CMTV_EARLY_SIGS", '0', ctx->early_sigs);
  if (const char* hp = std::getenv("CMTV_HOST_POLL")) ctx->host_poll = std::atoi(hp) != 0;
  if (const char* kl = std::getenv("CMTV_FORCE_K_LATE")) ctx->keyed_wait = kl[0] == '1' ? 0u : kKeyedWaitDefault;
  env_not("CMTV_HS_FOLD", '0', ctx->hs_fold);
  if (const char* pl = std::getenv("CMTV_FORCE_PS_LATE")) ctx->ps_wait = pl[0] == '1' ? 0u : kPsWaitDefault;
  env_not("CMTV_HS_SUM_SPLIT", '0', ctx->hs_sum_split);
  env_is("CMTV_FORCE_FG_LATE", '1', ctx->fg_late);
  if (ctx->fg_late && !std::getenv("CMTV_HS_SUM_SPLIT")) ctx->hs_sum_split = true;
  env_not("CMTV_HS_SUM_PIPE", '0', ctx->hs_sum_pipe);
  {
    uint32_t ft = 0;
    env_int("CMTV_HS_FOLD_TUNE", 0, 7, ft);
    ctx->hs_tune |= ft << 8;
  }
  env_int("CMTV_KEYED_BATCH_MIN_WAVES", 1, 1l << 20, ctx->keyed_batch_min_waves);
  env_int("CMTV_KEYED_BATCH_MIN_WAVES", 1, 1l << 20, ctx->secp_batch_min_waves);
  if (std::getenv("CMTV_KEYED_BATCH_MIN_WAVES")) ctx->secp_batch_max_kb = 8;
  env_not("CMTV_ROW_FENCE", '0', ctx->row_fence);
  env_is("CMTV_HOST_PHASES", '1', ctx->phases_on);
  if (const char* tm = std::getenv("CMTV_TIMING")) {
    const long v = std::strtol(tm, nullptr, 10);
    ctx->timing_every = v < 0 ? 0u : (uint32_t)std::min<long>(v, 1l << 20);
  }
  if (const char* fs = std::getenv("CMTV_FAULT_SYNC_DEV")) {
    char* end = nullptr;
    const long g = std::strtol(fs, &end, 10);
    if (end != fs && g >= 0) ctx->fault_sync_dev = g;
  }
  ctx->force_rccl = std::getenv("CMTV_FORCE_RCCL") != nullptr;
  if (const char* rl = std::getenv("CMTV_RCCL_LIB")) ctx->rccl_lib = rl;
  ctx->no_rccl = std::getenv("CMTV_NO_RCCL") != nullptr;
  ctx->no_rccl_fallback = std::getenv("CMTV_NO_RCCL_FALLBACK") != nullptr;
  env_int("CMTV_HOST_THREADS", 1, 256, ctx->host_threads);
  if (const char* v = std::getenv("CMTV_PIPE_MIN")) ctx->pipe_min = (size_t)std::strtoull(v, nullptr, 10);
  if (const char* v = std::getenv("CMTV_PIPE_CHUNK")) {
    const size_t c = (size_t)std::strtoull(v, nullptr, 10);
    if (c >= 64 && c <= (1u << 24)) ctx->pipe_chunk = c;
  }
  env_int("CMTV_PIPE_SLOTS", 2, kBulkSlotsMax, ctx->pipe_slots);
  env_not("CMTV_PIPELINE", '0', ctx->pipe_on);
  env_not("CMTV_PIPE_DIRECT", '0', ctx->pipe_direct);
  env_int("CMTV_SPEC_MIN", 1, LONG_MAX, ctx->spec_min);
  if (const char* v = std::getenv("CMTV_SPEC")) {
    if (v[0] == '0') ctx->spec_min = 0;
  }
  if (const char* v = std::getenv("CMTV_LAT_WINDOW_MS")) ctx->lat_window_ns = 1'000'000ull * std::strtoull(v, nullptr, 10);
  env_not("CMTV_LOAD_FORM", '0', ctx->load_form);
  env_not("CMTV_LOAD_ZC", '0', ctx->load_zc);
  env_is("CMTV_LOAD_POLL", '0', ctx->load_nopoll);
  env_is("CMTV_QUAD_POLL", '1', ctx->quad_poll);
  env_not("CMTV_KEYED_ZC", '0', ctx->keyed_zc);
  env_is("CMTV_SPIN_WAIT", '1', ctx->spin_wait);
  env_not("CMTV_PREP_STREAM", '0', ctx->prep_stream);
  env_is("CMTV_ONE_EXEC", '1', ctx->one_exec);
  env_is("CMTV_BULK_BM_DIRECT", '1', ctx->bulk_bm_direct);
  env_not("CMTV_SPLIT_SUBMIT", '0', ctx->split_submit);
  if (const char* v = std::getenv("CMTV_CALL_TRACE")) {
    ctx->call_trace = v[0] == '1' || v[0] == '2';
    ctx->call_trace_loaded_only = v[0] == '2';  // only calls beside a pipeline call
  }
  env_not("CMTV_LAT_ISOLATE", '0', ctx->lat_isolate);
  env_int("CMTV_LAT_RESERVE_CUS", 1, 64, ctx->lat_reserve_cus);
  env_int("CMTV_RCCL_DRAIN_MS", 1, 600000, ctx->rccl_drain_ms);
}

// CMTVERIFY_DEVICES: "0,1,2" or "all" (or unset: every visible device)
static std::vector<int> env_devices(int ndev) {
  std::vector<int> out;
  const char* v = std::getenv("CMTVERIFY_DEVICES");
  if (v && *v && std::strcmp(v, "all") != 0) {
    const char* p = v;
    while (*p) {
      char* end = nullptr;
      const long x = std::strtol(p, &end, 10);
      if (end == p) return {};
      out.push_back((int)x);
      p = end;
      while (*p == ',' || *p == ' ') p++;
    }
    return out;
  }
  for (int i = 0; i < ndev; i++) out.push_back(i);
  return out;
}

static int open_ctx(const cmtv_config* cfg, const std::vector<int>& ords, cmtv_ctx** out) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return CMTV_ENODEV;
  if (ords.empty() || ords.size() > (size_t)kMaxDevices) return CMTV_EINVAL;
  uint32_t cus = UINT32_MAX;
  for (int o : ords) {
    if (o < 0 || o >= ndev) return CMTV_ENODEV;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, o) != hipSuccess) return CMTV_ENODEV;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return CMTV_ENODEV;
    cus = std::min(cus, (uint32_t)std::max(prop.multiProcessorCount, 1));
  }
  auto* ctx = new (std::nothrow) cmtv_ctx();
  if (!ctx) return CMTV_ENOMEM;
  ctx->cus = cus;
  ctx->default_mode = cfg ? cfg->default_mode : CMTV_MODE_GO_STDLIB;
  if (!cfg) {
    const char* m = std::getenv("CMTVERIFY_MODE");
    if (m && std::strcmp(m, "zip215") == 0) ctx->default_mode = CMTV_MODE_ZIP215;
  }
  read_env(ctx);
  ctx->devs.resize(ords.size());
  for (size_t g = 0; g < ords.size(); g++) ctx->devs[g].ordinal = ords[g];
  for (auto& D : ctx->devs) {
    const int rc = init_device(ctx, D);
    if (rc != CMTV_OK) {
      cmtv_close(ctx);
      return rc;
    }
  }
  ctx->stats.n_devices = (uint32_t)ords.size();
  for (size_t g = 0; g < ords.size(); g++) ctx->live.push_back(g);
  // CMTV_FAULT_DEV=g: the g-th device's launches fail (re-shard test knob)
  if (const char* fd = std::getenv("CMTV_FAULT_DEV")) {
    char* end = nullptr;
    const long g = std::strtol(fd, &end, 10);
    if (end != fd && g >= 0 && (size_t)g < ords.size()) ctx->devs[(size_t)g].inject_fault = true;
  }
  if (ords.size() > 1) {
    for (size_t g = 0; g < ords.size(); g++) {  // peer access for the copy gathers
      (void)hipSetDevice(ords[g]);
      for (size_t h = 0; h < ords.size(); h++)
        if (ords[h] != ords[g]) (void)hipDeviceEnablePeerAccess(ords[h], 0);
    }
    (void)hipGetLastError();  // "already enabled" is not an error here
  }
  rebuild_comm(ctx);
  (void)hipSetDevice(ords[0]);
  *out = ctx;
  return CMTV_OK;
}

bool pinned_holds_locked(const cmtv_ctx* ctx, const void* p, size_t bytes) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  auto it = ctx->pinned.upper_bound(a);
  if (it == ctx->pinned.begin()) return false;
  --it;
  return a + bytes >= a && a + bytes <= it->first + it->second;
}

void pinned_ranges_locked(cmtv_ctx* ctx, std::vector<PinnedRange>& out) {
  out.clear();
  for (auto& b : ctx->pinned) out.push_back(PinnedRange{b.first, b.second});
}

}  // namespace cmtv

using namespace cmtv;

extern "C" {

int cmtv_abi_version(void) { return CMTV_ABI_VERSION; }

const char* cmtv_strerror(int code) {
  switch (code) {
    case CMTV_OK: return "ok";
    case CMTV_EINVAL: return "invalid argument";
    case CMTV_ENODEV: return "no usable gfx950 device";
    case CMTV_ENOMEM: return "out of device or pinned host memory";
    case CMTV_EHIP: return "HIP runtime error";
    case CMTV_ERCCL: return "collective communication error";
    case CMTV_ECOMMIT: return "commit verification failed";
    default: return "unknown error";
  }
}

int cmtv_open(const cmtv_config* cfg, cmtv_ctx** out) {
  if (!out) return CMTV_EINVAL;
  *out = nullptr;
  if (cfg && (cfg->flags != 0 || cfg->default_mode > CMTV_MODE_ZIP215)) return CMTV_EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return CMTV_ENODEV;
  int dev = 0;
  if (cfg && cfg->device >= 0) {
    dev = cfg->device;
  } else if (hipGetDevice(&dev) != hipSuccess) {
    dev = 0;
  }
  return open_ctx(cfg, {dev}, out);
}

int cmtv_open_devices(const cmtv_config* cfg, const int32_t* devices, size_t n_devices, cmtv_ctx** out) {
  if (!out) return CMTV_EINVAL;
  *out = nullptr;
  if (cfg && (cfg->flags != 0 || cfg->default_mode > CMTV_MODE_ZIP215)) return CMTV_EINVAL;
  if (n_devices > (size_t)kMaxDevices || (n_devices && !devices)) return CMTV_EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return CMTV_ENODEV;
  std::vector<int> ords = n_devices ? std::vector<int>(devices, devices + n_devices) : env_devices(ndev);
  if (ords.empty()) return CMTV_EINVAL;
  return open_ctx(cfg, ords, out);
}

void cmtv_close(cmtv_ctx* ctx) {
  if (!ctx) return;
  if (ctx->phases_on) {
    static const char* names[kPhCount] = {"prepare",   "stage",     "launch",      "wait",      "post",       "replay",
                                          "pipe_plan", "pipe_pack", "pipe_submit", "pipe_wait", "pipe_replay",
                                          "keyset",    "early",     "pipe_cut"};
    std::fprintf(stderr, "{\"cmtv_host_phases_us\": {");
    for (int p = 0; p < kPhCount; p++)
      std::fprintf(stderr, "%s\"%s\": %.3f", p ? ", " : "", names[p],
                   ctx->phase_calls ? 1e-3 * (double)ctx->phase_ns[p] / (double)ctx->phase_calls : 0.0);
    std::fprintf(stderr, "}, \"calls\": %llu}\n", (unsigned long long)ctx->phase_calls);
  }
  if (ctx->call_trace && !ctx->trace_rows.empty()) {
    static const char* seg[5] = {"to_lock", "to_launch", "gpu_and_wake", "post", "device_events"};
    std::fprintf(stderr, "{\"cmtv_call_trace_us\": {\"calls\": %zu", ctx->trace_rows.size());
    for (int k = 0; k < 5; k++) {
      std::vector<uint64_t> v;
      for (auto& r : ctx->trace_rows) v.push_back(r[k]);
      std::sort(v.begin(), v.end());
      auto q = [&](double f) { return 1e-3 * (double)v[std::min(v.size() - 1, (size_t)(f * (double)v.size()))]; };
      std::fprintf(stderr, ", \"%s\": [%.1f, %.1f, %.1f, %.1f]", seg[k], q(0.5), q(0.9), q(0.99), q(1.0));
    }
    // the slowest tenth of calls: which segment took their excess
    std::vector<size_t> idx(ctx->trace_rows.size());
    for (size_t i = 0; i < idx.size(); i++) idx[i] = i;
    auto total = [&](size_t i) { auto& r = ctx->trace_rows[i]; return r[0] + r[1] + r[2] + r[3]; };
    std::sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return total(a) < total(b); });
    std::fprintf(stderr, ", \"slowest_1pct\": [");
    const size_t from = idx.size() - std::max<size_t>(1, idx.size() / 100);
    for (size_t j = from; j < idx.size(); j++) {
      auto& r = ctx->trace_rows[idx[j]];
      std::fprintf(stderr, "%s[%.1f, %.1f, %.1f, %.1f, %.1f]", j > from ? ", " : "", 1e-3 * r[0], 1e-3 * r[1],
                   1e-3 * r[2], 1e-3 * r[3], 1e-3 * r[4]);
    }
    std::fprintf(stderr, "]}}\n");
  }
  for (auto& ev : ctx->trace_ev)
    if (ev) (void)hipEventDestroy(ev);
  ctx->pool.reset();
  for (auto& b : ctx->pinned) (void)hipHostFree(reinterpret_cast<void*>(b.first));  // the caller's leftovers
  ctx->pinned.clear();
  pipe_workspace_free(ctx->pipe_ws);
  ctx->pipe_ws = nullptr;
  for (auto& e : ctx->keysets) cmtv_keyset_free(e.second);
  ctx->keysets.clear();
  for (auto* k : ctx->secp_keysets) cmtv_secp_keyset_free(k);
  ctx->secp_keysets.clear();
  for (auto* z : ctx->zombies) cmtv_keyset_free(z);
  ctx->zombies.clear();
  drop_comms(ctx, false);
  for (auto& D : ctx->devs) release_device(D);
  delete ctx;
}

void* cmtv_stream(cmtv_ctx* ctx) { return ctx ? static_cast<void*>(ctx->devs[0].stream) : nullptr; }

int cmtv_device_count(const cmtv_ctx* ctx) { return ctx ? (int)ctx->devs.size() : 0; }

int cmtv_device_ordinal(const cmtv_ctx* ctx, int g) {
  if (!ctx || g < 0 || g >= (int)ctx->devs.size()) return CMTV_EINVAL;
  return ctx->devs[g].ordinal;
}

void* cmtv_device_stream(cmtv_ctx* ctx, int g) {
  if (!ctx || g < 0 || g >= (int)ctx->devs.size()) return nullptr;
  return static_cast<void*>(ctx->devs[g].stream);
}

int cmtv_sync(cmtv_ctx* ctx) {
  if (!ctx) return CMTV_EINVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  for (auto& D : ctx->devs) {
    if (D.failed) continue;
    if (hipSetDevice(D.ordinal) != hipSuccess) return CMTV_ENODEV;
    const hipError_t e = hipStreamSynchronize(D.stream);
    if (e != hipSuccess) return hip_fail(e);
  }
  harvest(ctx, false);
  (void)hipSetDevice(ctx->devs[0].ordinal);
  return CMTV_OK;
}

// the kernels' diagnostic counters of every usable device, summed
static void read_diag(cmtv_ctx* ctx) {
  uint64_t late = 0, late_ps = 0, late_sum = 0;
  for (auto& D : ctx->devs) {
    if (D.failed || !D.d_diag) continue;
    (void)hipSetDevice(D.ordinal);
    uint32_t w[kDiagWords] = {};
    if (hipMemcpy(w, D.d_diag, sizeof(w), hipMemcpyDeviceToHost) == hipSuccess) {
      late += w[kDiagLateK];
      late_ps += w[kDiagLatePs];
      late_sum += w[kDiagLateSum];
    }
  }
  ctx->stats.late_k_waves = late;
  ctx->stats.late_ps_waves = late_ps;
  ctx->late_sum_waves = late_sum;
}

int cmtv_stats_get(cmtv_ctx* ctx, cmtv_stats* out) {
  if (!ctx || !out) return CMTV_EINVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  harvest(ctx, true);
  read_diag(ctx);
  (void)hipSetDevice(ctx->devs[0].ordinal);
  ctx->stats.cache_entries = ctx->cache.size();
  ctx->stats.live_devices = (uint32_t)ctx->live.size();
  *out = ctx->stats;
  return CMTV_OK;
}

int cmtv_late_sum_waves(cmtv_ctx* ctx, uint64_t* out) {
  if (!ctx || !out) return CMTV_EINVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  harvest(ctx, true);
  read_diag(ctx);
  (void)hipSetDevice(ctx->devs[0].ordinal);
  *out = ctx->late_sum_waves;
  return CMTV_OK;
}

int cmtv_device_stats_get(cmtv_ctx* ctx, int g, cmtv_device_stats* out) {
  if (!ctx || !out || g < 0 || g >= (int)ctx->devs.size()) return CMTV_EINVAL;
  std::lock_guard<std::mutex> lk(ctx->mu);
  harvest(ctx, true);
  CmtvDev& D = ctx->devs[(size_t)g];
  std::memset(out, 0, sizeof(*out));
  out->ordinal = D.ordinal;
  out->failed = D.failed ? 1 : 0;
  out->calls = D.calls;
  out->signatures = D.signatures;
  out->kernel_launches = D.launches;
  out->device_ms = D.device_ms;
  out->timed_calls = D.timed_calls;
  (void)hipSetDevice(ctx->devs[0].ordinal);
  return CMTV_OK;
}

int cmtv_verdict_cache(cmtv_ctx* ctx, size_t max_entries) {
  if (!ctx || max_entries > (1u << 26)) return CMTV_EINVAL;
  std::lock_guard<std::mutex> g(ctx->mu);
  ctx->cache.reset(max_entries);
  return CMTV_OK;
}

int cmtv_verify_ed25519(cmtv_ctx* ctx, size_t n, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg,
                        const uint32_t* msg_off, uint32_t mode, uint8_t* out_valid, uint64_t* out_bitmap) {
  if (!host_args_ok(ctx, mode, n, pk, sig, msg, msg_off, out_valid, out_bitmap)) return CMTV_EINVAL;
  if (n == 0) return CMTV_OK;
  std::unique_lock<std::mutex> lk;
  if (ctx_lock(ctx, lk) != CMTV_OK) return CMTV_ENODEV;
  return verify_host_locked(ctx, n, pk, sig, msg, msg_off, mode, out_valid, out_bitmap);
}

int cmtv_verify_ed25519_device(cmtv_ctx* ctx, size_t n, const void* d_pk, const void* d_sig, const void* d_msg,
                               const void* d_msg_off, uint32_t mode, void* d_valid, void* d_bitmap, void* stream) {
  if (!device_args_ok(ctx, mode, n, d_pk, d_sig, d_msg, d_msg_off, d_valid, d_bitmap)) return CMTV_EINVAL;
  if (n == 0) return CMTV_OK;
  const DeviceArgs a(d_pk, d_sig, d_msg, d_msg_off, d_valid, d_bitmap, stream);
  return on_dev0(ctx, [&](CmtvDev& D) {
    return enqueue_verify(ctx, D, n, a.keys, a.sig, a.msg, a.off, mode, a.valid, a.bitmap, a.s);
  });
}

int cmtv_verify_sr25519(cmtv_ctx* ctx, size_t n, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg,
                        const uint32_t* msg_off, uint8_t* out_valid, uint64_t* out_bitmap) {
  if (!host_args_ok(ctx, 0, n, pk, sig, msg, msg_off, out_valid, out_bitmap)) return CMTV_EINVAL;
  if (n == 0) return CMTV_OK;
  std::unique_lock<std::mutex> lk;
  if (ctx_lock(ctx, lk) != CMTV_OK) return CMTV_ENODEV;
  return verify_host_locked(ctx, n, pk, sig, msg, msg_off, kModeSr25519, out_valid, out_bitmap);
}

int cmtv_verify_sr25519_device(cmtv_ctx* ctx, size_t n, const void* d_pk, const void* d_sig, const void* d_msg,
                               const void* d_msg_off, void* d_valid, void* d_bitmap, void* stream) {
  if (!device_args_ok(ctx, 0, n, d_pk, d_sig, d_msg, d_msg_off, d_valid, d_bitmap)) return CMTV_EINVAL;
  if (n == 0) return CMTV_OK;
  const DeviceArgs a(d_pk, d_sig, d_msg, d_msg_off, d_valid, d_bitmap, stream);
  return on_dev0(ctx, [&](CmtvDev& D) {
    return enqueue_verify(ctx, D, n, a.keys, a.sig, a.msg, a.off, kModeSr25519, a.valid, a.bitmap, a.s);
  });
}

int cmtv_verify_secp256k1(cmtv_ctx* ctx, size_t n, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg,
                          const uint32_t* msg_off, uint8_t* out_valid, uint64_t* out_bitmap) {
  if (!host_args_ok(ctx, 0, n, pk, sig, msg, msg_off, out_valid, out_bitmap)) return CMTV_EINVAL;
  if (n == 0) return CMTV_OK;
  return on_dev0(ctx, [&](CmtvDev&) {
    return verify_secp_host_locked(ctx, nullptr, n, pk, sig, msg, msg_off, out_valid, out_bitmap);
  });
}

int cmtv_verify_secp256k1_device(cmtv_ctx* ctx, size_t n, const void* d_pk, const void* d_sig, const void* d_msg,
                                 const void* d_msg_off, void* d_valid, void* d_bitmap, void* stream) {
  if (!device_args_ok(ctx, 0, n, d_pk, d_sig, d_msg, d_msg_off, d_valid, d_bitmap)) return CMTV_EINVAL;
  if (n == 0) return CMTV_OK;
  const DeviceArgs a(d_pk, d_sig, d_msg, d_msg_off, d_valid, d_bitmap, stream);
  return on_dev0(ctx, [&](CmtvDev& D) {
    return enqueue_verify_secp(ctx, D, n, a.keys, a.sig, a.msg, a.off, a.valid, a.bitmap, a.s);
  });
}

int cmtv_verify_ed25519_indexed(cmtv_ctx* ctx, const cmtv_keyset* ks, size_t n, const uint32_t* key_idx,
                                const uint8_t* sig, const uint8_t* msg, const uint32_t* msg_off, uint32_t mode,
                                uint8_t* out_valid, uint64_t* out_bitmap) {
  if (!ks || ks->ctx != ctx) return CMTV_EINVAL;
  if (!host_args_ok(ctx, mode, n, key_idx, sig, msg, msg_off, out_valid, out_bitmap)) return CMTV_EINVAL;
  if (n == 0) return CMTV_OK;
  for (size_t i = 0; i < n; i++)
    if (key_idx[i] >= ks->n) return CMTV_EINVAL;
  std::unique_lock<std::mutex> lk;
  if (ctx_lock(ctx, lk) != CMTV_OK) return CMTV_ENODEV;
  return verify_host_device(ctx, n, nullptr, sig, msg, msg_off, mode, out_valid, out_bitmap, ks, key_idx);
}

int cmtv_verify_ed25519_indexed_device(cmtv_ctx* ctx, const cmtv_keyset* ks, size_t n, const void* d_key_idx,
                                       const void* d_sig, const void* d_msg, const void* d_msg_off, uint32_t mode,
                                       void* d_valid, void* d_bitmap, void* stream) {
  if (!ks || ks->ctx != ctx) return CMTV_EINVAL;
  if (!device_args_ok(ctx, mode, n, d_key_idx, d_sig, d_msg, d_msg_off, d_valid, d_bitmap)) return CMTV_EINVAL;
  if (n == 0) return CMTV_OK;
  const DeviceArgs a(d_key_idx, d_sig, d_msg, d_msg_off, d_valid, d_bitmap, stream);
  return on_dev0(ctx, [&](CmtvDev& D) {
    const cmtv_keyset::PerDev& K = ks->dev[0];
    // a key set registered after device 0 was retired has no tables there
    if (!K.d_tab || !K.d_pk || !K.d_ok) return (int)CMTV_ENODEV;
    return enqueue_verify_keyed(ctx, D, K, ks->n, n, static_cast<const uint32_t*>(d_key_idx), a.sig, a.msg, a.off,
                                mode, a.valid, a.bitmap, a.s);
  });
}

int cmtv_verify_secp256k1_indexed(cmtv_ctx* ctx, const cmtv_secp_keyset* ks, size_t n, const uint32_t* key_idx,
                                  const uint8_t* sig, const uint8_t* msg, const uint32_t* msg_off,
                                  uint8_t* out_valid, uint64_t* out_bitmap) {
  if (!ks || ks->ctx != ctx) return CMTV_EINVAL;
  if (!host_args_ok(ctx, 0, n, key_idx, sig, msg, msg_off, out_valid, out_bitmap)) return CMTV_EINVAL;
  if (n == 0) return CMTV_OK;
  for (size_t i = 0; i < n; i++)
    if (key_idx[i] >= ks->n) return CMTV_EINVAL;
  return on_dev0(ctx, [&](CmtvDev&) {
    return verify_secp_host_locked(ctx, ks, n, key_idx, sig, msg, msg_off, out_valid, out_bitmap);
  });
}

int cmtv_verify_secp256k1_indexed_device(cmtv_ctx* ctx, const cmtv_secp_keyset* ks, size_t n, const void* d_key_idx,
                                         const void* d_sig, const void* d_msg, const void* d_msg_off, void* d_valid,
                                         void* d_bitmap, void* stream) {
  if (!ks || ks->ctx != ctx) return CMTV_EINVAL;
  if (!device_args_ok(ctx, 0, n, d_key_idx, d_sig, d_msg, d_msg_off, d_valid, d_bitmap)) return CMTV_EINVAL;
  if (n == 0) return CMTV_OK;
  const DeviceArgs a(d_key_idx, d_sig, d_msg, d_msg_off, d_valid, d_bitmap, stream);
  return on_dev0(ctx, [&](CmtvDev& D) {
    return enqueue_verify_secp_keyed(ctx, D, ks, n, static_cast<const uint32_t*>(d_key_idx), a.sig, a.msg, a.off,
                                     a.valid, a.bitmap, a.s);
  });
}

int cmtv_alloc_pinned(cmtv_ctx* ctx, size_t bytes, void** out) {
  if (!ctx || !out || bytes == 0) return CMTV_EINVAL;
  *out = nullptr;
  std::unique_lock<std::mutex> lk;
  if (ctx_lock(ctx, lk) != CMTV_OK) return CMTV_ENODEV;
  void* p = nullptr;
  // portable: every device of the context DMAs from it
  if (hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess || !p) {
    (void)hipGetLastError();
    return CMTV_ENOMEM;
  }
  try {
    ctx->pinned.emplace(reinterpret_cast<uintptr_t>(p), bytes);
  } catch (...) {
    (void)hipHostFree(p);
    return CMTV_ENOMEM;
  }
  *out = p;
  return CMTV_OK;
}

int cmtv_free_pinned(cmtv_ctx* ctx, void* p) {
  if (!ctx) return CMTV_EINVAL;
  if (!p) return CMTV_OK;
  std::unique_lock<std::mutex> lk;
  if (ctx_lock(ctx, lk) != CMTV_OK) return CMTV_ENODEV;
  auto it = ctx->pinned.find(reinterpret_cast<uintptr_t>(p));
  if (it == ctx->pinned.end()) return CMTV_EINVAL;  // not this context's block
  ctx->pinned.erase(it);
  return hipHostFree(p) == hipSuccess ? CMTV_OK : CMTV_EHIP;
}

int cmtv_pubkeys_ed25519(cmtv_ctx* ctx, size_t n, const uint8_t* seeds, uint8_t* out_pk) {
  if (!ctx || n > (1ull << 31) || (n && (!seeds || !out_pk))) return CMTV_EINVAL;
  if (n == 0) return CMTV_OK;
  std::unique_lock<std::mutex> lk;
  if (ctx_lock(ctx, lk) != CMTV_OK) return CMTV_ENODEV;
  // host buffers in and out: the first live device does it
  if (ctx->live.empty()) return CMTV_ENODEV;
  CmtvDev& D = ctx->devs[ctx->live[0]];
  if (hipSetDevice(D.ordinal) != hipSuccess) return CMTV_ENODEV;
  hipError_t e;
  if ((e = D.d_in.ensure(32 * n)) != hipSuccess) return hip_fail(e);
  if ((e = D.d_out.ensure(32 * n)) != hipSuccess) return hip_fail(e);
  if ((e = hipMemcpyAsync(D.d_in.p, seeds, 32 * n, hipMemcpyHostToDevice, D.stream)) != hipSuccess)
    return hip_fail(e);
  for (size_t c = 0; c < n; c += kChunk) {
    const uint32_t cn = (uint32_t)std::min<size_t>(kChunk, n - c);
    if ((e = launch_pubkey(cn, static_cast<uint8_t*>(D.d_in.p) + 32 * c, D.d_btab,
                           static_cast<uint8_t*>(D.d_out.p) + 32 * c, D.stream)) != hipSuccess)
      return hip_fail(e);
  }
  if ((e = hipMemcpyAsync(out_pk, D.d_out.p, 32 * n, hipMemcpyDeviceToHost, D.stream)) != hipSuccess)
    return hip_fail(e);
  if ((e = hipStreamSynchronize(D.stream)) != hipSuccess) return hip_fail(e);
  return CMTV_OK;
}

int cmtv_sign_ed25519(cmtv_ctx* ctx, size_t n, const uint8_t* seeds, const uint32_t* key_idx, const uint8_t* msg,
                      const uint32_t* msg_off, uint8_t* out_sig) {
  if (!ctx || n > (1ull << 31)) return CMTV_EINVAL;
  if (n == 0) return CMTV_OK;
  if (!seeds || !msg_off || !out_sig || (!msg && msg_off[n] != 0)) return CMTV_EINVAL;
  size_t nseeds = n;
  if (key_idx) {
    nseeds = 0;
    for (size_t i = 0; i < n; i++) nseeds = std::max<size_t>(nseeds, (size_t)key_idx[i] + 1);
  }
  for (size_t i = 0; i < n; i++)
    if (msg_off[i + 1] < msg_off[i]) return CMTV_EINVAL;
  std::unique_lock<std::mutex> lk;
  if (ctx_lock(ctx, lk) != CMTV_OK) return CMTV_ENODEV;
  // host buffers in and out: the first live device does it
  if (ctx->live.empty()) return CMTV_ENODEV;
  CmtvDev& D = ctx->devs[ctx->live[0]];
  if (hipSetDevice(D.ordinal) != hipSuccess) return CMTV_ENODEV;
  const size_t msg_bytes = msg_off[n];
  const size_t o_seed = 0, o_idx = align_up(32 * nseeds, 256), o_off = align_up(o_idx + (key_idx ? 4 * n : 0), 256);
  const size_t o_msg = align_up(o_off + 4 * (n + 1), 256), in_bytes = align_up(o_msg + msg_bytes + 16, 256);
  hipError_t e;
  if ((e = D.h_in.ensure(in_bytes)) != hipSuccess) return hip_fail(e);
  if ((e = D.d_in.ensure(in_bytes)) != hipSuccess) return hip_fail(e);
  if ((e = D.d_out.ensure(64 * n)) != hipSuccess) return hip_fail(e);
  auto* hin = static_cast<uint8_t*>(D.h_in.p);
  std::memcpy(hin + o_seed, seeds, 32 * nseeds);
  if (key_idx) std::memcpy(hin + o_idx, key_idx, 4 * n);
  std::memcpy(hin + o_off, msg_off, 4 * (n + 1));
  if (msg_bytes) std::memcpy(hin + o_msg, msg, msg_bytes);
  auto* din = static_cast<uint8_t*>(D.d_in.p);
  if ((e = hipMemcpyAsync(din, hin, in_bytes, hipMemcpyHostToDevice, D.stream)) != hipSuccess) return hip_fail(e);
  for (size_t c = 0; c < n; c += kChunk) {
    const uint32_t cn = (uint32_t)std::min<size_t>(kChunk, n - c);
    if ((e = launch_sign(cn, key_idx ? din + o_seed : din + o_seed + 32 * c, key_idx ? din + o_idx + 4 * c : nullptr,
                         din + o_msg, din + o_off + 4 * c, D.d_btab, static_cast<uint8_t*>(D.d_out.p) + 64 * c,
                         D.stream)) != hipSuccess)
      return hip_fail(e);
  }
  if ((e = hipMemcpyAsync(out_sig, D.d_out.p, 64 * n, hipMemcpyDeviceToHost, D.stream)) != hipSuccess)
    return hip_fail(e);
  if ((e = hipStreamSynchronize(D.stream)) != hipSuccess) return hip_fail(e);
  return CMTV_OK;
}

int cmtv_privkey_secp256k1_from_secret(const uint8_t* secret, size_t len, uint8_t out_priv[32]) {
  if (!out_priv || (len && !secret) || len > (1ull << 31)) return CMTV_EINVAL;
  // sha256_msg reads whole aligned words around its message: a copy of our own
  std::vector<uint32_t> buf(len / 4 + 2, 0u);
  if (len) std::memcpy(buf.data(), secret, len);
  uint32_t c[8];
  sha256_msg(c, reinterpret_cast<const uint8_t*>(buf.data()), (uint32_t)len);
  secp_privkey_from_digest(out_priv, c);
  return CMTV_OK;
}

// the device the secp256k1 and sr25519 test-data calls run on: the first live one, made current
static int secp_testdata_dev(cmtv_ctx* ctx, std::unique_lock<std::mutex>& lk, CmtvDev*& D) {
  if (ctx_lock(ctx, lk) != CMTV_OK) return CMTV_ENODEV;
  if (ctx->live.empty()) return CMTV_ENODEV;
  D = &ctx->devs[ctx->live[0]];
  return hipSetDevice(D->ordinal) == hipSuccess ? CMTV_OK : CMTV_ENODEV;
}

int cmtv_pubkeys_secp256k1(cmtv_ctx* ctx, size_t n, const uint8_t* priv, uint8_t* out_pk, uint8_t* out_addr) {
  if (!ctx || n > (1ull << 31)) return CMTV_EINVAL;
  if (n == 0) return CMTV_OK;
  if (!priv || !out_pk) return CMTV_EINVAL;
  for (size_t i = 0; i < n; i++)
    if (!secp_privkey_in_range(priv + 32 * i)) return CMTV_EINVAL;
  std::unique_lock<std::mutex> lk;
  CmtvDev* D = nullptr;
  if (const int rc = secp_testdata_dev(ctx, lk, D)) return rc;
  return secp_pubkeys_host_locked(ctx, *D, n, priv, out_pk, out_addr);
}

int cmtv_sign_secp256k1(cmtv_ctx* ctx, size_t n_keys, const uint8_t* priv, size_t n, const uint32_t* key_idx,
                        const uint8_t* msg, const uint32_t* msg_off, uint8_t* out_sig) {
  if (!ctx || n > (1ull << 31) || n_keys > (1ull << 31)) return CMTV_EINVAL;
  if (!key_idx && n != n_keys) return CMTV_EINVAL;
  if (n == 0) return CMTV_OK;
  if (!priv || !msg_off || !out_sig || n_keys == 0 || (!msg && msg_off[n] != 0)) return CMTV_EINVAL;
  for (size_t i = 0; i < n; i++)
    if (msg_off[i + 1] < msg_off[i] || (key_idx && key_idx[i] >= n_keys)) return CMTV_EINVAL;
  for (size_t i = 0; i < n_keys; i++)
    if (!secp_privkey_in_range(priv + 32 * i)) return CMTV_EINVAL;
  std::unique_lock<std::mutex> lk;
  CmtvDev* D = nullptr;
  if (const int rc = secp_testdata_dev(ctx, lk, D)) return rc;
  return secp_sign_host_locked(ctx, *D, n_keys, priv, n, key_idx, msg, msg_off, out_sig);
}

// every 32-byte string is a mini secret: no key-range check
int cmtv_pubkeys_sr25519(cmtv_ctx* ctx, size_t n, const uint8_t* mini, uint8_t* out_pk, uint8_t* out_addr) {
  if (!ctx || n > (1ull << 31)) return CMTV_EINVAL;
  if (n == 0) return CMTV_OK;
  if (!mini || !out_pk) return CMTV_EINVAL;
  std::unique_lock<std::mutex> lk;
  CmtvDev* D = nullptr;
  if (const int rc = secp_testdata_dev(ctx, lk, D)) return rc;
  return sr_pubkeys_host_locked(ctx, *D, n, mini, out_pk, out_addr);
}

int cmtv_sign_sr25519(cmtv_ctx* ctx, size_t n_keys, const uint8_t* mini, size_t n, const uint32_t* key_idx,
                      const uint8_t* msg, const uint32_t* msg_off, uint8_t* out_sig) {
  if (!ctx || n > (1ull << 31) || n_keys > (1ull << 31)) return CMTV_EINVAL;
  if (!key_idx && n != n_keys) return CMTV_EINVAL;
  if (n == 0) return CMTV_OK;
  if (!mini || !msg_off || !out_sig || n_keys == 0 || (!msg && msg_off[n] != 0)) return CMTV_EINVAL;
  for (size_t i = 0; i < n; i++)
    if (msg_off[i + 1] < msg_off[i] || (key_idx && key_idx[i] >= n_keys)) return CMTV_EINVAL;
  std::unique_lock<std::mutex> lk;
  CmtvDev* D = nullptr;
  if (const int rc = secp_testdata_dev(ctx, lk, D)) return rc;
  return sr_sign_host_locked(ctx, *D, n_keys, mini, n, key_idx, msg, msg_off, out_sig);
}

}  // extern "C"
