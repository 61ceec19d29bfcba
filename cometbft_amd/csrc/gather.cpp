// gather.cpp -- several devices in one context: the RCCL entry points
// (dlopen), the verdict-bitmap all-gather over them or over peer copies, the
// communicator's rebuild when a device is retired, and the sharded
// device-resident entry points.
#include <dlfcn.h>

#include <thread>

#include "runtime_state.h"

namespace cmtv {

static Rccl load_rccl(const char* path) {
  Rccl x;
  void* h = nullptr;
  if (path) {
    h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
  } else {
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
      if ((h = dlopen(name, RTLD_NOW | RTLD_LOCAL)) != nullptr) break;
  }
  if (!h) return x;
  x.CommInitAll = reinterpret_cast<decltype(x.CommInitAll)>(dlsym(h, "ncclCommInitAll"));
  x.CommDestroy = reinterpret_cast<decltype(x.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
  x.AllGather = reinterpret_cast<decltype(x.AllGather)>(dlsym(h, "ncclAllGather"));
  x.GroupStart = reinterpret_cast<decltype(x.GroupStart)>(dlsym(h, "ncclGroupStart"));
  x.GroupEnd = reinterpret_cast<decltype(x.GroupEnd)>(dlsym(h, "ncclGroupEnd"));
  x.CommAbort = reinterpret_cast<decltype(x.CommAbort)>(dlsym(h, "ncclCommAbort"));
  x.ok = x.CommInitAll && x.CommDestroy && x.AllGather && x.GroupStart && x.GroupEnd;
  return x;
}

// The RCCL entry points for a context: the system librccl, or the library
// CMTV_RCCL_LIB names (read at open; tests/host/rccl_stub.cpp rehearses the
// multi-rank code on one GPU). Each library is resolved once per process.
static const Rccl& rccl(const std::string& path = std::string()) {
  static std::mutex mu;
  static std::unordered_map<std::string, Rccl> libs;
  std::lock_guard<std::mutex> g(mu);
  auto it = libs.find(path);
  if (it == libs.end()) it = libs.emplace(path, load_rccl(path.empty() ? nullptr : path.c_str())).first;
  return it->second;
}

// ---------------------------------------------------------------- sharding

// Waits up to ctx->rccl_drain_ms for the streams of devices dev[0..G);
// false if one still has work queued (a collective that cannot complete).
static bool drain_bounded(cmtv_ctx* ctx, const size_t* dev, size_t G) {
  const auto t_end = std::chrono::steady_clock::now() + std::chrono::milliseconds(ctx->rccl_drain_ms);
  for (size_t g = 0; g < G; g++) {
    CmtvDev& D = ctx->devs[dev[g]];
    (void)hipSetDevice(D.ordinal);
    for (;;) {
      const hipError_t q = hipStreamQuery(D.stream);
      if (q != hipErrorNotReady) break;  // done (or failed: nothing left to wait for)
      if (std::chrono::steady_clock::now() > t_end) return false;
      std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
  }
  (void)hipGetLastError();
  return true;
}

// Releases every device's communicator; abort = ncclCommAbort where the
// library has it (ends collectives stuck on their peers), else CommDestroy.
void drop_comms(cmtv_ctx* ctx, bool abort) {
  const Rccl& R = rccl(ctx->rccl_lib);
  for (auto& D : ctx->devs) {
    if (D.comm && R.ok) {
      (void)hipSetDevice(D.ordinal);
      if (abort && R.CommAbort)
        (void)R.CommAbort(D.comm);
      else
        (void)R.CommDestroy(D.comm);
    }
    D.comm = nullptr;
  }
}

// Bitmap all-gather over the devices dev[0..G): the one at position g holds
// its shard in words [g W, (g+1) W) of bufs[g] (G x W words each); afterwards
// every bufs[g] holds all shards. RCCL all-gather in place when the context
// has a communicator (then dev must be ctx->live, the communicator's ranks in
// order), else peer copies (a context over a repeated device ordinal).
// Enqueued on the device streams.
int gather_bitmaps(cmtv_ctx* ctx, const size_t* dev, size_t G, size_t W, uint64_t* const* bufs) {
  // one device: nothing to exchange, unless CMTV_FORCE_RCCL gave it a
  // one-rank communicator (the RCCL path exercised on a one-GPU box)
  if (G <= 1 && !ctx->rccl) return CMTV_OK;
  ctx->stats.gathers++;
  if (ctx->rccl) {
    const Rccl& R = rccl(ctx->rccl_lib);
    int bad = R.GroupStart() != 0;
    for (size_t g = 0; g < G && !bad; g++) {
      CmtvDev& D = ctx->devs[dev[g]];
      (void)hipSetDevice(D.ordinal);
      bad |= R.AllGather(bufs[g] + g * W, bufs[g], W, kNcclUint64, D.comm, D.stream) != 0;
    }
    bad |= R.GroupEnd() != 0;
    if (!bad) return CMTV_OK;
    // RCCL refused the gather (a node whose xGMI / RCCL setup fails at run
    // time). Some ranks' collectives may already be enqueued (RCCL launches
    // each rank's kernel at GroupEnd): they wait for peers that never come,
    // and anything queued behind them would hang. So the communicators go
    // (aborted when a stream does not drain within rccl_drain_ms, which ends
    // a stuck collective), the context never builds one again, and only a
    // gather whose streams drained falls back to peer copies below -- this one
    // and every later one; CMTV_NO_RCCL_FALLBACK=1 reports CMTV_ERCCL instead.
    ctx->stats.rccl_failures++;
    const bool drained = drain_bounded(ctx, dev, G);
    drop_comms(ctx, !drained);
    ctx->rccl_broken = true;
    ctx->rccl = false;
    ctx->stats.rccl = 0;
    if (!drained) {
      // an aborted collective leaves its stream in an error state: wait once
      // more (bounded) so a later call does not queue behind it
      (void)drain_bounded(ctx, dev, G);
      return CMTV_ERCCL;
    }
    if (ctx->no_rccl_fallback) return CMTV_ERCCL;
  }
  hipError_t e;
  for (size_t h = 0; h < G; h++) {
    CmtvDev& H = ctx->devs[dev[h]];
    (void)hipSetDevice(H.ordinal);
    if ((e = hipEventRecord(H.done, H.stream)) != hipSuccess) return hip_fail(e);
  }
  for (size_t g = 0; g < G; g++) {
    CmtvDev& D = ctx->devs[dev[g]];
    (void)hipSetDevice(D.ordinal);
    for (size_t h = 0; h < G; h++) {
      if (h == g) continue;
      CmtvDev& H = ctx->devs[dev[h]];
      if ((e = hipStreamWaitEvent(D.stream, H.done, 0)) != hipSuccess) return hip_fail(e);
      if ((e = hipMemcpyPeerAsync(bufs[g] + h * W, D.ordinal, bufs[h] + h * W, H.ordinal, W * 8, D.stream)) !=
          hipSuccess)
        return hip_fail(e);
    }
  }
  // the copies read other devices' buffers: finish them before those
  // devices' next kernels may write
  for (size_t g = 0; g < G; g++) {
    CmtvDev& D = ctx->devs[dev[g]];
    (void)hipSetDevice(D.ordinal);
    if ((e = hipStreamSynchronize(D.stream)) != hipSuccess) return hip_fail(e);
  }
  return CMTV_OK;
}

// The bitmap communicator over the live devices (rank = position in
// ctx->live), when their ordinals are distinct and librccl loads; a one-rank
// communicator only under CMTV_FORCE_RCCL (the RCCL path on a one-GPU box).
// Otherwise gathers use peer copies. Called at open and after a device is
// retired (the old communicator included it).
void rebuild_comm(cmtv_ctx* ctx) {
  const Rccl& R = rccl(ctx->rccl_lib);
  drop_comms(ctx, false);
  ctx->rccl = false;
  std::vector<int> ords;
  for (size_t d : ctx->live) ords.push_back(ctx->devs[d].ordinal);
  std::vector<int> sorted = ords;
  std::sort(sorted.begin(), sorted.end());
  const bool distinct = std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end();
  // a repeated ordinal gets a communicator only from a library named by
  // CMTV_RCCL_LIB under CMTV_FORCE_RCCL (the one-GPU rehearsal of the
  // multi-rank path); the system RCCL refuses duplicate devices
  const bool repeat_ok = ctx->force_rccl && !ctx->rccl_lib.empty();
  const bool want = !ctx->rccl_broken && (ords.size() > 1 ? ((distinct || repeat_ok) && !ctx->no_rccl)
                                                           : (ords.size() == 1 && ctx->force_rccl));
  if (want && R.ok) {
    std::vector<ncclComm_t> comms(ords.size(), nullptr);
    if (R.CommInitAll(comms.data(), (int)ords.size(), ords.data()) == 0) {
      for (size_t g = 0; g < ords.size(); g++) ctx->devs[ctx->live[g]].comm = comms[g];
      ctx->rccl = true;
    }
  }
  ctx->stats.rccl = ctx->rccl ? 1 : 0;
  (void)hipSetDevice(ctx->devs[ctx->live.empty() ? 0 : ctx->live[0]].ordinal);
}

// Takes device d out of the context's rotation after a HIP error
// (per-GPU failure -> re-shard onto the remaining GPUs; the
// libs/fail/fail.go analogue is CMTV_FAULT_DEV). Its communicator rank goes
// too: the RCCL communicator is rebuilt over the survivors.
void retire_device(cmtv_ctx* ctx, size_t d) {
  if (ctx->devs[d].failed) return;
  ctx->devs[d].failed = true;
  ctx->stats.device_failures++;
  ctx->live.erase(std::remove(ctx->live.begin(), ctx->live.end(), d), ctx->live.end());
  rebuild_comm(ctx);
}

bool retire_device_locked(cmtv_ctx* ctx, size_t dev) {
  // retired meanwhile by another call (the pipeline holds the lock only
  // around submissions): already out of the rotation, so the chunks run again
  // on whatever is still live
  if (ctx->devs[dev].failed) return !ctx->live.empty();
  // CMTV_FAULT_AT stands for a failure of the call, not of the device
  const bool injected = ctx->fault_pending;
  ctx->fault_pending = false;
  if (injected || ctx->live.size() < 2) return false;
  retire_device(ctx, dev);
  ctx->stats.reshards++;
  return true;
}

// The sharded device-resident entry points (their argument checks and lock
// hold included): shard g's inputs on device g, each verified on its device's
// stream, then the bitmap gather.
static int sharded_device(cmtv_ctx* ctx, const cmtv_keyset* ks, const size_t* n_shard, const void* const* d_keys,
                          const void* const* d_sig, const void* const* d_msg, const void* const* d_off,
                          uint32_t mode, void* const* d_valid, void* const* d_bitmap_all, size_t* words_per_shard,
                          bool gather = true) {
  if (!ctx || mode > CMTV_MODE_ZIP215 || !n_shard || !d_keys || !d_sig || !d_msg || !d_off || !d_bitmap_all)
    return CMTV_EINVAL;
  std::unique_lock<std::mutex> lk;
  if (ctx_lock(ctx, lk) != CMTV_OK) return CMTV_ENODEV;
  const size_t G = ctx->devs.size();
  // the caller's inputs live on every device: a retired one cannot take part
  if (ctx->live.size() != G) return CMTV_ENODEV;
  size_t W = 0;
  for (size_t g = 0; g < G; g++) {
    if (n_shard[g] > (1ull << 31)) return CMTV_EINVAL;
    if (n_shard[g] && (!d_keys[g] || !d_sig[g] || !d_msg[g] || !d_off[g])) return CMTV_EINVAL;
    if (!d_bitmap_all[g]) return CMTV_EINVAL;
    W = std::max(W, (n_shard[g] + 63) / 64);
  }
  if (words_per_shard) *words_per_shard = W;
  if (W == 0) return CMTV_OK;
  uint64_t* bufs[kMaxDevices];
  hipError_t e;
  for (size_t g = 0; g < G; g++) {
    CmtvDev& D = ctx->devs[g];
    if (hipSetDevice(D.ordinal) != hipSuccess) return CMTV_ENODEV;
    bufs[g] = static_cast<uint64_t*>(d_bitmap_all[g]);
    // independent batches (no gather): device g's bitmap is its own words
    uint64_t* own_bm = gather ? bufs[g] + g * W : bufs[g];
    // words of this shard beyond its signatures stay zero (quad kernels write
    // whole 16-bit slices, lane kernels whole words; a short shard leaves the
    // rest of its W words untouched)
    const size_t own = (n_shard[g] + 63) / 64;
    if (gather && own < W && (e = hipMemsetAsync(own_bm + own, 0, 8 * (W - own), D.stream)) != hipSuccess)
      return hip_fail(e);
    uint8_t* dv = d_valid ? static_cast<uint8_t*>(d_valid[g]) : nullptr;
    int rc;
    if (ks)
      rc = enqueue_verify_keyed(ctx, D, ks->dev[g], ks->n, n_shard[g], static_cast<const uint32_t*>(d_keys[g]),
                                static_cast<const uint8_t*>(d_sig[g]), static_cast<const uint8_t*>(d_msg[g]),
                                static_cast<const uint32_t*>(d_off[g]), mode, dv, own_bm, D.stream);
    else
      rc = enqueue_verify(ctx, D, n_shard[g], static_cast<const uint8_t*>(d_keys[g]),
                          static_cast<const uint8_t*>(d_sig[g]), static_cast<const uint8_t*>(d_msg[g]),
                          static_cast<const uint32_t*>(d_off[g]), mode, dv, own_bm, D.stream);
    if (rc != CMTV_OK) {
      // a device's own HIP error takes it out of the rotation (host batches
      // re-plan over the others); this call fails: its inputs were there
      const bool injected = ctx->fault_pending;
      ctx->fault_pending = false;
      if (rc == CMTV_EHIP && !injected && G > 1) retire_device(ctx, g);
      (void)hipSetDevice(ctx->devs[0].ordinal);
      return rc;
    }
  }
  if (!gather) {
    (void)hipSetDevice(ctx->devs[0].ordinal);
    return CMTV_OK;
  }
  if (G > 1) ctx->stats.sharded_calls++;
  const int rc = gather_bitmaps(ctx, ctx->live.data(), G, W, bufs);
  (void)hipSetDevice(ctx->devs[0].ordinal);
  return rc;
}

}  // namespace cmtv

using namespace cmtv;

extern "C" {

int cmtv_verify_ed25519_sharded_device(cmtv_ctx* ctx, const size_t* n_shard, const void* const* d_pk,
                                       const void* const* d_sig, const void* const* d_msg,
                                       const void* const* d_msg_off, uint32_t mode, void* const* d_valid,
                                       void* const* d_bitmap_all, size_t* words_per_shard) {
  return sharded_device(ctx, nullptr, n_shard, d_pk, d_sig, d_msg, d_msg_off, mode, d_valid, d_bitmap_all,
                        words_per_shard);
}

int cmtv_verify_ed25519_multi_device(cmtv_ctx* ctx, const size_t* n_dev, const void* const* d_pk,
                                     const void* const* d_sig, const void* const* d_msg,
                                     const void* const* d_msg_off, uint32_t mode, void* const* d_valid,
                                     void* const* d_bitmap) {
  return sharded_device(ctx, nullptr, n_dev, d_pk, d_sig, d_msg, d_msg_off, mode, d_valid, d_bitmap, nullptr,
                        false);
}

int cmtv_verify_ed25519_indexed_sharded_device(cmtv_ctx* ctx, const cmtv_keyset* ks, const size_t* n_shard,
                                               const void* const* d_key_idx, const void* const* d_sig,
                                               const void* const* d_msg, const void* const* d_msg_off,
                                               uint32_t mode, void* const* d_valid, void* const* d_bitmap_all,
                                               size_t* words_per_shard) {
  if (!ks || ks->ctx != ctx) return CMTV_EINVAL;
  return sharded_device(ctx, ks, n_shard, d_key_idx, d_sig, d_msg, d_msg_off, mode, d_valid, d_bitmap_all,
                        words_per_shard);
}

}  // extern "C"
