// bulk_lane.cpp -- the cross-height pipeline's lane on each device
// (runtime_internal.h "bulk lanes"): its streams and staging slots, the
// CU-masked exec and latency streams that keep a latency call's CUs free
// beside it, the latency window, the host worker pool and the call trace.
#include <sched.h>

#include <cstdlib>
#include <fstream>
#include <thread>

#include "runtime_state.h"
#include "signbytes.h"

namespace cmtv {

// ---------------------------------------------------------------- bulk lanes

std::mutex& bulk_mutex(cmtv_ctx* ctx) { return ctx->bulk_mu; }

// CUs a masked bulk lane leaves to the latency stream (bulk_lane_init): a
// multiple of 8 (every XCD), at most a quarter of the device, 0 below 64 CUs
static uint32_t reserved_cus(const cmtv_ctx* ctx, uint32_t cus) {
  if (cus < 64) return 0;
  return std::min((ctx->lat_reserve_cus + 7) / 8 * 8, cus / 4 / 8 * 8);
}

// CPUs this process may run on: the affinity mask, bounded by a cgroup v2
// CPU quota (cpu.max) when one is set
static unsigned usable_cpus() {
  unsigned n = 0;
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof(set), &set) == 0) n = (unsigned)CPU_COUNT(&set);
  if (n == 0) n = std::max(1u, std::thread::hardware_concurrency());
  std::ifstream f("/sys/fs/cgroup/cpu.max");
  std::string quota, period;
  if (f >> quota >> period && quota != "max") {
    const double q = std::atof(quota.c_str()), p = std::atof(period.c_str());
    if (q > 0 && p > 0) n = std::min(n, std::max(1u, (unsigned)(q / p)));
  }
  return n;
}

HostPool& host_pool(cmtv_ctx* ctx) {
  if (!ctx->pool) {
    // default: at most 16, and three CPUs short of a small CPU budget, so a
    // latency caller (consensus) and the HIP runtime's threads keep a CPU
    // under a cgroup quota (round 6, tools/gpu_r6aa.sh, 16-CPU quota, three
    // alternating rounds: latency_150_under_load p99 0.125-0.137 ms with 13
    // workers against 0.132-0.173 with 16)
    const unsigned u = usable_cpus();
    const unsigned t = ctx->host_threads ? ctx->host_threads : std::min(16u, u > 8 ? u - 3 : u);
    ctx->pool.reset(new HostPool(t));
  }
  return *ctx->pool;
}

PipeConfig pipe_config(const cmtv_ctx* ctx) {
  PipeConfig pc{ctx->pipe_min, ctx->pipe_chunk, ctx->pipe_slots, ctx->pipe_on, ctx->pipe_direct};
  pc.split_submit = ctx->split_submit;
  // a masked lane's round: the chunk scaled to the CUs it keeps (bulk_lane_init)
  const uint32_t reserved = reserved_cus(ctx, ctx->cus);
  pc.chunk_masked = ctx->cus > reserved
                        ? std::max<size_t>(64, ctx->pipe_chunk / ctx->cus * (ctx->cus - reserved))
                        : ctx->pipe_chunk;
  return pc;
}

bool call_trace_on(const cmtv_ctx* ctx) { return ctx->call_trace; }
uint64_t call_trace_now() { return now_ns_steady(); }
void call_trace_begin_locked(cmtv_ctx* ctx) { ctx->trace_launch = ctx->trace_wait = 0; }
void call_trace_record_locked(cmtv_ctx* ctx, uint64_t t_entry, uint64_t t_locked) {
  const uint64_t t_end = now_ns_steady();
  if (!ctx->trace_launch || !ctx->trace_wait) return;  // no small host batch ran
  if (ctx->call_trace_loaded_only && !ctx->bulk_now) return;
  std::lock_guard<std::mutex> g(ctx->trace_mu);
  ctx->trace_rows.push_back({t_locked - t_entry, ctx->trace_launch - t_locked, ctx->trace_wait - ctx->trace_launch,
                             t_end - ctx->trace_wait, ctx->trace_dev_ns});
}

void note_latency(cmtv_ctx* ctx) {
  ctx->last_latency_ns.store(now_ns_steady(), std::memory_order_relaxed);
}

bool latency_recent(const cmtv_ctx* ctx) {
  if (!ctx->lat_window_ns) return false;
  const uint64_t t = ctx->last_latency_ns.load(std::memory_order_relaxed);
  return t && now_ns_steady() - t < ctx->lat_window_ns;
}

LatencyStreams::LatencyStreams(cmtv_ctx* c) : ctx(c) {
  // the pipeline's masked chunks leave the reserved CUs free only while the
  // latency window is open; bulk_now (snapshotted at ctx_lock) says a
  // pipeline call is in flight
  if (!ctx->bulk_now || !ctx->lat_window_ns || !ctx->lat_isolate) return;
  for (size_t g : ctx->live) {
    CmtvDev& D = ctx->devs[g];
    BulkLane& L = D.bulk;
    if (!L.lat || D.failed || g >= 64) continue;
    (void)hipSetDevice(D.ordinal);
    // everything already on the normal stream (keyset builds, a polled
    // launch) completes first -- through an event only when something is
    // still in flight there: a cross-queue wait costs the launch ~45 us
    // (tools/lat_queue_probe.hip: 22.8 -> 69.2 us p50 for a 10 us kernel)
    const hipError_t q = hipStreamQuery(D.stream);
    if (q != hipSuccess && (q != hipErrorNotReady || hipEventRecord(L.lat_in, D.stream) != hipSuccess ||
                            hipStreamWaitEvent(L.lat, L.lat_in, 0) != hipSuccess)) {
      (void)hipGetLastError();
      continue;
    }
    std::swap(D.stream, L.lat);
    swapped |= 1ull << g;
  }
  if (swapped) ctx->stats.isolated_calls++;
  if (!ctx->live.empty()) (void)hipSetDevice(ctx->devs[ctx->live[0]].ordinal);
}

LatencyStreams::~LatencyStreams() {
  for (size_t g = 0; g < 64 && swapped; g++) {
    if (!(swapped >> g & 1)) continue;
    CmtvDev& D = ctx->devs[g];
    BulkLane& L = D.bulk;
    (void)hipSetDevice(D.ordinal);
    std::swap(D.stream, L.lat);
    // and what the call left in flight (a polled launch retiring) precedes
    // whatever comes next on the normal stream (an event only if needed)
    const hipError_t q = hipStreamQuery(L.lat);
    if (q == hipErrorNotReady) {
      if (hipEventRecord(L.lat_out, L.lat) != hipSuccess || hipStreamWaitEvent(D.stream, L.lat_out, 0) != hipSuccess)
        (void)hipGetLastError();
    } else if (q != hipSuccess) {
      (void)hipGetLastError();
    }
  }
  if (swapped && !ctx->live.empty()) (void)hipSetDevice(ctx->devs[ctx->live[0]].ordinal);
}

BulkBusy::BulkBusy(cmtv_ctx* c) : ctx(c) { ctx->bulk_busy.fetch_add(1, std::memory_order_relaxed); }
BulkBusy::~BulkBusy() { ctx->bulk_busy.fetch_sub(1, std::memory_order_relaxed); }

void live_devices_locked(cmtv_ctx* ctx, std::vector<size_t>& out) { out = ctx->live; }

static hipError_t bulk_lane_init(cmtv_ctx* ctx, CmtvDev& D) {
  BulkLane& L = D.bulk;
  if (L.exec) return hipSuccess;
  // Every stream of the lane gets a hardware queue of its own (a CU-masked
  // stream has one; plain streams share the process's GPU_MAX_HW_QUEUES
  // queues round-robin). On a shared queue the device's normal stream -- a
  // 150-validator VerifyCommit -- waits behind whatever the lane queued
  // before it: the barrier packet of an 80 MB chunk DMA, a 2.7 ms keyed
  // launch (round 6: p99 1.12 ms under a configs[2] load with the copy and
  // exec streams plain, bench latency_150_under_load).
  int cus = 0;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, D.ordinal);
  L.cus = (uint32_t)std::max(cus, 1);
  const uint32_t words = (L.cus + 31) / 32;
  std::vector<uint32_t> all(words, 0);
  for (uint32_t c = 0; c < L.cus; c++) all[c / 32] |= 1u << (c % 32);
  auto own_queue = [&](hipStream_t* st) {
    if (hipExtStreamCreateWithCUMask(st, words, all.data()) == hipSuccess) return hipSuccess;
    (void)hipGetLastError();
    return hipStreamCreateWithFlags(st, hipStreamNonBlocking);
  };
  hipError_t e = own_queue(&L.copy);
  // CMTV_ONE_EXEC=1 (experiment): no unmasked exec queue -- every chunk on
  // the masked one (a queue fewer per lane, 16 CUs fewer for the bulk)
  if (e == hipSuccess && !ctx->one_exec) e = own_queue(&L.exec);

  if (e == hipSuccess) e = hipEventCreateWithFlags(&L.scratch.done, hipEventDisableTiming);
  if (e == hipSuccess) {
    // The reserved CUs: the masked exec stream gets every other CU, the
    // latency stream these. The driver deals a queue's CU-mask bits out
    // XCD-major round-robin -- bit i to XCD i mod 8, then to SE (i / 8) mod
    // 4, then to that SE's CU i / 32 (tools/cumask_probe.hip on MI355X:
    // bits 0..7 alone run on CU 0 of SE 0 of each XCD) -- and the dispatcher
    // deals a kernel's workgroups to the XCDs round-robin, so the reserve
    // must hold CUs on every XCD (an XCD whose share of a mask is empty runs
    // the queue on all its CUs). Taken in whole CU pairs (the pair shares
    // one instruction cache): bits 0..7 and 32..39 are CUs 0 and 1 of SE 0
    // on each XCD, then 8..15 and 40..47 (SE 1), and so on.
    std::vector<uint32_t> mask = all, lat(words, 0);
    const uint32_t reserved = reserved_cus(ctx, L.cus);
    for (uint32_t k = 0; k < reserved; k++) {
      const uint32_t pair = k / 16, cu_bit = (k / 8) % 2, xcd = k % 8;
      const uint32_t b = cu_bit * 32 + pair * 8 + xcd;
      mask[b / 32] &= ~(1u << (b % 32));
      lat[b / 32] |= 1u << (b % 32);
    }
    L.masked_waves = 8 * (L.cus - reserved);
    if (reserved == 0 || L.cus <= reserved ||
        hipExtStreamCreateWithCUMask(&L.exec_masked, words, mask.data()) != hipSuccess) {
      (void)hipGetLastError();
      L.exec_masked = nullptr;  // no masking: chunks keep the plain exec stream
    }
    if (L.exec_masked && ctx->lat_isolate) {
      if (hipExtStreamCreateWithCUMask(&L.lat, words, lat.data()) != hipSuccess ||
          hipEventCreateWithFlags(&L.lat_in, hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&L.lat_out, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        if (L.lat) (void)hipStreamDestroy(L.lat);
        L.lat = nullptr;  // latency calls keep the normal stream
      }
    }
  }
  if (e == hipSuccess && !L.exec) {
    if (L.exec_masked)
      L.exec = L.exec_masked;
    else
      e = own_queue(&L.exec);
  }
  for (int k = 0; k < kBulkSlotsMax && e == hipSuccess; k++) {
    e = hipEventCreateWithFlags(&L.slot[k].h2d, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&L.slot[k].done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&L.slot[k].prep, hipEventDisableTiming);
  }
  return e;
}

void bulk_lane_release(CmtvDev& D) {
  BulkLane& L = D.bulk;
  if (L.exec) (void)hipStreamSynchronize(L.exec);
  if (L.exec_masked) (void)hipStreamSynchronize(L.exec_masked);
  if (L.copy) (void)hipStreamSynchronize(L.copy);
  for (auto& S : L.slot) {
    S.h_in.release();
    S.h_bm.release();
    S.d_in.release();
    S.d_bm.release();
    if (S.h2d) (void)hipEventDestroy(S.h2d);
    if (S.done) (void)hipEventDestroy(S.done);
    if (S.prep) (void)hipEventDestroy(S.prep);
    S.h2d = S.done = S.prep = nullptr;
    S.pending = false;
  }
  L.scratch.buf.release();
  if (L.scratch.done) (void)hipEventDestroy(L.scratch.done);
  L.scratch.done = nullptr;
  L.scratch.used = false;
  if (L.exec == L.exec_masked) L.exec = nullptr;  // CMTV_ONE_EXEC: one stream
  if (L.exec) (void)hipStreamDestroy(L.exec);
  if (L.exec_masked) (void)hipStreamDestroy(L.exec_masked);
  if (L.copy) (void)hipStreamDestroy(L.copy);
  if (L.lat) (void)hipStreamDestroy(L.lat);
  if (L.lat_in) (void)hipEventDestroy(L.lat_in);
  if (L.lat_out) (void)hipEventDestroy(L.lat_out);
  L.exec = L.exec_masked = L.copy = L.lat = nullptr;
  L.lat_in = L.lat_out = nullptr;
}

int bulk_stage(cmtv_ctx* ctx, size_t dev, int slot, const BulkLayout& L, uint8_t** host) {
  CmtvDev& D = ctx->devs[dev];
  if (hipSetDevice(D.ordinal) != hipSuccess) return CMTV_ENODEV;
  hipError_t e = bulk_lane_init(ctx, D);
  BulkSlot& S = D.bulk.slot[slot];
  if (e == hipSuccess) e = S.h_in.ensure(L.in_bytes);
  if (e != hipSuccess) return hip_fail(e);
  *host = static_cast<uint8_t*>(S.h_in.p);
  return CMTV_OK;
}

// Where a chunk's gather + sign-bytes run: an unmasked chunk's on the lane's
// masked exec stream -- idle while no latency call is near, and a queue the
// lane already has -- so they overlap the previous chunk's keyed launch on
// exec (VerifyCommit pass 39.9 -> 39.3 ms, profiles/r06_prep_stream_ab.txt);
// a masked chunk's in line on its own stream (CMTV_PREP_STREAM=0: always in
// line)
static hipStream_t bulk_prep_stream(const cmtv_ctx* ctx, const BulkLane& BL, bool masked) {
  if (masked) return BL.exec_masked;
  return ctx->prep_stream && BL.exec_masked ? BL.exec_masked : BL.exec;
}

int bulk_prepare(cmtv_ctx* ctx, size_t dev, int slot, const BulkLayout& L, const cmtv_keyset* ks) {
  // Everything of a chunk's submission that touches only the lane (its
  // streams, its slot's buffers): the staging's H2D, the direct chunk's
  // DMAs and gather, the sign-bytes. The bulk lock orders it; the context
  // lock is not taken, so a latency call never waits behind these ~10 HIP
  // calls (round 6) -- bulk_submit_locked then enqueues the launch.
  CmtvDev& D = ctx->devs[dev];
  if (hipSetDevice(D.ordinal) != hipSuccess) return CMTV_ENODEV;
  BulkLane& BL = D.bulk;
  BulkSlot& S = BL.slot[slot];
  const size_t words = (L.m + 63) / 64;
  hipError_t e = S.d_in.ensure(L.dev_bytes);
  if (e == hipSuccess) e = S.d_bm.ensure(8 * std::max<size_t>(words, 1));
  if (e == hipSuccess) e = S.h_bm.ensure(8 * std::max<size_t>(words, 1));
  if (e != hipSuccess) return hip_fail(e);
  const bool masked = L.masked && BL.exec_masked;
  hipStream_t ex = masked ? BL.exec_masked : BL.exec;
  auto* din = static_cast<uint8_t*>(S.d_in.p);
  // H2D on the copy stream (overlaps the exec stream's previous chunk); a
  // direct chunk's per-signature data comes straight from the caller's
  // pinned arena, one DMA per span, and is laid out by k_bulk_gather
  if ((e = hipMemcpyAsync(din, S.h_in.p, L.in_bytes, hipMemcpyHostToDevice, BL.copy)) != hipSuccess) return hip_fail(e);
  if (L.direct)
    for (int k = 0; k < L.n_spans; k++)
      if ((e = hipMemcpyAsync(din + L.o_arena + L.spans[k].dev_off, L.spans[k].host, L.spans[k].bytes,
                              hipMemcpyHostToDevice, BL.copy)) != hipSuccess)
        return hip_fail(e);
  // the gather and the sign-bytes: on the prep stream for an unmasked chunk
  // (they overlap the previous chunk's keyed launch on exec: ~60 + 40 us a
  // chunk, round 6 rocprof of replay_c3_host), else in line on exec
  hipStream_t ps = bulk_prep_stream(ctx, BL, masked);
  if ((e = hipEventRecord(S.h2d, BL.copy)) != hipSuccess || (e = hipStreamWaitEvent(ps, S.h2d, 0)) != hipSuccess)
    return hip_fail(e);
  auto* off = reinterpret_cast<uint32_t*>(din + L.o_off);
  if (L.direct) {
    if (!ks) return CMTV_EINVAL;  // direct chunks are registered-key chunks
    auto* cb = reinterpret_cast<uint32_t*>(din + L.o_cbase);
    if ((e = launch_bulk_gather((uint32_t)L.n_tmpls, (uint32_t)L.m, din + L.o_desc, din + L.o_tmpl, din + L.o_arena,
                                reinterpret_cast<uint32_t*>(din + L.o_key), din + L.o_sig, off,
                                reinterpret_cast<uint32_t*>(din + L.o_tidx), din + L.o_flag,
                                reinterpret_cast<int64_t*>(din + L.o_sec), reinterpret_cast<int32_t*>(din + L.o_nanos),
                                cb, cb + L.n_tmpls, ps)) != hipSuccess)
      return hip_fail(e);
  }
  // sign-bytes from the chunk's templates into o_msg (k_sign_bytes; the
  // bulk chunks run the lane kernels, whose launches take no fused form)
  if ((e = launch_sign_bytes((uint32_t)L.m, din + L.o_tmpl, din + L.o_blob, reinterpret_cast<uint32_t*>(din + L.o_tidx),
                             din + L.o_flag, reinterpret_cast<int64_t*>(din + L.o_sec),
                             reinterpret_cast<int32_t*>(din + L.o_nanos), off, din + L.o_msg, ps)) != hipSuccess)
    return hip_fail(e);
  if (ps != ex && (e = hipEventRecord(S.prep, ps)) != hipSuccess) return hip_fail(e);
  return CMTV_OK;
}

int bulk_submit_locked(cmtv_ctx* ctx, size_t dev, int slot, const BulkLayout& L, const cmtv_keyset* ks,
                       uint32_t mode) {
  CmtvDev& D = ctx->devs[dev];
  if (D.failed) return CMTV_EHIP;  // retired by another call meanwhile
  if (hipSetDevice(D.ordinal) != hipSuccess) return CMTV_ENODEV;
  BulkLane& BL = D.bulk;
  BulkSlot& S = BL.slot[slot];
  const size_t words = (L.m + 63) / 64;
  hipError_t e;
  // near a latency call: the CU-masked stream, and batched launches sized
  // to the waves its CUs hold in one round
  const bool masked = L.masked && BL.exec_masked;
  hipStream_t ex = masked ? BL.exec_masked : BL.exec;
  auto* din = static_cast<uint8_t*>(S.d_in.p);
  auto* dbm = static_cast<uint64_t*>(S.d_bm.p);
  auto* off = reinterpret_cast<uint32_t*>(din + L.o_off);
  // the chunk's prep (bulk_prepare) ran on the prep stream: exec waits for it
  if (bulk_prep_stream(ctx, BL, masked) != ex && (e = hipStreamWaitEvent(ex, S.prep, 0)) != hipSuccess)
    return hip_fail(e);
  int rc;
  // a registered-key chunk's kernel stores its verdict words straight into
  // the slot's mapped host bitmap: no D2H between this launch and the next
  // chunk's on exec (round 6: consecutive keyed launches were 84-135 us
  // apart, ~2 ms of a 40 ms pass; CMTV_BULK_BM_DIRECT=1, measured neutral)
  uint64_t* hbm_dev = nullptr;
  if (ks && ctx->bulk_bm_direct) {
    void* q = nullptr;
    if ((e = hipHostGetDevicePointer(&q, S.h_bm.p, 0)) != hipSuccess) return hip_fail(e);
    hbm_dev = static_cast<uint64_t*>(q);
  }
  if (ks)
    rc = enqueue_verify_keyed(ctx, D, ks->dev[dev], ks->n, L.m, reinterpret_cast<uint32_t*>(din + L.o_key),
                              din + L.o_sig, din + L.o_msg, off, mode, nullptr, hbm_dev ? hbm_dev : dbm, ex,
                              &BL.scratch, nullptr, masked ? BL.masked_waves : 0);
  else
    rc = enqueue_verify(ctx, D, L.m, din + L.o_key, din + L.o_sig, din + L.o_msg, off, mode, nullptr, dbm, ex,
                        nullptr, &BL.scratch);
  if (rc != CMTV_OK) return rc;
  if ((!hbm_dev && (e = hipMemcpyAsync(S.h_bm.p, dbm, 8 * words, hipMemcpyDeviceToHost, ex)) != hipSuccess) ||
      (e = hipEventRecord(S.done, ex)) != hipSuccess)
    return hip_fail(e);
  S.pending = true;
  if (masked) ctx->stats.masked_chunks++;
  return CMTV_OK;
}

int bulk_wait(cmtv_ctx* ctx, size_t dev, int slot, const uint64_t** bitmap) {
  CmtvDev& D = ctx->devs[dev];
  BulkSlot& S = D.bulk.slot[slot];
  if (hipSetDevice(D.ordinal) != hipSuccess) return CMTV_ENODEV;
  const hipError_t e = hipEventSynchronize(S.done);
  S.pending = false;
  if (e != hipSuccess) return hip_fail(e);
  if ((long)dev == ctx->fault_sync_dev) return CMTV_EHIP;  // CMTV_FAULT_SYNC_DEV (see run_host_batch_)
  *bitmap = static_cast<const uint64_t*>(S.h_bm.p);
  return CMTV_OK;
}

void bulk_drain(cmtv_ctx* ctx) {
  for (auto& D : ctx->devs) {
    if (!D.bulk.exec) continue;
    (void)hipSetDevice(D.ordinal);
    (void)hipStreamSynchronize(D.bulk.copy);
    (void)hipStreamSynchronize(D.bulk.exec);
    if (D.bulk.exec_masked) (void)hipStreamSynchronize(D.bulk.exec_masked);
    for (auto& S : D.bulk.slot) S.pending = false;
  }
  (void)hipGetLastError();
}

void count_invalid_locked(cmtv_ctx* ctx, uint64_t n) { ctx->stats.invalid += n; }
void count_direct_locked(cmtv_ctx* ctx) { ctx->stats.direct_chunks++; }

PipeWorkspace*& pipe_workspace(cmtv_ctx* ctx) { return ctx->pipe_ws; }

}  // namespace cmtv
