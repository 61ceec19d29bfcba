// host_batch.cpp -- batches in host memory: staging and launch of a shard
// (enqueue_shard), the single-device mapped-memory call and the sharded one
// (run_host_batch), the verdict cache in front of them, templated commit
// batches, early-staged signatures and the secp256k1 host calls (messages in
// host memory, or commit signatures with templated sign-bytes).
#include <functional>

#include "runtime_state.h"
#include "shard.h"
#include "signbytes.h"
#include "verdict_bits.h"

namespace cmtv {

// SipHash-2-4 (Aumasson & Bernstein), keyed per process: the verdict cache's
// index, so a peer cannot aim many entries at one bucket.
static uint64_t rotl(uint64_t x, int b) { return (x << b) | (x >> (64 - b)); }

static uint64_t siphash24(const SipKey& key, const uint8_t* p, size_t n) {
  uint64_t v0 = 0x736f6d6570736575ull ^ key.k0, v1 = 0x646f72616e646f6dull ^ key.k1;
  uint64_t v2 = 0x6c7967656e657261ull ^ key.k0, v3 = 0x7465646279746573ull ^ key.k1;
  auto round = [&] {
    v0 += v1; v1 = rotl(v1, 13); v1 ^= v0; v0 = rotl(v0, 32);
    v2 += v3; v3 = rotl(v3, 16); v3 ^= v2;
    v0 += v3; v3 = rotl(v3, 21); v3 ^= v0;
    v2 += v1; v1 = rotl(v1, 17); v1 ^= v2; v2 = rotl(v2, 32);
  };
  const size_t full = n & ~(size_t)7;
  for (size_t i = 0; i < full; i += 8) {
    uint64_t m;
    std::memcpy(&m, p + i, 8);
    v3 ^= m;
    round();
    round();
    v0 ^= m;
  }
  uint64_t b = (uint64_t)n << 56;
  for (size_t i = full; i < n; i++) b |= (uint64_t)p[i] << (8 * (i - full));
  v3 ^= b;
  round();
  round();
  v0 ^= b;
  v2 ^= 0xff;
  round();
  round();
  round();
  round();
  return v0 ^ v1 ^ v2 ^ v3;
}

uint64_t VerdictCache::hash(const std::string& k) const {
  return siphash24(sk, reinterpret_cast<const uint8_t*>(k.data()), k.size());
}

// A batch in host memory: generic (pk rows), registered keys (key_idx into
// ks) or sr25519; messages either host-encoded (msg) or written on the
// device from per-commit CanonicalVote templates (signbytes.h).
struct HostBatch {
  size_t n = 0;
  uint32_t mode = 0;
  const uint8_t* pk = nullptr;
  const cmtv_keyset* ks = nullptr;
  const uint32_t* key_idx = nullptr;
  const uint8_t* sig = nullptr;
  const uint32_t* msg_off = nullptr;
  uint32_t msg_bound = 0;  // templated with msg_off null: every message is at most this long
  const uint8_t* msg = nullptr;
  const SbTemplate* tmpls = nullptr;
  size_t n_tmpls = 0;
  const uint8_t* blob = nullptr;
  size_t blob_len = 0;
  const uint32_t* tidx = nullptr;
  const uint8_t* tflag = nullptr;
  const int64_t* sec = nullptr;
  const int32_t* nanos = nullptr;
  // a speculative launch (commit.cpp's speculative VerifyCommit): run once
  // the batch's kernels are enqueued, before the call waits for them; its
  // answer goes to *between_ok (the caller discards the verdicts on false)
  const std::function<bool()>* between = nullptr;
  bool* between_ok = nullptr;
  void after_launch() const {
    if (between) *between_ok = (*between)();
  }
};

// Stage rows [a, b) of B on device g and enqueue sign-bytes (templated) and
// verification; verdict bytes to D.d_out (when want_valid), bitmap words to
// `bitmap` (device memory of D).
static int enqueue_shard(cmtv_ctx* ctx, size_t g, const HostBatch& B, size_t a, size_t b, bool want_valid,
                         uint64_t* bitmap, size_t& o_valid_out, bool zero_copy = false) {
  CmtvDev& D = ctx->devs[g];
  const size_t m = b - a;
  const bool keyed = B.ks != nullptr, tpl = B.msg == nullptr;
  // no offsets (verify_templated_locked: the fused small-batch path only):
  // sized by the bound, never written
  const bool no_off = tpl && !B.msg_off;
  const size_t mb = no_off ? (size_t)B.msg_bound * m : (size_t)B.msg_off[b] - B.msg_off[a];
  const size_t key_bytes = keyed ? 4 * m : 32 * m;
  // signatures first: an early-staged commit's (stage_sigs_early_locked) are
  // already there, on their way to the device
  const size_t o_sig = 0, o_key = align_up(64 * m, 256), o_off = align_up(o_key + key_bytes, 256);
  size_t o_tidx = 0, o_flag = 0, o_sec = 0, o_nanos = 0, o_tmpl = 0, o_blob = 0, in_bytes, o_msg, dev_bytes;
  const size_t tb = B.n_tmpls * sizeof(SbTemplate);
  if (tpl) {
    o_tidx = align_up(o_off + 4 * (m + 1), 256);
    o_flag = align_up(o_tidx + 4 * m, 256);
    o_sec = align_up(o_flag + m, 256);
    o_nanos = align_up(o_sec + 8 * m, 256);
    o_tmpl = align_up(o_nanos + 4 * m, 256);
    o_blob = align_up(o_tmpl + tb, 256);
    in_bytes = align_up(o_blob + B.blob_len + 16, 256);
    o_msg = in_bytes;  // device only: k_sign_bytes writes the messages here
    dev_bytes = align_up(o_msg + mb + 16, 256);
  } else {
    o_msg = align_up(o_off + 4 * (m + 1), 256);
    in_bytes = align_up(o_msg + mb + 16, 256);
    dev_bytes = in_bytes;
  }
  const size_t o_valid = 0, out_bytes = align_up(std::max<size_t>(m, 1), 256);
  o_valid_out = o_valid;
  hipError_t e;
  const uint64_t t_stage = phase_clock(ctx);
  (void)hipSetDevice(D.ordinal);
  // message lengths first: they decide the fused / zero-copy forms
  const uint32_t base = no_off ? 0u : B.msg_off[a];
  uint32_t max_len = no_off ? B.msg_bound : 0u;
  if (!no_off)
    for (size_t i = 0; i < m; i++) max_len = std::max(max_len, B.msg_off[a + i + 1] - B.msg_off[a + i]);
  // templated sign-bytes written by the verify kernel's helper wave (no
  // k_sign_bytes launch) when the batch runs a split kernel and every
  // message fits the helper's LDS slot; CMTV_NO_SB_FUSE turns it off
  const bool fuse = tpl && ctx->sb_fuse && max_len <= kSbFuseMaxMsg && (keyed ? keyed_fuse_ok(ctx, m) : fuse_ok(ctx, m));
  // a fused small batch reads its staging in mapped host memory directly
  // (CMTV_NO_ZC_IN turns it off), and so does a small plain host-API batch
  // whose messages fit the same bound (keys, signatures and messages; no
  // sign-bytes kernel writes into the staging then; CMTV_ZC_HOST_IN=0 copies
  // it). Measured on MI355X (round 4, profiles/r04_zc_host_ab.txt): host API
  // 150 0.116 -> 0.109 ms, 4,096 0.284 -> 0.269, 10,000 0.343 -> 0.326 ms.
  // Registered-key batches copy it (their signatures are early-staged past
  // the keyed row band): reading all of it in place was measured no faster
  // at 150 (p50 0.0525 vs 0.0523-0.0534 ms) and slower at 10k (0.144-0.148
  // vs 0.136-0.137 ms, kernel 0.089-0.093 vs 0.078 ms; round 5,
  // profiles/r05_zc_keyed_ab.txt), and that option was retired.
  // the signatures (and keys) staged ahead of the plan: the same bytes are
  // already in h_in (and on their way to d_in on this stream), unless a
  // buffer must grow; a batch that has them reads HBM, not its staging in place
  const bool early = D.early_src && D.early_src == B.sig + 64 * a && m <= D.early_n && in_bytes <= D.h_in.cap &&
                     dev_bytes <= D.d_in.cap;
  const bool early_pk = early && !keyed && D.early_pk && D.early_pk == B.pk + 32 * a && m == D.early_n;
  D.early_src = D.early_pk = nullptr;
  const bool zc = !early && (!keyed || ctx->keyed_zc || (ctx->bulk_now && ctx->load_zc)) && zero_copy && ctx->zc_in &&
                  (fuse || (!tpl && ctx->zc_host_in && max_len <= kSbFuseMaxMsg));
  // split: the early-staged signatures (and keys) in HBM, the rest -- the
  // fused helper's templates, flags and timestamps, ~17 bytes a signature --
  // read in place from mapped memory, so the launch waits for no second copy.
  // Measured on MI355X (tools/early_ab.sh, three alternating rounds):
  // verify_commit_10k_keyset p50 0.1435-0.1443 -> 0.1350-0.1359 ms (kernel
  // +3 us: its hash helper reads the fields over PCIe), verify_commit_10k
  // 0.293-0.303 -> 0.289-0.294 ms.
  const bool split = early && zero_copy && ctx->zc_in && fuse && (keyed || early_pk);
  HostBuf& HB = (zc || split) ? D.h_zin : D.h_in;
  if ((e = HB.ensure(in_bytes)) != hipSuccess) return hip_fail(e);
  if (!zc && (e = D.d_in.ensure(dev_bytes)) != hipSuccess) return hip_fail(e);
  if ((e = D.d_out.ensure(out_bytes)) != hipSuccess) return hip_fail(e);
  auto* hin = static_cast<uint8_t*>(HB.p);
  // a null key_idx (registered keys) means signature i is by key i, a null
  // tidx that every signature uses template 0: the fused kernels take them
  // as null, anything else gets the arrays written out
  const bool null_kidx = keyed && !B.key_idx && fuse, null_tidx = tpl && !B.tidx && fuse;
  if (keyed) {
    if (B.key_idx)
      std::memcpy(hin + o_key, B.key_idx + a, 4 * m);
    else if (!null_kidx)
      for (size_t i = 0; i < m; i++) reinterpret_cast<uint32_t*>(hin + o_key)[i] = (uint32_t)(a + i);
  } else if (!early_pk) {
    std::memcpy(hin + o_key, B.pk + 32 * a, 32 * m);
  }
  // zero-copy signatures already in the caller's cmtv_alloc_pinned memory are
  // read from there (no host copy)
  const bool sig_in_place = zc && pinned_holds_locked(ctx, B.sig + 64 * a, 64 * m);
  if (!early && !sig_in_place) std::memcpy(hin + o_sig, B.sig + 64 * a, 64 * m);
  if (no_off && !fuse) return CMTV_EINVAL;  // verify_templated_locked derives offsets for every other form
  auto* hoff = reinterpret_cast<uint32_t*>(hin + o_off);
  if (!no_off)
    for (size_t i = 0; i <= m; i++) hoff[i] = B.msg_off[a + i] - base;
  if (tpl) {
    if (B.tidx)
      std::memcpy(hin + o_tidx, B.tidx + a, 4 * m);
    else if (!null_tidx)
      std::memset(hin + o_tidx, 0, 4 * m);
    std::memcpy(hin + o_flag, B.tflag + a, m);
    std::memcpy(hin + o_sec, B.sec + a, 8 * m);
    std::memcpy(hin + o_nanos, B.nanos + a, 4 * m);
    std::memcpy(hin + o_tmpl, B.tmpls, tb);
    if (B.blob_len) std::memcpy(hin + o_blob, B.blob, B.blob_len);
  } else {
    if (mb) std::memcpy(hin + o_msg, B.msg + base, mb);
    std::memset(hin + o_msg + mb, 0, 16);
  }
  phase_add(ctx, kPhStage, t_stage);
  const uint64_t t_launch = phase_clock(ctx);
  uint8_t* din = static_cast<uint8_t*>(D.d_in.p);
  uint8_t* dmsg = din + o_msg;  // the templated sign-bytes, written by k_sign_bytes
  auto* dout = static_cast<uint8_t*>(D.d_out.p);
  // where the kernel reads the signatures and (generic) keys: HBM unless
  // the whole staging is read in place
  uint8_t* dsig = din + o_sig;
  uint8_t* dkey = din + o_key;
  if (zc || split) {
    void* p = nullptr;
    if ((e = hipHostGetDevicePointer(&p, HB.p, 0)) != hipSuccess) return hip_fail(e);
    din = static_cast<uint8_t*>(p);
    dmsg = din + o_msg;
    if (zc) dsig = din + o_sig;
    if (sig_in_place) {
      void* q = nullptr;
      if ((e = hipHostGetDevicePointer(&q, const_cast<uint8_t*>(B.sig + 64 * a), 0)) != hipSuccess) return hip_fail(e);
      dsig = static_cast<uint8_t*>(q);
    }
    if (zc || keyed) dkey = din + o_key;  // key indices (keyed) are in the mapped staging
  } else {
    const size_t from = early_pk ? o_off : early ? o_key : 0;  // what the early copy did not carry
    if ((e = hipMemcpyAsync(din + from, hin + from, in_bytes - from, hipMemcpyHostToDevice, D.stream)) != hipSuccess)
      return hip_fail(e);
  }
  SbFuse sb;
  if (fuse) {
    sb.tmpls = din + o_tmpl;
    sb.blob = din + o_blob;
    sb.tidx = null_tidx ? nullptr : reinterpret_cast<uint32_t*>(din + o_tidx);
    sb.flag = din + o_flag;
    sb.sec = reinterpret_cast<int64_t*>(din + o_sec);
    sb.nanos = reinterpret_cast<int32_t*>(din + o_nanos);
    ctx->stats.fused_sign_bytes++;
  } else if (tpl) {
    // k_sign_bytes also writes the 16 zero bytes after the last message
    if ((e = launch_sign_bytes((uint32_t)m, din + o_tmpl, din + o_blob, reinterpret_cast<uint32_t*>(din + o_tidx),
                               din + o_flag, reinterpret_cast<int64_t*>(din + o_sec),
                               reinterpret_cast<int32_t*>(din + o_nanos), reinterpret_cast<uint32_t*>(din + o_off),
                               dmsg, D.stream)) != hipSuccess)
      return hip_fail(e);
  }
  uint8_t* dv = want_valid ? dout + o_valid : nullptr;
  int rc;
  if (keyed)
    rc = enqueue_verify_keyed(ctx, D, B.ks->dev[g], B.ks->n, m,
                              null_kidx ? nullptr : reinterpret_cast<uint32_t*>(dkey), dsig,
                              tpl ? dmsg : din + o_msg, reinterpret_cast<uint32_t*>(din + o_off), B.mode, dv, bitmap,
                              D.stream, nullptr, fuse ? &sb : nullptr);
  else
    rc = enqueue_verify(ctx, D, m, dkey, dsig, din + o_msg, reinterpret_cast<uint32_t*>(din + o_off), B.mode, dv,
                        bitmap, D.stream, fuse ? &sb : nullptr);
  phase_add(ctx, kPhLaunch, t_launch);
  return rc;
}

// Verdicts of a host batch, sharded over the context's live devices. Caller
// holds the lock. On a device's HIP error *bad_dev names it.
// Wait for a tagged row launch (CmtvDev::tag_used) of n signatures on device
// D: poll the entries until each carries the call's tag, asking the stream
// every 256 polls so that an error ends the wait; a launch that finished with
// an entry untagged (which cannot happen) is an error, not a hang.
// A small host batch's wait for its stream: hipStreamSynchronize, or with
// spin_wait (CMTV_SPIN_WAIT=1, A/B knob) a busy poll of hipStreamQuery that
// keeps the calling thread on its CPU
static hipError_t wait_stream(const cmtv_ctx* ctx, hipStream_t s) {
  if (!ctx->spin_wait) return hipStreamSynchronize(s);
  for (;;) {
    const hipError_t q = hipStreamQuery(s);
    if (q != hipErrorNotReady) return q;
  }
}

static hipError_t wait_row_tags(CmtvDev& D, size_t n) {
  const uint64_t* e = static_cast<const uint64_t*>(D.h_tags.p);
  const size_t n32 = (n + D.tag_width - 1) / D.tag_width;  // entries
  size_t j = 0;
  auto scan = [&] {
    while (j < n32 && (uint32_t)(__atomic_load_n(e + j, __ATOMIC_ACQUIRE) >> 32) == D.tag_seq) j++;
    return j == n32;
  };
  for (uint32_t spin = 1;; spin++) {
    if (scan()) return hipSuccess;
    if ((spin & 255) == 0) {
      const hipError_t q = hipStreamQuery(D.stream);
      if (q == hipSuccess) return scan() ? hipSuccess : hipErrorLaunchFailure;
      if (q != hipErrorNotReady) return q;
    }
  }
}

static int run_host_batch_(cmtv_ctx* ctx, const HostBatch& B, uint8_t* out_valid, uint64_t* out_bitmap,
                           long* bad_dev) {
  const size_t n = B.n;
  if (n == 0) return CMTV_OK;
  const std::vector<size_t>& live = ctx->live;
  if (live.empty()) return CMTV_ENODEV;
  const ShardPlan P = plan_shards(n, live.size(), ctx->shard_min);
  const size_t words = (n + 63) / 64;
  hipError_t e;
  const size_t d0 = live[0];
  if (P.G == 1 && n <= ctx->zc_max) {
    // one device, a small batch: the verify kernel writes the bitmap into
    // mapped host memory, so the call is H2D + (sign-bytes) + verify + sync
    CmtvDev& D = ctx->devs[d0];
    *bad_dev = (long)d0;
    (void)hipSetDevice(D.ordinal);
    // the previous polled launch read h_zin: it must be done before the
    // staging below overwrites it
    if ((e = settle_polled(D)) != hipSuccess) return hip_fail(e);
    if ((e = D.h_zc.ensure(8 * words)) != hipSuccess) return hip_fail(e);
    void* dzc = nullptr;
    if ((e = hipHostGetDevicePointer(&dzc, D.h_zc.p, 0)) != hipSuccess) return hip_fail(e);
    // a row launch tags its bitmap words (kernels.h RowSlot; CMTV_HOST_POLL=0:
    // it writes the bitmap and the call waits for the stream)
    if (ctx->host_poll && !D.d_tags) {
      void* dt = nullptr;
      if ((e = D.h_tags.ensure(8 * kTagEntries)) != hipSuccess) return hip_fail(e);
      std::memset(D.h_tags.p, 0, 8 * kTagEntries);
      if ((e = hipHostGetDevicePointer(&dt, D.h_tags.p, 0)) != hipSuccess) return hip_fail(e);
      D.d_tags = static_cast<uint64_t*>(dt);
    }
    // ... but not beside a pipeline call (bulk_now): polled under a configs[2]
    // load the 150-validator call's p99 was 1.05-1.11 ms against 0.148 ms
    // waiting for the stream (round 6, tools/gpu_r6o.sh)
    const bool poll = ctx->host_poll && !(ctx->bulk_now && ctx->load_nopoll);
    if (poll && ++D.tag_seq == 0) D.tag_seq = 1;
    D.tag_arm = poll ? D.d_tags : nullptr;
    D.tag_used = false;
    size_t o_valid = 0;
    // CMTV_CALL_TRACE: the device time of this call's work, between two events
    if (ctx->call_trace) {
      if (!ctx->trace_ev[0]) {
        (void)hipEventCreate(&ctx->trace_ev[0]);
        (void)hipEventCreate(&ctx->trace_ev[1]);
      }
      (void)hipEventRecord(ctx->trace_ev[0], D.stream);
    }
    const int rc = enqueue_shard(ctx, d0, B, 0, n, false, static_cast<uint64_t*>(dzc), o_valid, true);
    if (ctx->call_trace) (void)hipEventRecord(ctx->trace_ev[1], D.stream);
    D.tag_arm = nullptr;
    if (rc != CMTV_OK) return rc;
    B.after_launch();
    if (D.tag_used) {  // settled by the next call (settle_polled)
      if (!D.poll_ev && (e = hipEventCreateWithFlags(&D.poll_ev, hipEventDisableTiming)) != hipSuccess)
        return hip_fail(e);
      if ((e = hipEventRecord(D.poll_ev, D.stream)) != hipSuccess) return hip_fail(e);
      D.poll_pending = true;
    }
    const uint64_t t_wait = phase_clock(ctx);
    if (ctx->call_trace) ctx->trace_launch = call_trace_now();
    if ((e = D.tag_used ? wait_row_tags(D, n) : wait_stream(ctx, D.stream)) != hipSuccess) return hip_fail(e);
    if (ctx->call_trace) {
      ctx->trace_wait = call_trace_now();
      float ms = 0;
      if (!D.tag_used && hipEventElapsedTime(&ms, ctx->trace_ev[0], ctx->trace_ev[1]) == hipSuccess)
        ctx->trace_dev_ns = (uint64_t)(ms * 1e6f);
      else
        ctx->trace_dev_ns = 0;
    }
    uint64_t* bm = static_cast<uint64_t*>(D.h_zc.p);
    if (D.tag_used) {
      ctx->stats.polled_calls++;
      const uint64_t* tg = static_cast<const uint64_t*>(D.h_tags.p);
      if (D.tag_width == 32) {
        const size_t n32 = (n + 31) / 32;
        for (size_t w = 0; w < words; w++)
          bm[w] = (tg[2 * w] & 0xFFFFFFFFull) | (2 * w + 1 < n32 ? (tg[2 * w + 1] & 0xFFFFFFFFull) << 32 : 0);
      } else {
        const size_t n16 = (n + 15) / 16;
        for (size_t w = 0; w < words; w++) {
          uint64_t x = 0;
          for (size_t k = 0; k < 4 && 4 * w + k < n16; k++) x |= (tg[4 * w + k] & 0xFFFFull) << (16 * k);
          bm[w] = x;
        }
      }
    }
    phase_add(ctx, kPhWait, t_wait);
    const uint64_t t_post = phase_clock(ctx);
    if ((long)d0 == ctx->fault_sync_dev) {  // CMTV_FAULT_SYNC_DEV (see below)
      ctx->stats.faults_injected++;
      return CMTV_EHIP;
    }
    *bad_dev = -1;
    harvest(ctx, false);
    (void)hipSetDevice(D.ordinal);
    ctx->stats.invalid += bitmap_tail(bm, n, out_bitmap, out_valid);
    phase_add(ctx, kPhPost, t_post);
    return CMTV_OK;
  }
  // devices in the gather: the shards' devices, or with RCCL every rank of
  // the communicator (a rank without a shard contributes zero words)
  const size_t GG = P.G == 1 ? 1 : (ctx->rccl ? live.size() : P.G);
  uint64_t* bufs[kMaxDevices];
  for (size_t g = 0; g < GG; g++) {
    CmtvDev& D = ctx->devs[live[g]];
    *bad_dev = (long)live[g];
    (void)hipSetDevice(D.ordinal);
    if ((e = D.d_all.ensure(8 * std::max<size_t>(GG * P.W, 1))) != hipSuccess) return hip_fail(e);
    bufs[g] = static_cast<uint64_t*>(D.d_all.p);
  }
  size_t o_valid = 0;
  for (size_t g = 0; g < GG; g++) {
    const size_t a = P.lo(g, n), b = P.hi(g, n);
    *bad_dev = (long)live[g];
    if (a == b) {
      // an empty shard still takes part in the gather
      (void)hipSetDevice(ctx->devs[live[g]].ordinal);
      if ((e = hipMemsetAsync(bufs[g] + g * P.W, 0, 8 * P.W, ctx->devs[live[g]].stream)) != hipSuccess)
        return hip_fail(e);
      continue;
    }
    const int rc = enqueue_shard(ctx, live[g], B, a, b, P.G == 1, bufs[g] + g * P.W, o_valid);
    if (rc != CMTV_OK) return rc;
  }
  *bad_dev = -1;
  B.after_launch();
  if (P.G > 1) {
    ctx->stats.sharded_calls++;
    const int rc = gather_bitmaps(ctx, live.data(), GG, P.W, bufs);
    if (rc != CMTV_OK) return rc;
  }
  // results from the first live device: verdict bytes + bitmap (one device)
  // or the gathered bitmap (several)
  CmtvDev& D0 = ctx->devs[d0];
  (void)hipSetDevice(D0.ordinal);
  const size_t o_bm = 0, o_v = align_up(8 * words, 256);
  const size_t out_bytes = P.G == 1 ? align_up(o_v + n, 256) : 8 * words;
  if ((e = D0.h_out.ensure(out_bytes)) != hipSuccess) return hip_fail(e);
  auto* hout = static_cast<uint8_t*>(D0.h_out.p);
  if ((e = hipMemcpyAsync(hout + o_bm, bufs[0], 8 * words, hipMemcpyDeviceToHost, D0.stream)) != hipSuccess)
    return hip_fail(e);
  if (P.G == 1 &&
      (e = hipMemcpyAsync(hout + o_v, static_cast<uint8_t*>(D0.d_out.p) + o_valid, n, hipMemcpyDeviceToHost,
                          D0.stream)) != hipSuccess)
    return hip_fail(e);
  const uint64_t t_wait = phase_clock(ctx);
  for (size_t g = 0; g < GG; g++) {
    *bad_dev = (long)live[g];
    (void)hipSetDevice(ctx->devs[live[g]].ordinal);
    if ((e = hipStreamSynchronize(ctx->devs[live[g]].stream)) != hipSuccess) return hip_fail(e);
    // CMTV_FAULT_SYNC_DEV: this device's work "failed" after its launch
    if ((long)live[g] == ctx->fault_sync_dev) {
      ctx->stats.faults_injected++;
      return CMTV_EHIP;
    }
  }
  *bad_dev = -1;
  phase_add(ctx, kPhWait, t_wait);
  const uint64_t t_post = phase_clock(ctx);
  (void)hipSetDevice(D0.ordinal);
  harvest(ctx, false);
  (void)hipSetDevice(D0.ordinal);
  uint64_t* bm = reinterpret_cast<uint64_t*>(hout + o_bm);
  // one device: the verdict bytes are the kernel's own, not the bitmap's
  ctx->stats.invalid += bitmap_tail(bm, n, out_bitmap, P.G == 1 ? nullptr : out_valid);
  if (out_valid && P.G == 1) std::memcpy(out_valid, hout + o_v, n);
  phase_add(ctx, kPhPost, t_post);
  return CMTV_OK;
}

static void drain(cmtv_ctx* ctx) {
  // work already enqueued for other shards still reads the pinned staging
  // the next call refills: drain it before returning or retrying
  for (auto& D : ctx->devs) {
    (void)hipSetDevice(D.ordinal);
    (void)hipStreamSynchronize(D.stream);
  }
  (void)hipGetLastError();
}

static int run_host_batch(cmtv_ctx* ctx, const HostBatch& B, uint8_t* out_valid, uint64_t* out_bitmap) {
  int rc = CMTV_OK;
  // every launch of this call is waited for before it returns (or drained)
  struct HostSync {
    cmtv_ctx* c;
    explicit HostSync(cmtv_ctx* x) : c(x) { c->host_sync = true; }
    ~HostSync() { c->host_sync = false; }
  } host_sync(ctx);
  // a device error retires that device and re-plans the batch over the
  // others, once per surviving device at most
  for (size_t attempt = 0; attempt < ctx->devs.size(); attempt++) {
    long bad = -1;
    rc = run_host_batch_(ctx, B, out_valid, out_bitmap, &bad);
    if (rc == CMTV_OK) break;
    drain(ctx);
    // only a device's own HIP error retires it (not CMTV_FAULT_AT, which
    // stands for a failure of the call, nor an allocation failure)
    const bool injected = ctx->fault_pending;
    ctx->fault_pending = false;
    if (rc != CMTV_EHIP || injected || bad < 0 || ctx->live.size() < 2) break;
    retire_device(ctx, (size_t)bad);
    ctx->stats.reshards++;
  }
  for (auto& D : ctx->devs) D.early_src = nullptr;  // used by this batch or never
  (void)hipSetDevice(ctx->devs[ctx->live.empty() ? 0 : ctx->live[0]].ordinal);
  return rc;
}

static const uint8_t kNoMessageBytes = 0;

int verify_host_device(cmtv_ctx* ctx, size_t n, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg,
                       const uint32_t* msg_off, uint32_t mode, uint8_t* out_valid, uint64_t* out_bitmap,
                       const cmtv_keyset* ks, const uint32_t* key_idx) {
  if (!msg) msg = &kNoMessageBytes;  // all messages empty (a null msg selects templated sign-bytes)
  HostBatch B;
  B.n = n;
  B.mode = mode;
  B.pk = pk;
  B.ks = ks;
  B.key_idx = key_idx;
  B.sig = sig;
  B.msg = msg;
  B.msg_off = msg_off;
  return run_host_batch(ctx, B, out_valid, out_bitmap);
}

bool cache_enabled(const cmtv_ctx* ctx) { return ctx->cache.cap != 0; }

int verify_host_locked(cmtv_ctx* ctx, size_t n, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg,
                       const uint32_t* msg_off, uint32_t mode, uint8_t* out_valid, uint64_t* out_bitmap) {
  if (n == 0) return CMTV_OK;
  if (!ctx->cache.cap) return verify_host_device(ctx, n, pk, sig, msg, msg_off, mode, out_valid, out_bitmap);
  // cache lookups; the misses go to the device as one compacted batch
  std::vector<uint8_t> valid(n);
  std::vector<size_t> miss;
  std::vector<uint64_t> hs(n);
  std::vector<std::string> keys(n);
  for (size_t i = 0; i < n; i++) {
    VerdictCache::make_key(keys[i], mode, pk + 32 * i, sig + 64 * i, msg + msg_off[i], msg_off[i + 1] - msg_off[i]);
    hs[i] = ctx->cache.hash(keys[i]);
    const int v = ctx->cache.find(hs[i], keys[i]);
    if (v < 0)
      miss.push_back(i);
    else
      valid[i] = (uint8_t)v;
  }
  ctx->stats.cache_hits += n - miss.size();
  if (!miss.empty()) {
    const size_t m = miss.size();
    std::vector<uint8_t> mpk(32 * m), msg_(64 * m), mmsg, mv(m);
    std::vector<uint32_t> moff(m + 1, 0);
    for (size_t j = 0; j < m; j++) {
      const size_t i = miss[j];
      std::memcpy(&mpk[32 * j], pk + 32 * i, 32);
      std::memcpy(&msg_[64 * j], sig + 64 * i, 64);
      mmsg.insert(mmsg.end(), msg + msg_off[i], msg + msg_off[i + 1]);
      moff[j + 1] = (uint32_t)mmsg.size();
    }
    if (mmsg.empty()) mmsg.push_back(0);
    const int rc = verify_host_device(ctx, m, mpk.data(), msg_.data(), mmsg.data(), moff.data(), mode, mv.data(),
                                      nullptr);
    if (rc != CMTV_OK) return rc;
    for (size_t j = 0; j < m; j++) {
      const size_t i = miss[j];
      valid[i] = mv[j];
      ctx->cache.insert(hs[i], std::move(keys[i]), mv[j]);
    }
  }
  if (out_valid) std::memcpy(out_valid, valid.data(), n);
  if (out_bitmap) bitmap_pack(valid.data(), n, out_bitmap);
  return CMTV_OK;
}

int verify_templated_locked(cmtv_ctx* ctx, size_t n, const uint8_t* pk, const uint8_t* sig, const uint32_t* msg_off,
                            const void* tmpls, size_t n_tmpls, const uint8_t* blob, size_t blob_len,
                            const uint32_t* tidx, const uint8_t* commit_flag, const int64_t* sec,
                            const int32_t* nanos, uint32_t mode, uint8_t* out_valid, const cmtv_keyset* ks,
                            const uint32_t* key_idx, uint32_t msg_bound, const std::function<bool()>* between,
                            bool* between_ok) {
  // no offsets: the fused kernels of a small single-device batch build every
  // message from its template and never read them (enqueue_shard); any other
  // form gets them derived here, exactly as sb_msg_len gives them
  std::vector<uint32_t> off_v;
  if (!msg_off) {
    const bool fused_small = ctx->live.size() == 1 && n <= ctx->zc_max && ctx->sb_fuse && msg_bound <= kSbFuseMaxMsg &&
                             (ks ? keyed_fuse_ok(ctx, n) : fuse_ok(ctx, n));
    if (!fused_small) {
      off_v.resize(n + 1);
      uint64_t o = 0;
      const auto* tp = static_cast<const SbTemplate*>(tmpls);
      for (size_t i = 0; i < n; i++) {
        off_v[i] = (uint32_t)o;
        o += sb_msg_len(tp[tidx ? tidx[i] : 0], commit_flag[i] != 0, sec[i], nanos[i]);
      }
      if (o + 16 >= (1ull << 31)) return CMTV_EINVAL;
      off_v[n] = (uint32_t)o;
      msg_off = off_v.data();
    }
  }
  HostBatch B;
  B.n = n;
  B.mode = mode;
  B.pk = ks ? nullptr : pk;
  B.ks = ks;
  B.key_idx = key_idx;
  B.sig = sig;
  B.msg_off = msg_off;
  B.msg_bound = msg_bound;
  B.tmpls = static_cast<const SbTemplate*>(tmpls);
  B.n_tmpls = n_tmpls;
  B.blob = blob;
  B.blob_len = blob_len;
  B.tidx = tidx;
  B.tflag = commit_flag;
  B.between = between;
  B.between_ok = between_ok;
  B.sec = sec;
  B.nanos = nanos;
  return run_host_batch(ctx, B, out_valid, nullptr);
}

// A single-commit VerifyCommit on one device with registered keys spends
// ~25 us planning 10k signatures before its staging is copied: its
// signatures (the bulk of the staging) go to the device first, so their H2D
// copy overlaps the plan. Their bytes are only used if the batch that
// follows stages exactly those signatures on this device (enqueue_shard);
// otherwise they are overwritten unused.
int stage_sigs_early_locked(cmtv_ctx* ctx, const uint8_t* sigs, size_t n, const uint8_t* pk) {
  const uint64_t t0 = phase_clock(ctx);
  struct Done {
    cmtv_ctx* c;
    uint64_t t;
    ~Done() { phase_add(c, kPhEarly, t); }
  } done{ctx, t0};
  clear_early_locked(ctx);  // whatever returns below stages nothing
  if (n == 0 || n > ctx->zc_max || ctx->live.size() != 1 || !ctx->early_sigs) return CMTV_OK;
  // the generic row kernels read their staging from mapped memory instead
  // (a copy's latency is most of their call); the quad-family forms gain the
  // HBM reads (10k: kernel 0.255 ms zero-copy, 0.220 ms from HBM)
  if (pk && (ed_form(ctx, n) == kFormRow4 || ed_form(ctx, n) == kFormRow)) return CMTV_OK;
  // nor is the copy worth its own latency for the keyed row kernel's
  // commits (150 validators: p50 0.0566 with it, 0.0534 without)
  if (!pk && keyed_form(ctx, n) == kKeyedRow) return CMTV_OK;
  // nor beside a pipeline call (bulk_now): the copy would queue behind its DMAs
  if (!pk && ((ctx->bulk_now && ctx->load_zc) || ctx->keyed_zc)) return CMTV_OK;
  CmtvDev& D = ctx->devs[ctx->live[0]];
  if (hipSetDevice(D.ordinal) != hipSuccess) return CMTV_ENODEV;
  hipError_t e;
  // the previous polled launch may still read h_in's neighbour h_zin only,
  // but settle it anyway so the buffers below are never in use
  if ((e = settle_polled(D)) != hipSuccess) return hip_fail(e);
  // room for any layout of n signatures that can follow (keys, offsets,
  // templates, sign-bytes), so enqueue_shard never reallocates under the copy
  const size_t in_cap = 136 * n + 64 * 1024, dev_cap = in_cap + 400 * n;
  if ((e = D.h_in.ensure(in_cap)) != hipSuccess) return hip_fail(e);
  if ((e = D.d_in.ensure(dev_cap)) != hipSuccess) return hip_fail(e);
  // the keys where enqueue_shard's layout puts them for m = n signatures
  const size_t o_key = align_up(64 * n, 256);
  auto* hin = static_cast<uint8_t*>(D.h_in.p);
  auto* din = static_cast<uint8_t*>(D.d_in.p);
  // arrays in the caller's cmtv_alloc_pinned memory go to the device by DMA
  // straight from there (no host copy: 640 KB of signatures at 10k); the
  // others through h_in as before
  const bool sig_pinned = pinned_holds_locked(ctx, sigs, 64 * n);
  const bool pk_pinned = pk && pinned_holds_locked(ctx, pk, 32 * n);
  if (!sig_pinned) std::memcpy(hin, sigs, 64 * n);
  if (pk && !pk_pinned) std::memcpy(hin + o_key, pk, 32 * n);
  if (!sig_pinned && pk && !pk_pinned) {  // one copy of both
    e = hipMemcpyAsync(din, hin, o_key + 32 * n, hipMemcpyHostToDevice, D.stream);
  } else {
    e = hipMemcpyAsync(din, sig_pinned ? sigs : hin, 64 * n, hipMemcpyHostToDevice, D.stream);
    if (e == hipSuccess && pk)
      e = hipMemcpyAsync(din + o_key, pk_pinned ? pk : hin + o_key, 32 * n, hipMemcpyHostToDevice, D.stream);
  }
  if (e != hipSuccess) return hip_fail(e);
  D.early_src = sigs;
  D.early_pk = pk;
  D.early_n = n;
  return CMTV_OK;
}

// What every secp256k1 host batch does once its inputs are on their way to
// D.secp_in on D.stream: the launch (enqueue(bitmap, stream)), the verdict
// bitmap back, the wait for it.
template <class Enqueue>
static int secp_finish(cmtv_ctx* ctx, CmtvDev& D, size_t n, uint8_t* out_valid, uint64_t* out_bitmap, Enqueue enqueue) {
  hipStream_t s = D.stream;
  auto* dbm = static_cast<uint64_t*>(D.secp_out.p);
  const int rc = enqueue(dbm, s);
  if (rc != CMTV_OK) {
    (void)hipStreamSynchronize(s);  // the copies read the caller's buffers (or the staging)
    return rc;
  }
  std::vector<uint64_t> bm((n + 63) / 64);
  hipError_t e;
  if ((e = hipMemcpyAsync(bm.data(), dbm, 8 * bm.size(), hipMemcpyDeviceToHost, s)) != hipSuccess) return hip_fail(e);
  if ((e = wait_stream(ctx, s)) != hipSuccess) return hip_fail(e);
  // (the kernel's ballot words hold 0 for the lanes past n: the mask changes nothing)
  ctx->stats.invalid += bitmap_tail(bm.data(), n, out_bitmap, out_valid);
  return CMTV_OK;
}

// Host buffers in, verdicts out, on devs[0] (caller holds the context lock):
// one staging block keys | sig | off | msg, the verdict bitmap back. keys: n x
// 33 key bytes, or with ks n u32 indices of registered keys (the caller has
// checked every index against the key set).
int verify_secp_host_locked(cmtv_ctx* ctx, const cmtv_secp_keyset* ks, size_t n, const void* keys, const uint8_t* sig,
                            const uint8_t* msg, const uint32_t* msg_off, uint8_t* out_valid, uint64_t* out_bitmap) {
  CmtvDev& D = ctx->devs[0];
  const size_t msg_bytes = msg_off[n], key_bytes = (ks ? 4 : 33) * n;
  const size_t o_sig = align_up(key_bytes, 16), o_off = o_sig + 64 * n, o_msg = o_off + 4 * (n + 1);
  hipError_t e;
  // +4: the kernel's aligned reads end inside the last message byte's word
  if ((e = D.secp_in.ensure(o_msg + msg_bytes + 4)) != hipSuccess) return hip_fail(e);
  if ((e = D.secp_out.ensure(8 * ((n + 63) / 64))) != hipSuccess) return hip_fail(e);
  auto* din = static_cast<uint8_t*>(D.secp_in.p);
  hipStream_t s = D.stream;
  if ((e = hipMemcpyAsync(din, keys, key_bytes, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e);
  if ((e = hipMemcpyAsync(din + o_sig, sig, 64 * n, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e);
  if ((e = hipMemcpyAsync(din + o_off, msg_off, 4 * (n + 1), hipMemcpyHostToDevice, s)) != hipSuccess)
    return hip_fail(e);
  if (msg_bytes && (e = hipMemcpyAsync(din + o_msg, msg, msg_bytes, hipMemcpyHostToDevice, s)) != hipSuccess)
    return hip_fail(e);
  const auto* d_off = reinterpret_cast<const uint32_t*>(din + o_off);
  return secp_finish(ctx, D, n, out_valid, out_bitmap, [&](uint64_t* dbm, hipStream_t st) {
    return ks ? enqueue_verify_secp_keyed(ctx, D, ks, n, reinterpret_cast<const uint32_t*>(din), din + o_sig,
                                          din + o_msg, d_off, nullptr, dbm, st)
              : enqueue_verify_secp(ctx, D, n, din, din + o_sig, din + o_msg, d_off, nullptr, dbm, st);
  });
}

// Commit signatures over secp256k1 keys with templated sign-bytes
// (runtime_internal.h): one staging block
//   sec i64 | nanos i32 | tidx u32 | key_idx u32 (registered keys) | off u32
//   (n + 1, non-fused only) | templates | sig | pk (n x 33) | flag | blob
// with the 8-byte array first and the 4-byte ones next, so every array the
// kernels read as int64 / int32 is aligned whatever n is; on the device the
// non-fused route's messages follow it. r.bulk: the fused registered-key
// route may take the batched kernel (launch.cpp enqueue_verify_secp_keyed).
int verify_secp_templated_locked(cmtv_ctx* ctx, const SecpTemplated& r, uint8_t* out_valid) {
  const size_t n = r.n, n_tmpls = r.n_tmpls, blob_len = r.blob_len;
  const cmtv_secp_keyset* ks = r.ks;
  const uint32_t* tidx = r.tidx;
  if (n == 0) return CMTV_OK;
  if (!r.sig || !r.tmpls || !n_tmpls || !r.commit_flag || !r.sec || !r.nanos || (ks ? !r.key_idx : !r.pk33))
    return CMTV_EINVAL;
  if (ctx->devs.empty() || ctx->devs[0].failed) return CMTV_ENODEV;
  CmtvDev& D = ctx->devs[0];
  (void)hipSetDevice(D.ordinal);
  const auto* tp = static_cast<const SbTemplate*>(r.tmpls);
  // message lengths: they decide the route, and give the non-fused route's offsets
  uint32_t max_len = 0;
  uint64_t total = 0;
  for (size_t i = 0; i < n; i++) {
    const uint32_t ti = tidx ? tidx[i] : 0u;
    if (ti >= n_tmpls) return CMTV_EINVAL;
    if (ks && r.key_idx[i] >= ks->n) return CMTV_EINVAL;
    const uint32_t len = sb_msg_len(tp[ti], r.commit_flag[i] != 0, r.sec[i], r.nanos[i]);
    max_len = std::max(max_len, len);
    total += len;
  }
  if (total + 16 >= (1ull << 31)) return CMTV_EINVAL;
  const bool fuse = ctx->sb_fuse && max_len <= kSbFuseMaxMsg;
  static_assert(sizeof(SbTemplate) % 4 == 0, "the arrays after the templates stay 4-byte aligned");
  const size_t tb = n_tmpls * sizeof(SbTemplate);
  const size_t o_sec = 0, o_nanos = o_sec + 8 * n, o_tidx = o_nanos + 4 * n, o_kidx = o_tidx + 4 * n;
  const size_t o_off = o_kidx + (ks ? 4 * n : 0), o_tmpl = o_off + (fuse ? 0 : 4 * (n + 1));
  const size_t o_sig = o_tmpl + tb, o_pk = o_sig + 64 * n, o_flag = o_pk + (ks ? 0 : 33 * n), o_blob = o_flag + n;
  // +16: the template runs are fetched in aligned words (LdsBytes::copy)
  const size_t in_bytes = align_up(o_blob + blob_len + 16, 16);
  // k_sign_bytes writes 16 zero bytes after the last message
  const size_t o_msg = in_bytes, dev_bytes = fuse ? in_bytes : align_up(o_msg + total + 16 + 4, 16);
  hipError_t e;
  if ((e = D.secp_in.ensure(dev_bytes)) != hipSuccess) return hip_fail(e);
  if ((e = D.secp_out.ensure(8 * ((n + 63) / 64))) != hipSuccess) return hip_fail(e);
  if (D.secp_stage.size() < in_bytes) D.secp_stage.resize(in_bytes);
  uint8_t* h = D.secp_stage.data();
  std::memcpy(h + o_sec, r.sec, 8 * n);
  std::memcpy(h + o_nanos, r.nanos, 4 * n);
  if (tidx)
    std::memcpy(h + o_tidx, tidx, 4 * n);
  else
    std::memset(h + o_tidx, 0, 4 * n);
  if (ks) std::memcpy(h + o_kidx, r.key_idx, 4 * n);
  if (!fuse) {
    uint32_t o = 0;
    for (size_t i = 0; i <= n; i++) {
      std::memcpy(h + o_off + 4 * i, &o, 4);
      if (i < n) o += sb_msg_len(tp[tidx ? tidx[i] : 0u], r.commit_flag[i] != 0, r.sec[i], r.nanos[i]);
    }
  }
  std::memcpy(h + o_tmpl, r.tmpls, tb);
  std::memcpy(h + o_sig, r.sig, 64 * n);
  if (!ks) std::memcpy(h + o_pk, r.pk33, 33 * n);
  std::memcpy(h + o_flag, r.commit_flag, n);
  if (blob_len) std::memcpy(h + o_blob, r.blob, blob_len);
  std::memset(h + o_blob + blob_len, 0, in_bytes - o_blob - blob_len);
  auto* din = static_cast<uint8_t*>(D.secp_in.p);
  if ((e = hipMemcpyAsync(din, h, in_bytes, hipMemcpyHostToDevice, D.stream)) != hipSuccess) return hip_fail(e);
  SbFuse sb;
  sb.tmpls = din + o_tmpl;
  sb.blob = din + o_blob;
  sb.tidx = reinterpret_cast<const uint32_t*>(din + o_tidx);
  sb.flag = din + o_flag;
  sb.sec = reinterpret_cast<const int64_t*>(din + o_sec);
  sb.nanos = reinterpret_cast<const int32_t*>(din + o_nanos);
  return secp_finish(ctx, D, n, out_valid, nullptr, [&](uint64_t* dbm, hipStream_t s) {
    return enqueue_verify_secp_templated(ctx, D, n, din + o_pk, ks, reinterpret_cast<const uint32_t*>(din + o_kidx),
                                         din + o_sig, sb, max_len, reinterpret_cast<const uint32_t*>(din + o_off),
                                         din + o_msg, nullptr, dbm, s, r.bulk);
  });
}

}  // namespace cmtv
