// launch.cpp -- the three verification launchers (generic Ed25519 / sr25519,
// registered keys, secp256k1): form selection is runtime_state.h's, here are
// the row kernels' bitmap ring, the lane scratch hand-over and the
// bookkeeping every launch shares.
#include "runtime_state.h"

namespace cmtv {

// What every verification call does around its launches: the device's
// completed timing pairs are harvested, one call in timing_every is timed
// (event begin before the first launch, end after the scratch release), and
// the launch and call counters are bumped.
struct LaunchScope {
  cmtv_ctx* ctx;
  CmtvDev& D;
  hipStream_t s;
  Timing::Pair tp{};
  bool timed = false;
  hipError_t begin() {
    D.timing.harvest(ctx->stats, D.device_ms, D.timed_calls, false);
    timed = ctx->timing_every && D.timing_seq++ % ctx->timing_every == 0;
    return timed ? D.timing.begin(tp, s) : hipSuccess;
  }
  // one launch's result: counted, or the call's timing pair abandoned
  hipError_t launched(hipError_t e) {
    if (e != hipSuccess) {
      D.timing.abandon(tp);
      return e;
    }
    ctx->stats.kernel_launches++;
    D.launches++;
    return hipSuccess;
  }
  // the lane scratch (when the call took it) handed on, then the timing end
  int finish(size_t n, Scratch* lane_scratch) {
    hipError_t e;
    if (lane_scratch && (e = release_scratch(*lane_scratch, s)) != hipSuccess) return hip_fail(e);
    if (timed && (e = D.timing.end(tp, s)) != hipSuccess) return hip_fail(e);
    ctx->stats.calls++;
    ctx->stats.signatures += n;
    D.calls++;
    D.signatures += n;
    return CMTV_OK;
  }
  // the end of a call that verifies nothing (test-data generation): timed
  // like the others, not counted among the verification calls
  int finish_uncounted() {
    hipError_t e;
    if (timed && (e = D.timing.end(tp, s)) != hipSuccess) return hip_fail(e);
    return CMTV_OK;
  }
};

// An armed host batch's tagged bitmap (CmtvDev::tag_arm) taken by a launch:
// entries of `width` signatures, polled by the call (wait_row_tags).
static void take_tags(CmtvDev& D, RowSlot& slot, uint32_t width) {
  slot.tagged = D.tag_arm;
  slot.seq = D.tag_seq;
  D.tag_used = true;
  D.tag_width = width;
}

// CMTV_FAULT_AT: true when this verification launch is the one to fail
bool fault_hit(cmtv_ctx* ctx) {
  ctx->launch_seq++;
  if (ctx->fault_at && ctx->launch_seq == ctx->fault_at) {
    ctx->stats.faults_injected++;
    ctx->fault_pending = true;
    return true;
  }
  return false;
}

// The row kernels' verdict-byte ring (kernels.h kRowSlots): the next slot for
// a launch on stream s. The kernel's last wave packs the bitmap from the slot
// and resets its counter, so two launches in flight on one slot would count
// each other's waves. A slot whose last user was a device-resident launch
// (enqueued on a caller's stream, not waited for before its call returned) is
// fenced: s waits for that launch's event. Host-buffer calls finish their
// launches before they return (ctx->host_sync) and record nothing.
// With a bitmap, a launch of an armed host batch also takes the tagged bitmap
// (CmtvDev::tag_arm). Each entry is stored after its slot word is zero again,
// so a slot needs no fence against a tagged launch still retiring.
static hipError_t row_slot_acquire(cmtv_ctx* ctx, CmtvDev& D, hipStream_t s, bool bitmap, RowSlot& slot,
                                   uint32_t& k) {
  hipError_t e0 = settle_polled(D);
  if (e0 != hipSuccess) return e0;
  k = D.row_seq++ % kRowSlots;
  slot = RowSlot{};
  slot.words = D.d_rowslots + (size_t)k * kRowSlotWords;
  if (bitmap && D.tag_arm) take_tags(D, slot, 32);
  if (!D.row_pending[k] || !ctx->row_fence) return hipSuccess;
  hipError_t e = hipEventQuery(D.row_ev[k]);
  if (e == hipErrorNotReady) e = hipStreamWaitEvent(s, D.row_ev[k], 0);
  if (e != hipSuccess) return e;
  D.row_pending[k] = false;
  return hipSuccess;
}

static hipError_t row_slot_release(cmtv_ctx* ctx, CmtvDev& D, hipStream_t s, uint32_t k) {
  if (ctx->host_sync || !ctx->row_fence) return hipSuccess;
  hipError_t e = hipSuccess;
  if (!D.row_ev[k]) e = hipEventCreateWithFlags(&D.row_ev[k], hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventRecord(D.row_ev[k], s);
  if (e == hipSuccess) D.row_pending[k] = true;
  return e;
}

// Enqueue verification of n signatures whose inputs are in device memory of
// device D (current on this thread).
int enqueue_verify(cmtv_ctx* ctx, CmtvDev& D, size_t n, const uint8_t* d_pk, const uint8_t* d_sig,
                   const uint8_t* d_msg, const uint32_t* d_off, uint32_t mode, uint8_t* d_valid, uint64_t* d_bitmap,
                   hipStream_t s, const SbFuse* sb, Scratch* scr) {
  Scratch& S = scr ? *scr : D.scratch;
  if (n == 0) return CMTV_OK;
  if (fault_hit(ctx) || D.inject_fault) return CMTV_EHIP;
  // fused sign-bytes only where the split kernels run, in one launch
  if (sb && (mode == kModeSr25519 || !fuse_ok(ctx, n))) return CMTV_EINVAL;
  // Small batches cannot fill the chip at one signature per lane: more lanes
  // per signature below the bands' crossovers (quad.h, oct.h, row.h,
  // sr25519_quad.h)
  const bool sr = mode == kModeSr25519;
  const uint32_t form = sr ? sr_form(ctx, n) : ed_form(ctx, n);
  const bool lane = form == kFormLane;
  const bool row = form == kFormRow || form == kFormRow4;
  const uint32_t hs_tune = ctx->hs_tune | (ctx->hs_sum_split ? kHsTuneSumSplit : 0u) |
                           (ctx->fg_late ? kHsTuneFgLate : 0u) | (ctx->hs_sum_pipe ? kHsTunePipe : 0u);
  const uint32_t kflags = form | (form == kFormQuad ? hs_tune << 16 : 0u) |
                          (ctx->force_wide ? kLaunchForceWide : 0u) | (ctx->hs_fold ? kLaunchHsFold : 0u);
  hipError_t e = hipSuccess;
  if (lane) {
    const size_t lanes = std::min<size_t>(n, ctx->lane_chunk);
    const size_t lanes_padded = (lanes + 63) / 64 * 64;
    if ((e = acquire_scratch(S, lanes_padded * kAtabWordsPerLane * sizeof(uint32_t), s)) != hipSuccess)
      return hip_fail(e);
  }
  // a row launch is one chunk (n <= kRowMaxCap)
  RowSlot slot;
  uint32_t slot_k = 0;
  if (row && (e = row_slot_acquire(ctx, D, s, d_bitmap != nullptr, slot, slot_k)) != hipSuccess) return hip_fail(e);
  // the quad kernel of an armed host batch (one launch) tags its 16-signature
  // slices (as enqueue_verify_keyed's)
  const bool qtag = ctx->quad_poll && !sr && form == kFormQuad && d_bitmap && D.tag_arm && n <= kChunk;
  if (qtag) {
    slot = RowSlot{};
    take_tags(D, slot, 16);
  }
  LaunchScope L{ctx, D, s};
  if ((e = L.begin()) != hipSuccess) return hip_fail(e);
  const size_t chunk = lane ? ctx->lane_chunk : kChunk;
  for (size_t c = 0; c < n; c += chunk) {
    const uint32_t cn = (uint32_t)std::min<size_t>(chunk, n - c);
    if (sr)
      e = launch_verify_sr25519(cn, d_pk + 32 * c, d_sig + 64 * c, d_msg, d_off + c, D.d_btab,
                                static_cast<uint32_t*>(S.buf.p), D.d_srprog, ctx->sr_nops,
                                d_valid ? d_valid + c : nullptr, d_bitmap ? d_bitmap + c / 64 : nullptr, kflags, s);
    else
      e = launch_verify(mode, cn, d_pk + 32 * c, d_sig + 64 * c, d_msg, d_off + c, D.d_btab,
                        static_cast<uint32_t*>(S.buf.p), d_valid ? d_valid + c : nullptr,
                        d_bitmap ? d_bitmap + c / 64 : nullptr, kflags, s, sb, row || qtag ? &slot : nullptr,
                        ctx->ps_wait, D.d_diag);
    if (e == hipSuccess && row) e = row_slot_release(ctx, D, s, slot_k);
    if ((e = L.launched(e)) != hipSuccess) return hip_fail(e);
  }
  return L.finish(n, lane ? &S : nullptr);
}

int enqueue_verify_keyed(cmtv_ctx* ctx, CmtvDev& D, const cmtv_keyset::PerDev& K, size_t n_keys, size_t n,
                         const uint32_t* d_idx, const uint8_t* d_sig, const uint8_t* d_msg, const uint32_t* d_off,
                         uint32_t mode, uint8_t* d_valid, uint64_t* d_bitmap, hipStream_t s, Scratch* scr,
                         const SbFuse* sb, uint32_t min_waves) {
  if (n == 0) return CMTV_OK;
  if (!min_waves) min_waves = ctx->keyed_batch_min_waves;  // a masked bulk lane holds fewer
  Scratch& S = scr ? *scr : D.scratch;
  if (sb && !keyed_fuse_ok(ctx, n)) return CMTV_EINVAL;
  if (!d_idx && !sb) return CMTV_EINVAL;  // identity keys only in the one-launch fused forms
  if (fault_hit(ctx) || D.inject_fault) return CMTV_EHIP;
  const uint32_t form = keyed_form(ctx, n);
  // lane launches: KB signatures per lane sharing one inversion while that
  // still gives two waves per SIMD (k_verify_keyed_batch; ZIP-215 by coset)
  const bool batch = form == kKeyedLane;
  // batched launches of kKeyedBatchChunk = 2^20 signatures: one full round
  // of 2,048 waves at KB = 8 (equal launches of 1.07M measured 53.9 ms for
  // configs[2]'s 15M against 37.8 ms: 2,093 waves start a second, nearly
  // empty round)
  const size_t chunk = batch ? kKeyedBatchChunk : kChunk;
  auto kb_for = [&](size_t cn) -> uint32_t { return batch ? keyed_batch_kb(cn, min_waves) : 1; };
  hipError_t e;
  const uint32_t kb0 = kb_for(std::min(chunk, n));
  if (kb0 > 1) {
    const size_t lanes = (std::min(chunk, n) + 64 * kb0 - 1) / (64 * kb0) * 64;
    if ((e = acquire_scratch(S, lanes * kb0 * kKeyedBatchScratchWordsPerSig * sizeof(uint32_t), s)) != hipSuccess)
      return hip_fail(e);
  }
  // the keyed row kernel: one chunk, one slot of the bitmap ring
  const bool krow = form == kKeyedRow;
  RowSlot slot;
  uint32_t slot_k = 0;
  if (krow && (e = row_slot_acquire(ctx, D, s, d_bitmap != nullptr, slot, slot_k)) != hipSuccess)
    return hip_fail(e);
  // the keyed quad kernel of an armed host batch (one launch) tags its
  // 16-signature slices instead of writing the bitmap: the call polls them
  // (wait_row_tags) rather than wait for the stream
  RowSlot qtags;
  const bool qtag = ctx->quad_poll && form == kKeyedQuad && d_bitmap && D.tag_arm && n <= chunk;
  if (qtag) take_tags(D, qtags, 16);
  LaunchScope L{ctx, D, s};
  if ((e = L.begin()) != hipSuccess) return hip_fail(e);
  for (size_t c = 0; c < n; c += chunk) {
    const uint32_t cn = (uint32_t)std::min<size_t>(chunk, n - c);
    // a chunk never needs more scratch than the first (kb and lanes shrink together)
    const uint32_t kb = kb0 > 1 ? kb_for(cn) : 1;
    e = launch_verify_keyed(mode, cn, (uint32_t)n_keys, d_idx ? d_idx + c : nullptr, d_sig + 64 * c, d_msg,
                            d_off + c, K.d_pk, K.d_ok, K.d_tab, d_valid ? d_valid + c : nullptr,
                            d_bitmap ? d_bitmap + c / 64 : nullptr, form, ctx->keyed_wait, D.d_diag, kb,
                            static_cast<uint32_t*>(S.buf.p), form == kKeyedLane ? K.d_wide : nullptr, D.d_btab, s,
                            krow ? &slot : qtag ? &qtags : nullptr, sb);
    if (e == hipSuccess && krow) e = row_slot_release(ctx, D, s, slot_k);
    if ((e = L.launched(e)) != hipSuccess) return hip_fail(e);
    ctx->stats.keyed_launches++;
  }
  return L.finish(n, kb0 > 1 ? &S : nullptr);
}

// ---------------------------------------------------------------- secp256k1
// ECDSA over secp256k1 (secp256k1.hip): one lane kernel for key bytes and one
// for registered keys, each also in a form whose lanes build their messages
// from commit templates; on devs[0] only; no verdict cache, no sharding.

// The fixed table of G's multiples, built on the device by the context's
// first secp256k1 batch (cmtv_open's cost and footprint stay as they were).
// Built on D's own stream and waited for, so launches on any stream may read it.
static hipError_t ensure_secp_gtab(CmtvDev& D) {
  if (D.d_secp_gtab) return hipSuccess;
  uint32_t* t = nullptr;
  hipError_t e = hipMalloc(&t, (size_t)kSecpGtabWords * sizeof(uint32_t));
  if (e != hipSuccess) return e;
  e = launch_secp_gtab_build(t, D.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(D.stream);
  if (e != hipSuccess) {
    (void)hipFree(t);
    return e;
  }
  D.d_secp_gtab = t;
  return hipSuccess;
}

// A chunk's view of a batch's templated sign-bytes: the per-signature arrays
// advanced to signature c
static SbFuse sb_at(const SbFuse& sb, size_t c) {
  SbFuse r = sb;
  if (r.tidx) r.tidx += c;
  r.flag += c;
  r.sec += c;
  r.nanos += c;
  return r;
}

// Enqueue verification of n secp256k1 signatures whose inputs are in device
// memory of device D (current on this thread): pk n x 33 bytes. With sb the
// lanes build their messages from the commit templates (d_msg / d_off unused;
// every message at most kSbFuseMaxMsg bytes).
int enqueue_verify_secp(cmtv_ctx* ctx, CmtvDev& D, size_t n, const uint8_t* d_pk, const uint8_t* d_sig,
                        const uint8_t* d_msg, const uint32_t* d_off, uint8_t* d_valid, uint64_t* d_bitmap,
                        hipStream_t s, const SbFuse* sb) {
  if (n == 0) return CMTV_OK;
  if (fault_hit(ctx) || D.inject_fault) return CMTV_EHIP;
  hipError_t e = ensure_secp_gtab(D);
  if (e != hipSuccess) return hip_fail(e);
  Scratch& S = D.scratch;
  const size_t chunk = ctx->lane_chunk;
  const size_t lanes_padded = (std::min<size_t>(n, chunk) + 63) / 64 * 64;
  if ((e = acquire_scratch(S, lanes_padded * kSecpQtabWordsPerLane * sizeof(uint32_t), s)) != hipSuccess)
    return hip_fail(e);
  LaunchScope L{ctx, D, s};
  if ((e = L.begin()) != hipSuccess) return hip_fail(e);
  for (size_t c = 0; c < n; c += chunk) {
    const uint32_t cn = (uint32_t)std::min<size_t>(chunk, n - c);
    if (sb)
      e = launch_verify_secp256k1_tmpl(cn, d_pk + 33 * c, d_sig + 64 * c, sb_at(*sb, c), D.d_secp_gtab,
                                       static_cast<uint32_t*>(S.buf.p), d_valid ? d_valid + c : nullptr,
                                       d_bitmap ? d_bitmap + c / 64 : nullptr, s);
    else
      e = launch_verify_secp256k1(cn, d_pk + 33 * c, d_sig + 64 * c, d_msg, d_off + c, D.d_secp_gtab,
                                  static_cast<uint32_t*>(S.buf.p), d_valid ? d_valid + c : nullptr,
                                  d_bitmap ? d_bitmap + c / 64 : nullptr, s);
    if ((e = L.launched(e)) != hipSuccess) return hip_fail(e);
  }
  return L.finish(n, &S);
}

// The same by registered keys (keyset.cpp cmtv_register_keys_secp256k1):
// d_idx n key indices in place of the key bytes; no scratch. batch (templated
// sign-bytes only; the cross-height typed batches): launches of
// kKeyedBatchChunk signatures, KB per lane sharing one inversion mod n
// (k_verify_secp256k1_keyed_batch) while keyed_batch_kb finds secp_batch_min_waves
// waves for it; the lanes' running products in the device's scratch.
int enqueue_verify_secp_keyed(cmtv_ctx* ctx, CmtvDev& D, const cmtv_secp_keyset* ks, size_t n, const uint32_t* d_idx,
                              const uint8_t* d_sig, const uint8_t* d_msg, const uint32_t* d_off, uint8_t* d_valid,
                              uint64_t* d_bitmap, hipStream_t s, const SbFuse* sb, bool batch) {
  if (n == 0) return CMTV_OK;
  if (fault_hit(ctx) || D.inject_fault) return CMTV_EHIP;
  hipError_t e = ensure_secp_gtab(D);
  if (e != hipSuccess) return hip_fail(e);
  const uint32_t min_waves = ctx->secp_batch_min_waves;
  auto kb_for = [&](size_t cn) -> uint32_t { return keyed_batch_kb(cn, min_waves, ctx->secp_batch_max_kb); };
  batch = batch && sb && min_waves != 0 && kb_for(std::min<size_t>(kKeyedBatchChunk, n)) > 1;
  Scratch& S = D.scratch;
  if (batch) {
    // the first chunk is the largest: kb and lanes shrink together
    const size_t cn = std::min<size_t>(kKeyedBatchChunk, n);
    const uint32_t kb = kb_for(cn);
    const size_t lanes = (cn + 64 * kb - 1) / (64 * kb) * 64;
    if ((e = acquire_scratch(S, lanes * kb * kSecpBatchScratchWordsPerSig * sizeof(uint32_t), s)) != hipSuccess)
      return hip_fail(e);
  }
  LaunchScope L{ctx, D, s};
  if ((e = L.begin()) != hipSuccess) return hip_fail(e);
  const size_t chunk = batch ? (size_t)kKeyedBatchChunk : ctx->lane_chunk;
  for (size_t c = 0; c < n; c += chunk) {
    const uint32_t cn = (uint32_t)std::min<size_t>(chunk, n - c);
    const uint32_t kb = batch ? kb_for(cn) : 1;
    if (kb > 1) {
      e = launch_verify_secp256k1_keyed_batch(kb, cn, (uint32_t)ks->n, d_idx + c, ks->d_ok, ks->d_tab, d_sig + 64 * c,
                                              sb_at(*sb, c), D.d_secp_gtab, static_cast<uint32_t*>(S.buf.p),
                                              d_valid ? d_valid + c : nullptr, d_bitmap ? d_bitmap + c / 64 : nullptr,
                                              s);
      if (e == hipSuccess) ctx->stats.secp_batch_launches++;
    } else if (sb)
      e = launch_verify_secp256k1_keyed_tmpl(cn, (uint32_t)ks->n, d_idx + c, ks->d_ok, ks->d_tab, d_sig + 64 * c,
                                             sb_at(*sb, c), D.d_secp_gtab, d_valid ? d_valid + c : nullptr,
                                             d_bitmap ? d_bitmap + c / 64 : nullptr, s);
    else
      e = launch_verify_secp256k1_keyed(cn, (uint32_t)ks->n, d_idx + c, ks->d_ok, ks->d_tab, d_sig + 64 * c, d_msg,
                                        d_off + c, D.d_secp_gtab, d_valid ? d_valid + c : nullptr,
                                        d_bitmap ? d_bitmap + c / 64 : nullptr, s);
    if ((e = L.launched(e)) != hipSuccess) return hip_fail(e);
    ctx->stats.keyed_launches++;
  }
  return L.finish(n, batch ? &S : nullptr);
}

// Commit signatures over secp256k1 keys, sign-bytes from the commits'
// templates: the templated kernels when every message fits a lane's LDS slot
// (max_len <= kSbFuseMaxMsg); otherwise k_sign_bytes writes the messages to
// d_msg at the offsets d_off (sb.tidx set then) and the message-reading
// kernels run. ks null: key bytes d_pk, else registered keys by d_idx. batch:
// the fused registered-key route may take the batched kernel.
int enqueue_verify_secp_templated(cmtv_ctx* ctx, CmtvDev& D, size_t n, const uint8_t* d_pk,
                                  const cmtv_secp_keyset* ks, const uint32_t* d_idx, const uint8_t* d_sig,
                                  const SbFuse& sb, uint32_t max_len, const uint32_t* d_off, uint8_t* d_msg,
                                  uint8_t* d_valid, uint64_t* d_bitmap, hipStream_t s, bool batch) {
  if (n == 0) return CMTV_OK;
  if (!sb.tmpls || !sb.flag || !sb.sec || !sb.nanos) return CMTV_EINVAL;
  const bool fuse = ctx->sb_fuse && max_len <= kSbFuseMaxMsg;
  if (fuse) {
    ctx->stats.fused_sign_bytes++;
  } else {
    if (!sb.tidx || !d_off || !d_msg) return CMTV_EINVAL;
    const hipError_t e = launch_sign_bytes((uint32_t)n, sb.tmpls, sb.blob, sb.tidx, sb.flag, sb.sec, sb.nanos, d_off,
                                           d_msg, s);
    if (e != hipSuccess) return hip_fail(e);
  }
  if (ks)
    return enqueue_verify_secp_keyed(ctx, D, ks, n, d_idx, d_sig, d_msg, d_off, d_valid, d_bitmap, s,
                                     fuse ? &sb : nullptr, batch);
  return enqueue_verify_secp(ctx, D, n, d_pk, d_sig, d_msg, d_off, d_valid, d_bitmap, s, fuse ? &sb : nullptr);
}

// ---------------------------------------------------------------- secp256k1 test data
// cmtv_pubkeys_secp256k1 / cmtv_sign_secp256k1 behind their argument checks
// (runtime.cpp), after the Ed25519 pair there: host buffers in and out, one
// launch per kChunk on D's stream, waited for. The comb runs over the
// verifier's fixed table.

int secp_pubkeys_host_locked(cmtv_ctx* ctx, CmtvDev& D, size_t n, const uint8_t* priv, uint8_t* out_pk,
                             uint8_t* out_addr) {
  hipError_t e = ensure_secp_gtab(D);
  if (e != hipSuccess) return hip_fail(e);
  const size_t o_addr = align_up(33 * n, 256);
  if ((e = D.d_in.ensure(32 * n)) != hipSuccess) return hip_fail(e);
  if ((e = D.d_out.ensure(o_addr + (out_addr ? 20 * n : 0))) != hipSuccess) return hip_fail(e);
  auto* dout = static_cast<uint8_t*>(D.d_out.p);
  if ((e = hipMemcpyAsync(D.d_in.p, priv, 32 * n, hipMemcpyHostToDevice, D.stream)) != hipSuccess)
    return hip_fail(e);
  LaunchScope L{ctx, D, D.stream};
  if ((e = L.begin()) != hipSuccess) return hip_fail(e);
  for (size_t c = 0; c < n; c += kChunk) {
    const uint32_t cn = (uint32_t)std::min<size_t>(kChunk, n - c);
    e = launch_secp_pubkey(cn, static_cast<uint8_t*>(D.d_in.p) + 32 * c, D.d_secp_gtab, dout + 33 * c,
                           out_addr ? dout + o_addr + 20 * c : nullptr, D.stream);
    if ((e = L.launched(e)) != hipSuccess) return hip_fail(e);
  }
  if (const int rc = L.finish_uncounted()) return rc;
  if ((e = hipMemcpyAsync(out_pk, dout, 33 * n, hipMemcpyDeviceToHost, D.stream)) != hipSuccess) return hip_fail(e);
  if (out_addr &&
      (e = hipMemcpyAsync(out_addr, dout + o_addr, 20 * n, hipMemcpyDeviceToHost, D.stream)) != hipSuccess)
    return hip_fail(e);
  if ((e = hipStreamSynchronize(D.stream)) != hipSuccess) return hip_fail(e);
  return CMTV_OK;
}

int secp_sign_host_locked(cmtv_ctx* ctx, CmtvDev& D, size_t n_keys, const uint8_t* priv, size_t n,
                          const uint32_t* key_idx, const uint8_t* msg, const uint32_t* msg_off, uint8_t* out_sig) {
  hipError_t e = ensure_secp_gtab(D);
  if (e != hipSuccess) return hip_fail(e);
  const size_t msg_bytes = msg_off[n];
  const size_t o_idx = align_up(32 * n_keys, 256), o_off = align_up(o_idx + (key_idx ? 4 * n : 0), 256);
  const size_t o_msg = align_up(o_off + 4 * (n + 1), 256), in_bytes = align_up(o_msg + msg_bytes + 16, 256);
  if ((e = D.h_in.ensure(in_bytes)) != hipSuccess) return hip_fail(e);
  if ((e = D.d_in.ensure(in_bytes)) != hipSuccess) return hip_fail(e);
  if ((e = D.d_out.ensure(64 * n)) != hipSuccess) return hip_fail(e);
  auto* hin = static_cast<uint8_t*>(D.h_in.p);
  std::memcpy(hin, priv, 32 * n_keys);
  if (key_idx) std::memcpy(hin + o_idx, key_idx, 4 * n);
  std::memcpy(hin + o_off, msg_off, 4 * (n + 1));
  if (msg_bytes) std::memcpy(hin + o_msg, msg, msg_bytes);
  auto* din = static_cast<uint8_t*>(D.d_in.p);
  if ((e = hipMemcpyAsync(din, hin, in_bytes, hipMemcpyHostToDevice, D.stream)) != hipSuccess) return hip_fail(e);
  LaunchScope L{ctx, D, D.stream};
  if ((e = L.begin()) != hipSuccess) return hip_fail(e);
  for (size_t c = 0; c < n; c += kChunk) {
    const uint32_t cn = (uint32_t)std::min<size_t>(kChunk, n - c);
    e = launch_secp_sign(cn, key_idx ? din : din + 32 * c, key_idx ? din + o_idx + 4 * c : nullptr, din + o_msg,
                         din + o_off + 4 * c, D.d_secp_gtab, static_cast<uint8_t*>(D.d_out.p) + 64 * c, D.stream);
    if ((e = L.launched(e)) != hipSuccess) return hip_fail(e);
  }
  if (const int rc = L.finish_uncounted()) return rc;
  if ((e = hipMemcpyAsync(out_sig, D.d_out.p, 64 * n, hipMemcpyDeviceToHost, D.stream)) != hipSuccess)
    return hip_fail(e);
  if ((e = hipStreamSynchronize(D.stream)) != hipSuccess) return hip_fail(e);
  return CMTV_OK;
}

// ---------------------------------------------------------------- sr25519 test data
// cmtv_pubkeys_sr25519 / cmtv_sign_sr25519 behind their argument checks
// (runtime.cpp), in the shape of the secp256k1 pair above: the same staging
// layout, the shared fixed-base table and the transcript's prefix sponge the
// context holds since it was made.

int sr_pubkeys_host_locked(cmtv_ctx* ctx, CmtvDev& D, size_t n, const uint8_t* mini, uint8_t* out_pk,
                           uint8_t* out_addr) {
  hipError_t e;
  const size_t o_addr = align_up(32 * n, 256);
  if ((e = D.d_in.ensure(32 * n)) != hipSuccess) return hip_fail(e);
  if ((e = D.d_out.ensure(o_addr + (out_addr ? 20 * n : 0))) != hipSuccess) return hip_fail(e);
  auto* dout = static_cast<uint8_t*>(D.d_out.p);
  if ((e = hipMemcpyAsync(D.d_in.p, mini, 32 * n, hipMemcpyHostToDevice, D.stream)) != hipSuccess)
    return hip_fail(e);
  LaunchScope L{ctx, D, D.stream};
  if ((e = L.begin()) != hipSuccess) return hip_fail(e);
  for (size_t c = 0; c < n; c += kChunk) {
    const uint32_t cn = (uint32_t)std::min<size_t>(kChunk, n - c);
    e = launch_pubkey_sr25519(cn, static_cast<uint8_t*>(D.d_in.p) + 32 * c, D.d_btab, dout + 32 * c,
                              out_addr ? dout + o_addr + 20 * c : nullptr, D.stream);
    if ((e = L.launched(e)) != hipSuccess) return hip_fail(e);
  }
  if (const int rc = L.finish_uncounted()) return rc;
  if ((e = hipMemcpyAsync(out_pk, dout, 32 * n, hipMemcpyDeviceToHost, D.stream)) != hipSuccess) return hip_fail(e);
  if (out_addr &&
      (e = hipMemcpyAsync(out_addr, dout + o_addr, 20 * n, hipMemcpyDeviceToHost, D.stream)) != hipSuccess)
    return hip_fail(e);
  if ((e = hipStreamSynchronize(D.stream)) != hipSuccess) return hip_fail(e);
  return CMTV_OK;
}

int sr_sign_host_locked(cmtv_ctx* ctx, CmtvDev& D, size_t n_keys, const uint8_t* mini, size_t n,
                        const uint32_t* key_idx, const uint8_t* msg, const uint32_t* msg_off, uint8_t* out_sig) {
  hipError_t e;
  const size_t msg_bytes = msg_off[n];
  const size_t o_idx = align_up(32 * n_keys, 256), o_off = align_up(o_idx + (key_idx ? 4 * n : 0), 256);
  const size_t o_msg = align_up(o_off + 4 * (n + 1), 256), in_bytes = align_up(o_msg + msg_bytes + 16, 256);
  if ((e = D.h_in.ensure(in_bytes)) != hipSuccess) return hip_fail(e);
  if ((e = D.d_in.ensure(in_bytes)) != hipSuccess) return hip_fail(e);
  if ((e = D.d_out.ensure(64 * n)) != hipSuccess) return hip_fail(e);
  auto* hin = static_cast<uint8_t*>(D.h_in.p);
  std::memcpy(hin, mini, 32 * n_keys);
  if (key_idx) std::memcpy(hin + o_idx, key_idx, 4 * n);
  std::memcpy(hin + o_off, msg_off, 4 * (n + 1));
  if (msg_bytes) std::memcpy(hin + o_msg, msg, msg_bytes);
  auto* din = static_cast<uint8_t*>(D.d_in.p);
  if ((e = hipMemcpyAsync(din, hin, in_bytes, hipMemcpyHostToDevice, D.stream)) != hipSuccess) return hip_fail(e);
  LaunchScope L{ctx, D, D.stream};
  if ((e = L.begin()) != hipSuccess) return hip_fail(e);
  for (size_t c = 0; c < n; c += kChunk) {
    const uint32_t cn = (uint32_t)std::min<size_t>(kChunk, n - c);
    e = launch_sign_sr25519(cn, key_idx ? din : din + 32 * c, key_idx ? din + o_idx + 4 * c : nullptr, din + o_msg,
                            din + o_off + 4 * c, D.d_btab, D.d_srprog, ctx->sr_nops,
                            static_cast<uint8_t*>(D.d_out.p) + 64 * c, D.stream);
    if ((e = L.launched(e)) != hipSuccess) return hip_fail(e);
  }
  if (const int rc = L.finish_uncounted()) return rc;
  if ((e = hipMemcpyAsync(out_sig, D.d_out.p, 64 * n, hipMemcpyDeviceToHost, D.stream)) != hipSuccess)
    return hip_fail(e);
  if ((e = hipStreamSynchronize(D.stream)) != hipSuccess) return hip_fail(e);
  return CMTV_OK;
}

}  // namespace cmtv
