// keyset.cpp -- registered key sets: the per-device comb (and wide) tables of
// a validator set, the context's cache of them (cmtv_keyset_cache) with its
// eviction and pins, and their ABI entry points; and registered secp256k1
// keys (cmtv_secp_keyset: per-key combs on the first device; the typed
// commits' cache of them).
#include <new>

#include "runtime_state.h"

namespace cmtv {

// keys per comb-build launch (prefix-product scratch = 160 KiB per key)
constexpr uint32_t kCombKeyChunk = 256;

// keys per wide-comb build launch (prefix-product scratch = 20 MiB per key)
constexpr uint32_t kWideKeyChunk = 16;

// The wide combs of a key set on device D (current): 64 MiB per key.
static hipError_t build_wide(CmtvDev& D, cmtv_keyset::PerDev& K, size_t n_keys) {
  DevBuf scratch, bases;
  const size_t chunk = std::min<size_t>(n_keys, kWideKeyChunk);
  hipError_t e = hipMalloc(&K.d_wide, n_keys * kWideTableWords * sizeof(uint32_t));
  if (e == hipSuccess) e = scratch.ensure(chunk * kWideScratchWordsPerKey * sizeof(uint32_t));
  if (e == hipSuccess) e = bases.ensure(chunk * kWideBaseWordsPerKey * sizeof(uint32_t));
  for (size_t c = 0; e == hipSuccess && c < n_keys; c += kWideKeyChunk) {
    const uint32_t cn = (uint32_t)std::min<size_t>(kWideKeyChunk, n_keys - c);
    e = launch_wide_build(cn, K.d_pk + 8 * c, K.d_wide + c * kWideTableWords, static_cast<uint32_t*>(bases.p),
                          static_cast<uint32_t*>(scratch.p), D.stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(D.stream);
  scratch.release();
  bases.release();
  return e;
}

int register_keys_locked(cmtv_ctx* ctx, size_t n_keys, const uint8_t* pk, cmtv_keyset** out, uint32_t flags) {
  auto* ks = new (std::nothrow) cmtv_keyset();
  if (!ks) return CMTV_ENOMEM;
  ks->ctx = ctx;
  ks->n = n_keys;
  ks->pk.assign(pk, pk + 32 * n_keys);
  ks->dev.resize(ctx->devs.size());
  for (size_t g = 0; g < ctx->devs.size(); g++) {
    CmtvDev& D = ctx->devs[g];
    auto& K = ks->dev[g];
    if (D.failed) continue;  // retired: never given work again
    (void)hipSetDevice(D.ordinal);
    DevBuf scratch;
    hipError_t e = hipMalloc(&K.d_pk, 32 * n_keys);
    if (e == hipSuccess) e = hipMalloc(&K.d_ok, n_keys);
    if (e == hipSuccess) e = hipMalloc(&K.d_tab, n_keys * (size_t)kCombWords * sizeof(uint32_t));
    if (e == hipSuccess)
      e = scratch.ensure((size_t)std::min<size_t>(n_keys, kCombKeyChunk) * kCombScratchWordsPerKey *
                         sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpyAsync(K.d_pk, pk, 32 * n_keys, hipMemcpyHostToDevice, D.stream);
    for (size_t c = 0; e == hipSuccess && c < n_keys; c += kCombKeyChunk) {
      const uint32_t cn = (uint32_t)std::min<size_t>(kCombKeyChunk, n_keys - c);
      e = launch_comb_build(cn, K.d_pk + 8 * c, K.d_ok + c, K.d_tab + c * (size_t)kCombWords,
                            static_cast<uint32_t*>(scratch.p), true, D.stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(D.stream);
    scratch.release();
    if (e == hipSuccess && (flags & CMTV_KEYS_WIDE)) e = build_wide(D, K, n_keys);
    if (e != hipSuccess) {
      cmtv_keyset_free(ks);
      (void)hipSetDevice(ctx->devs[0].ordinal);
      return hip_fail(e);
    }
  }
  (void)hipSetDevice(ctx->devs[0].ordinal);
  *out = ks;
  return CMTV_OK;
}

// A cached key set leaving the cache: freed now, or by the pipeline call
// that still has it pinned (keyset_unpin_locked).
static void evict_keyset_locked(cmtv_ctx* ctx, cmtv_keyset* ks) {
  if (ctx->guess_ks == ks) ctx->guess_ks = nullptr;
  if (ks->pins > 0) {
    ks->evicted = true;
    ctx->zombies.push_back(ks);
    return;
  }
  cmtv_keyset_free(ks);
}

void keyset_pin_locked(const cmtv_keyset* ks) { const_cast<cmtv_keyset*>(ks)->pins++; }

void keyset_unpin_locked(cmtv_ctx* ctx, const cmtv_keyset* cks) {
  auto* ks = const_cast<cmtv_keyset*>(cks);
  if (--ks->pins > 0 || !ks->evicted) return;
  ctx->zombies.erase(std::remove(ctx->zombies.begin(), ctx->zombies.end(), ks), ctx->zombies.end());
  cmtv_keyset_free(ks);
}

const cmtv_keyset* keyset_for_locked(cmtv_ctx* ctx, const uint8_t* pk32, size_t n_keys) {
  if (!ctx->keyset_cap || n_keys == 0) return nullptr;
  const size_t bytes = 32 * n_keys;
  auto remember = [&](const cmtv_keyset* k) {
    ctx->guess_pk = pk32;
    ctx->guess_n = n_keys;
    ctx->guess_ks = k;
    return k;
  };
  for (auto& e : ctx->keysets)  // compared in place: no copy of the keys per call
    if (e.first.size() == bytes && std::memcmp(e.first.data(), pk32, bytes) == 0) return remember(e.second);
  std::string key(reinterpret_cast<const char*>(pk32), bytes);
  cmtv_keyset* ks = nullptr;
  if (register_keys_locked(ctx, n_keys, pk32, &ks, 0) != CMTV_OK) return nullptr;  // generic path instead
  if (ctx->keysets.size() >= ctx->keyset_cap) {
    evict_keyset_locked(ctx, ctx->keysets.front().second);
    ctx->keysets.erase(ctx->keysets.begin());
  }
  ctx->keysets.emplace_back(std::move(key), ks);
  return remember(ks);
}

const cmtv_keyset* keyset_guess_locked(const cmtv_ctx* ctx, const uint8_t* pk32, size_t n_keys) {
  return ctx->guess_ks && ctx->guess_pk == pk32 && ctx->guess_n == n_keys ? ctx->guess_ks : nullptr;
}

uint32_t spec_min(const cmtv_ctx* ctx) { return ctx->spec_min; }

bool keyset_holds_locked(const cmtv_keyset* ks, const uint8_t* pk32, size_t n_keys) {
  return ks->n == n_keys && std::memcmp(ks->pk.data(), pk32, 32 * n_keys) == 0;
}

bool keyset_cache_enabled(const cmtv_ctx* ctx) { return ctx->keyset_cap != 0; }

// The comb tables of n_keys secp256k1 keys on devs[0] (lock held).
static int register_secp_keys_locked(cmtv_ctx* ctx, size_t n_keys, const uint8_t* pk, cmtv_secp_keyset** out) {
  CmtvDev& D = ctx->devs[0];
  if (D.failed) return CMTV_ENODEV;
  auto* ks = new (std::nothrow) cmtv_secp_keyset();
  if (!ks) return CMTV_ENOMEM;
  ks->ctx = ctx;
  ks->n = n_keys;
  ks->pk.assign(pk, pk + 33 * n_keys);
  (void)hipSetDevice(D.ordinal);
  hipError_t e = hipMalloc(&ks->d_pk, 33 * n_keys);
  if (e == hipSuccess) e = hipMalloc(&ks->d_ok, n_keys);
  if (e == hipSuccess) e = hipMalloc(&ks->d_tab, n_keys * (size_t)kSecpGtabWords * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemcpyAsync(ks->d_pk, pk, 33 * n_keys, hipMemcpyHostToDevice, D.stream);
  if (e == hipSuccess) e = launch_secp_qcomb_build((uint32_t)n_keys, ks->d_pk, ks->d_ok, ks->d_tab, D.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(D.stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    cmtv_secp_keyset_free(ks);
    return hip_fail(e);
  }
  *out = ks;
  return CMTV_OK;
}

// cmtv_keyset_cache's secp256k1 sets (cmtv_ctx::secp_keysets): found by key
// bytes, registered on first use, the oldest freed when the list is full
// (every call that used it waited for its verdicts, and cmtv_secp_keyset_free
// waits for the stream). NULL when the cache is off, the set is too large to
// register or registration failed.
const cmtv_secp_keyset* secp_keyset_for_locked(cmtv_ctx* ctx, const uint8_t* pk33, size_t n_keys) {
  if (!ctx->keyset_cap || n_keys == 0 || n_keys > (1u << 16)) return nullptr;
  const size_t bytes = 33 * n_keys;
  for (auto* k : ctx->secp_keysets)
    if (k->pk.size() == bytes && std::memcmp(k->pk.data(), pk33, bytes) == 0) return k;
  cmtv_secp_keyset* ks = nullptr;
  if (register_secp_keys_locked(ctx, n_keys, pk33, &ks) != CMTV_OK) return nullptr;
  if (ctx->secp_keysets.size() >= ctx->keyset_cap) {
    cmtv_secp_keyset_free(ctx->secp_keysets.front());
    ctx->secp_keysets.erase(ctx->secp_keysets.begin());
  }
  ctx->secp_keysets.push_back(ks);
  return ks;
}

}  // namespace cmtv

using namespace cmtv;

extern "C" {

int cmtv_register_keys_ex(cmtv_ctx* ctx, size_t n_keys, const uint8_t* pk, uint32_t flags, cmtv_keyset** out) {
  if (!out) return CMTV_EINVAL;
  *out = nullptr;
  // 512 KiB of comb per key; 2^20 keys would already be 512 GiB (wide: 64 MiB
  // per key, 4096 keys = 256 GiB)
  if (!ctx || n_keys == 0 || n_keys > (1u << 20) || !pk || (flags & ~(uint32_t)CMTV_KEYS_WIDE)) return CMTV_EINVAL;
  if ((flags & CMTV_KEYS_WIDE) && n_keys > 4096) return CMTV_EINVAL;
  std::unique_lock<std::mutex> lk;
  if (ctx_lock(ctx, lk) != CMTV_OK) return CMTV_ENODEV;
  return cmtv::register_keys_locked(ctx, n_keys, pk, out, flags);
}

int cmtv_register_keys(cmtv_ctx* ctx, size_t n_keys, const uint8_t* pk, cmtv_keyset** out) {
  return cmtv_register_keys_ex(ctx, n_keys, pk, 0, out);
}

int cmtv_keyset_cache(cmtv_ctx* ctx, size_t max_sets) {
  if (!ctx || max_sets > 4096) return CMTV_EINVAL;
  std::unique_lock<std::mutex> lk;
  if (ctx_lock(ctx, lk) != CMTV_OK) return CMTV_ENODEV;
  for (auto& D : ctx->devs) {
    (void)hipSetDevice(D.ordinal);
    (void)hipStreamSynchronize(D.stream);
  }
  while (ctx->keysets.size() > max_sets) {
    evict_keyset_locked(ctx, ctx->keysets.front().second);
    ctx->keysets.erase(ctx->keysets.begin());
  }
  while (ctx->secp_keysets.size() > max_sets) {
    cmtv_secp_keyset_free(ctx->secp_keysets.front());
    ctx->secp_keysets.erase(ctx->secp_keysets.begin());
  }
  ctx->keyset_cap = max_sets;
  (void)hipSetDevice(ctx->devs[0].ordinal);
  return CMTV_OK;
}

void cmtv_keyset_free(cmtv_keyset* ks) {
  if (!ks) return;
  for (size_t g = 0; g < ks->dev.size(); g++) {
    (void)hipSetDevice(ks->ctx->devs[g].ordinal);
    (void)hipStreamSynchronize(ks->ctx->devs[g].stream);  // no kernel may still read the combs
    auto& K = ks->dev[g];
    if (K.d_pk) (void)hipFree(K.d_pk);
    if (K.d_ok) (void)hipFree(K.d_ok);
    if (K.d_tab) (void)hipFree(K.d_tab);
    if (K.d_wide) (void)hipFree(K.d_wide);
  }
  if (!ks->ctx->devs.empty()) (void)hipSetDevice(ks->ctx->devs[0].ordinal);
  delete ks;
}

size_t cmtv_keyset_len(const cmtv_keyset* ks) { return ks ? ks->n : 0; }

// secp256k1: the tables live on devs[0] only, where every secp256k1 launch runs.
int cmtv_register_keys_secp256k1(cmtv_ctx* ctx, size_t n_keys, const uint8_t* pk, cmtv_secp_keyset** out) {
  if (!out) return CMTV_EINVAL;
  *out = nullptr;
  // 528 KiB of comb per key: 65,536 keys are 33 GiB
  if (!ctx || n_keys == 0 || n_keys > (1u << 16) || !pk) return CMTV_EINVAL;
  std::unique_lock<std::mutex> lk;
  if (ctx_lock(ctx, lk) != CMTV_OK) return CMTV_ENODEV;
  return register_secp_keys_locked(ctx, n_keys, pk, out);
}

void cmtv_secp_keyset_free(cmtv_secp_keyset* ks) {
  if (!ks) return;
  if (!ks->ctx->devs.empty()) {
    (void)hipSetDevice(ks->ctx->devs[0].ordinal);
    (void)hipStreamSynchronize(ks->ctx->devs[0].stream);  // no kernel may still read the tables
  }
  if (ks->d_pk) (void)hipFree(ks->d_pk);
  if (ks->d_ok) (void)hipFree(ks->d_ok);
  if (ks->d_tab) (void)hipFree(ks->d_tab);
  delete ks;
}

size_t cmtv_secp_keyset_len(const cmtv_secp_keyset* ks) { return ks ? ks->n : 0; }

}  // extern "C"
