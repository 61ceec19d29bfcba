// fake_typed_runtime.cpp -- test double of the runtime functions only the
// typed commit layer calls (runtime_internal.h verify_secp_templated_locked,
// secp_keyset_for_locked), beside the unchanged fake_runtime.cpp, for
// tests/host/typedcheck.cpp. The "device" rebuilds each message from its
// template with signbytes.h sb_write, as the templated kernels do, and
// verifies with the host-compiled secp256k1.h (secp_verify_one over the fixed
// table built by secp_gtab_row). Registered keys are looked up in the set's
// host copy and verified the same way. Test infrastructure only.
#define CMTV_HD inline
#include <cstring>
#include <memory>
#include <vector>

#include "../../cometbft_amd/csrc/secp256k1.h"
#include "../../cometbft_amd/csrc/signbytes.h"
#include "../../include/cmtverify.h"
#include "../../cometbft_amd/csrc/runtime_internal.h"

struct cmtv_secp_keyset {
  size_t n = 0;
  std::vector<uint8_t> pk;
};

namespace {

using namespace cmtv;

struct HostQTab {
  pt256 t[SECP_QTAB_ENTRIES];
  void store(int e, const pt256& p) { t[e] = p; }
  void load(int e, pt256& p) const { p = t[e]; }
};

struct HostGTab {
  std::vector<uint32_t> rows;
  HostGTab() : rows((size_t)SECP_GTAB_ENTRIES * SECP_GTAB_ROW_WORDS) {
    for (int j = 0; j < SECP_GTAB_POS; j++)
      for (int d = 1; d <= SECP_GTAB_PER_POS; d++)
        secp_gtab_row(&rows[(size_t)(j * SECP_GTAB_PER_POS + d - 1) * SECP_GTAB_ROW_WORDS], j, d);
  }
  void load(int row, pt256& p) const {
    const uint32_t* q = &rows[(size_t)row * SECP_GTAB_ROW_WORDS];
    for (int i = 0; i < 10; i++) {
      p.X.v[i] = q[i];
      p.Y.v[i] = q[10 + i];
      p.Z.v[i] = q[20 + i];
    }
  }
};

struct VecOut {
  uint8_t* p;
  void put(uint32_t pos, uint8_t b) { p[pos] = b; }
  void copy(uint32_t pos, const uint8_t* s, uint32_t len) {
    if (len) std::memcpy(p + pos, s, len);
  }
};

std::vector<std::unique_ptr<cmtv_secp_keyset>> g_sets;  // kept until exit, as the fake keeps its key sets until close
uint64_t g_calls = 0, g_keyed_calls = 0, g_sigs = 0;

}  // namespace

extern "C" void fake_typed_counts(uint64_t* out) {
  out[0] = g_calls;
  out[1] = g_keyed_calls;
  out[2] = g_sigs;
}

namespace cmtv {

int verify_secp_templated_locked(cmtv_ctx*, size_t n, const uint8_t* pk33, const cmtv_secp_keyset* ks,
                                 const uint32_t* key_idx, const uint8_t* sig, const void* tmpls, size_t n_tmpls,
                                 const uint8_t* blob, size_t, const uint32_t* tidx, const uint8_t* commit_flag,
                                 const int64_t* sec, const int32_t* nanos, uint8_t* out_valid) {
  static const HostGTab gt;
  g_calls++;
  g_keyed_calls += ks ? 1 : 0;
  g_sigs += n;
  if (ks ? !key_idx : !pk33) return CMTV_EINVAL;
  const auto* tp = static_cast<const SbTemplate*>(tmpls);
  for (size_t i = 0; i < n; i++) {
    const uint32_t ti = tidx ? tidx[i] : 0u;
    if (ti >= n_tmpls) return CMTV_EINVAL;
    const uint32_t len = sb_msg_len(tp[ti], commit_flag[i] != 0, sec[i], nanos[i]);
    // word-aligned, with the slack the hash's aligned loads may touch
    std::vector<uint32_t> buf(len / 4 + 2, 0);
    VecOut out{reinterpret_cast<uint8_t*>(buf.data())};
    if (sb_write(out, tp[ti], blob, commit_flag[i] != 0, sec[i], nanos[i]) != len) return CMTV_EINVAL;
    const uint8_t* pk;
    if (ks) {
      if (key_idx[i] >= ks->n) return CMTV_EINVAL;
      pk = ks->pk.data() + 33 * (size_t)key_idx[i];
    } else {
      pk = pk33 + 33 * i;
    }
    HostQTab qt;
    out_valid[i] = secp_verify_one(pk, sig + 64 * i, out.p, len, qt, gt) ? 1 : 0;
  }
  return CMTV_OK;
}

const cmtv_secp_keyset* secp_keyset_for_locked(cmtv_ctx* ctx, const uint8_t* pk33, size_t n_keys) {
  if (!keyset_cache_enabled(ctx) || !n_keys) return nullptr;
  for (auto& k : g_sets)
    if (k->n == n_keys && std::memcmp(k->pk.data(), pk33, 33 * n_keys) == 0) return k.get();
  g_sets.emplace_back(new cmtv_secp_keyset());
  g_sets.back()->n = n_keys;
  g_sets.back()->pk.assign(pk33, pk33 + 33 * n_keys);
  return g_sets.back().get();
}

}  // namespace cmtv
