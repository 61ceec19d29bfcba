// fake_typed_runtime.cpp -- test double of the runtime functions only the
// typed commit layer calls (runtime_internal.h verify_secp_templated_locked,
// secp_keyset_for_locked), beside fake_runtime.cpp, for
// tests/host/typedcheck.cpp and tests/host/typedcommitscheck.cpp. The "device" rebuilds each message from its
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
// [0..3): calls, calls by registered keys, signatures; [3..7): of the bulk
// calls (SecpTemplated::bulk), the same three and the templates shipped
uint64_t g_counts[7] = {};

}  // namespace

extern "C" void fake_typed_counts(uint64_t* out) { std::memcpy(out, g_counts, sizeof g_counts); }

namespace cmtv {

int verify_secp_templated_locked(cmtv_ctx*, const SecpTemplated& r, uint8_t* out_valid) {
  static const HostGTab gt;
  for (int c = 0; c <= (r.bulk ? 3 : 0); c += 3) {
    g_counts[c]++;
    g_counts[c + 1] += r.ks ? 1 : 0;
    g_counts[c + 2] += r.n;
  }
  g_counts[6] += r.bulk ? r.n_tmpls : 0;
  if (r.ks ? !r.key_idx : !r.pk33) return CMTV_EINVAL;
  const auto* tp = static_cast<const SbTemplate*>(r.tmpls);
  for (size_t i = 0; i < r.n; i++) {
    const uint32_t ti = r.tidx ? r.tidx[i] : 0u;
    if (ti >= r.n_tmpls) return CMTV_EINVAL;
    const bool for_block = r.commit_flag[i] != 0;
    const uint32_t len = sb_msg_len(tp[ti], for_block, r.sec[i], r.nanos[i]);
    // word-aligned, with the slack the hash's aligned loads may touch
    std::vector<uint32_t> buf(len / 4 + 2, 0);
    VecOut out{reinterpret_cast<uint8_t*>(buf.data())};
    if (sb_write(out, tp[ti], r.blob, for_block, r.sec[i], r.nanos[i]) != len) return CMTV_EINVAL;
    const uint8_t* pk = r.pk33 + 33 * i;
    if (r.ks) {
      if (r.key_idx[i] >= r.ks->n) return CMTV_EINVAL;
      pk = r.ks->pk.data() + 33 * (size_t)r.key_idx[i];
    }
    HostQTab qt;
    out_valid[i] = secp_verify_one(pk, r.sig + 64 * i, out.p, len, qt, gt) ? 1 : 0;
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
