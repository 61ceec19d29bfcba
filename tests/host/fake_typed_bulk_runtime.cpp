// fake_typed_bulk_runtime.cpp -- test double of the one runtime function only
// commits_typed.cpp calls (runtime_internal.h
// verify_secp_templated_bulk_locked), beside the unchanged fake_runtime.cpp
// and fake_typed_runtime.cpp, for tests/host/typedcommitscheck.cpp. The bulk
// form's verdicts are verify_secp_templated_locked's by contract, so the
// double forwards to fake_typed_runtime.cpp's and counts. Test
// infrastructure only.
#include <cstddef>
#include <cstdint>

#include "../../include/cmtverify.h"
#include "../../cometbft_amd/csrc/runtime_internal.h"

namespace {
uint64_t g_bulk_calls = 0, g_bulk_keyed = 0, g_bulk_sigs = 0, g_bulk_tmpls = 0;
}

// out[0..4): calls, calls by registered keys, signatures, templates shipped
extern "C" void fake_typed_bulk_counts(uint64_t* out) {
  out[0] = g_bulk_calls;
  out[1] = g_bulk_keyed;
  out[2] = g_bulk_sigs;
  out[3] = g_bulk_tmpls;
}

namespace cmtv {

int verify_secp_templated_bulk_locked(cmtv_ctx* ctx, size_t n, const uint8_t* pk33, const cmtv_secp_keyset* ks,
                                      const uint32_t* key_idx, const uint8_t* sig, const void* tmpls, size_t n_tmpls,
                                      const uint8_t* blob, size_t blob_len, const uint32_t* tidx,
                                      const uint8_t* commit_flag, const int64_t* sec, const int32_t* nanos,
                                      uint8_t* out_valid) {
  g_bulk_calls++;
  g_bulk_keyed += ks ? 1 : 0;
  g_bulk_sigs += n;
  g_bulk_tmpls += n_tmpls;
  return verify_secp_templated_locked(ctx, n, pk33, ks, key_idx, sig, tmpls, n_tmpls, blob, blob_len, tidx,
                                      commit_flag, sec, nanos, out_valid);
}

}  // namespace cmtv
