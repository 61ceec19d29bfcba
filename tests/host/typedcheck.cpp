// typedcheck.cpp -- the typed commit layer (cometbft_amd/csrc/commit_typed.cpp,
// with commit.cpp) on the CPU, linked against fake_runtime.cpp and
// fake_typed_runtime.cpp, under AddressSanitizer + UBSan: the partition
// of a plan by key type, the three batches' arrays and the scatter of their
// verdicts back into plan order. A single commit never takes the routes of
// the many-heights call: no secp256k1 batch is a bulk one, and the Ed25519
// share of a mixed set arrives as one batch without message offsets.
//
//   typedcheck FILE
// FILE holds cases written by tests/test_typed_commit_host.py (little-endian):
//   u32 n_cases, then per case
//     u32 kind, u32 keyset_cap, u64 trust_num, u64 trust_den, i64 height, u32 chain_len, chain
//     u32 n_vals, per validator: u8 type, u32 key_len, key, i64 power, u8 addr[20]
//     commit: i64 height, i32 round, u8 hash[32], u32 psh_total, u8 psh_hash[32],
//             u32 n_sigs, per signature: u8 flag, u8 addr[20], i64 sec, i32 nanos, u32 sig_len, sig
//     expected: i32 rc, i32 code, i32 sig_index (-2: not compared), u32 msg_len, msg,
//               u32 n_verified, i32 keyed (1: the secp256k1 batch must be by registered keys, 0: must not, -1: none)
// Prints one line per case and "typedcheck ok (N cases)"; exit status 1 on a mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cmtverify.h"
#include "case_reader.h"

extern "C" {
cmtv_ctx* fake_open(size_t n_devs, unsigned threads, size_t pipe_min, size_t chunk, int slots, bool pipe_on,
                    size_t keyset_cap, long fail_dev);
void fake_close(cmtv_ctx* c);
void fake_counts(cmtv_ctx* c, uint64_t* out);
void fake_typed_counts(uint64_t* out);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  Reader r;
  if (!r.load(argv[1])) return 2;
  const uint32_t n_cases = r.get<uint32_t>();
  int bad = 0;
  for (uint32_t c = 0; c < n_cases; c++) {
    const uint32_t kind = r.get<uint32_t>(), cap = r.get<uint32_t>();
    const uint64_t num = r.get<uint64_t>(), den = r.get<uint64_t>();
    const int64_t height = r.get<int64_t>();
    const auto chain = r.bytes(r.get<uint32_t>());
    const uint32_t nv = r.get<uint32_t>();
    // exact-size arrays, so that AddressSanitizer sees any read past them
    std::vector<uint8_t> types(nv), keys, addrs;
    bool any_ed = false, any_other = false;
    std::vector<uint32_t> pk_off(nv + 1, 0);
    std::vector<int64_t> power(nv), prio(nv, 0);
    for (uint32_t i = 0; i < nv; i++) {
      types[i] = r.get<uint8_t>();
      (types[i] == CMTV_KEY_ED25519 ? any_ed : any_other) = true;
      const auto k = r.bytes(r.get<uint32_t>());
      keys.insert(keys.end(), k.begin(), k.end());
      pk_off[i + 1] = (uint32_t)keys.size();
      power[i] = r.get<int64_t>();
      const auto a = r.bytes(20);
      addrs.insert(addrs.end(), a.begin(), a.end());
    }
    cmtv_commit cm{};
    cm.height = r.get<int64_t>();
    cm.round = r.get<int32_t>();
    const auto hash = r.bytes(32);
    const uint32_t total = r.get<uint32_t>();
    const auto psh = r.bytes(32);
    cm.block_id = cmtv_block_id{hash.data(), 32, total, psh.data(), 32};
    const uint32_t ns = r.get<uint32_t>();
    std::vector<uint8_t> flags(ns), vaddrs, sigs;
    std::vector<int64_t> sec(ns);
    std::vector<int32_t> nanos(ns);
    std::vector<uint32_t> sig_off(ns + 1, 0);
    for (uint32_t i = 0; i < ns; i++) {
      flags[i] = r.get<uint8_t>();
      const auto a = r.bytes(20);
      vaddrs.insert(vaddrs.end(), a.begin(), a.end());
      sec[i] = r.get<int64_t>();
      nanos[i] = r.get<int32_t>();
      const auto s = r.bytes(r.get<uint32_t>());
      sigs.insert(sigs.end(), s.begin(), s.end());
      sig_off[i + 1] = (uint32_t)sigs.size();
    }
    static const uint8_t none = 0;
    cm.n_sigs = ns;
    cm.flags = flags.data();
    cm.ts_seconds = sec.data();
    cm.ts_nanos = nanos.data();
    cm.sigs = sigs.empty() ? &none : sigs.data();
    cm.sig_off = sig_off.data();
    cm.val_addrs = vaddrs.data();
    cmtv_valset vs{nv, keys.data(), pk_off.data(), power.data(), addrs.data(), prio.data()};
    const int32_t want_rc = r.get<int32_t>(), want_code = r.get<int32_t>(), want_idx = r.get<int32_t>();
    const auto wm = r.bytes(r.get<uint32_t>());
    const std::string want_msg(wm.begin(), wm.end());
    const uint32_t want_nv = r.get<uint32_t>();
    const int32_t want_keyed = r.get<int32_t>();

    cmtv_ctx* ctx = fake_open(1, 1, (size_t)1 << 40, 1u << 20, 3, false, cap, -1);
    uint64_t c0[7], c1[7], cnt[9];
    fake_typed_counts(c0);
    cmtv_commit_result res{};
    char msg[2048];
    const int rc = cmtv_verify_commit_typed(ctx, kind, CMTV_MODE_GO_STDLIB, reinterpret_cast<const char*>(chain.data()),
                                            chain.size(), &vs, types.data(), &cm.block_id, height, &cm, num, den, &res,
                                            msg, sizeof msg);
    fake_typed_counts(c1);
    fake_counts(ctx, cnt);
    fake_close(ctx);
    const int keyed = c1[0] == c0[0] ? -1 : (c1[1] > c0[1] ? 1 : 0);
    // no bulk call; a mixed set's Ed25519 share is the context's one offset-free templated batch
    const bool routes = c1[3] == c0[3] && cnt[8] == (any_ed && any_other ? 1u : 0u);
    const bool ok = routes && rc == want_rc && res.code == want_code && (want_idx == -2 || res.sig_index == want_idx) &&
                    want_msg == msg && res.n_verified == want_nv && keyed == want_keyed;
    std::printf("case %u: rc %d code %d index %d verified %u keyed %d bulk %llu offset-free %llu %s\n", c, rc, res.code,
                res.sig_index, res.n_verified, keyed, (unsigned long long)(c1[3] - c0[3]), (unsigned long long)cnt[8],
                ok ? "ok" : "MISMATCH");
    if (!ok) {
      std::printf("  want rc %d code %d index %d verified %u keyed %d\n  got  \"%s\"\n  want \"%s\"\n", want_rc, want_code,
                  want_idx, want_nv, want_keyed, msg, want_msg.c_str());
      bad++;
    }
  }
  if (bad) return 1;
  std::printf("typedcheck ok (%u cases)\n", n_cases);
  return 0;
}
