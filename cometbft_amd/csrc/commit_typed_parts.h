// commit_typed_parts.h -- what the typed commit entry points share
// (commit_typed.cpp: one commit; commits_typed.cpp: many heights): a key
// type's share of the planned signatures and the loop that splits a commit's
// plan into the three shares. Header-only and free of runtime calls, so each
// file links with exactly the runtime functions it names itself.
#pragma once
#include <cstring>
#include <vector>

#include "../../include/cmtverify.h"
#include "commit_internal.h"
#include "signbytes.h"

namespace cmtv {

// Byte writer (signbytes.h sb_write) into host memory
struct HostBytes {
  uint8_t* p;
  void put(uint32_t pos, uint8_t b) { p[pos] = b; }
  void copy(uint32_t pos, const uint8_t* src, uint32_t len) {
    if (len) std::memcpy(p + pos, src, len);
  }
};

// One key type's share of the plan: verdict positions and the per-signature
// arrays its batch reads
struct Part {
  std::vector<uint32_t> at;  // verdict position (plan item) of each entry
  std::vector<uint8_t> pk, sg, flag;
  std::vector<int64_t> sec;
  std::vector<int32_t> nanos;
  std::vector<uint32_t> kidx;
  std::vector<uint32_t> tidx;  // the entry's commit template (all 0 for one commit)
  size_t size() const { return at.size(); }
  void reserve(size_t n, size_t key_width) {
    at.reserve(n);
    pk.reserve(key_width * n);
    sg.reserve(64 * n);
    flag.reserve(n);
    sec.reserve(n);
    nanos.reserve(n);
    kidx.reserve(n);
    tidx.reserve(n);
  }
  void clear() {
    at.clear();
    pk.clear();
    sg.clear();
    flag.clear();
    sec.clear();
    nanos.clear();
    kidx.clear();
    tidx.clear();
  }
  void add(uint32_t j, const uint8_t* key, size_t key_len, size_t key_width, const uint8_t* sig, bool for_block,
           int64_t s, int32_t ns, uint32_t vi, uint32_t ti = 0) {
    at.push_back(j);
    // the key in a zeroed array of the type's width (sr25519: truncated or
    // zero-padded, crypto/sr25519/pubkey.go:36-45; the others arrive whole)
    const size_t o = pk.size();
    pk.resize(o + key_width, 0);
    std::memcpy(&pk[o], key, key_len < key_width ? key_len : key_width);
    sg.insert(sg.end(), sig, sig + 64);
    flag.push_back(for_block ? 1 : 0);
    sec.push_back(s);
    nanos.push_back(ns);
    kidx.push_back(vi);
    tidx.push_back(ti);
  }
};

// The planned signatures of J (J.plan_idx / J.plan_val, m of them), split by
// their validators' key types; plan item j gets verdict position base + j
// and template ti. A signature that is not 64 bytes is wrong for every type
// before its key is looked at, and a secp256k1 key that is not 33 bytes fails
// ParsePubKey: neither goes to a device, their verdict stays 0.
inline void partition_plan(const CommitJob& J, size_t m, size_t base, uint32_t ti, Part& ed, Part& secp, Part& sr) {
  const cmtv_valset* vals = J.vals;
  const cmtv_commit* commit = J.commit;
  for (size_t j = 0; j < m; j++) {
    const uint32_t idx = J.plan_idx[j], vi = J.plan_val[j];
    const uint32_t s0 = commit->sig_off[idx], s1 = commit->sig_off[idx + 1];
    if (s1 - s0 != 64) continue;
    const uint8_t* key = vals->pubkeys + vals->pk_off[vi];
    const size_t kl = vals->pk_off[vi + 1] - vals->pk_off[vi];
    const bool for_block = commit->flags[idx] == kFlagCommit;
    const uint8_t t = J.key_type(vi);
    if (t == CMTV_KEY_SECP256K1 && kl != 33) continue;
    Part& P = t == CMTV_KEY_ED25519 ? ed : t == CMTV_KEY_SECP256K1 ? secp : sr;
    P.add((uint32_t)(base + j), key, kl, t == CMTV_KEY_SECP256K1 ? 33 : 32, commit->sigs + s0, for_block,
          commit->ts_seconds[idx], commit->ts_nanos[idx], vi, ti);
  }
}

}  // namespace cmtv
