// commits_typed.cpp -- VerifyCommit* of many heights in one call over
// validator sets of Ed25519, secp256k1 and sr25519 keys, and sets that mix
// them (cmtv_verify_commits_typed): the typed form of cmtv_verify_commits,
// for blocksync and light-client replay of a chain whose validators do not
// all hold Ed25519 keys (blockchain/v0/reactor.go:349-400,
// light/client.go:613-689).
//
// Every commit is planned as commit_typed.cpp plans one (job_preamble /
// job_plan with CommitJob::key_types) and gets one sign-bytes template; the
// planned signatures of ALL commits are split by key type
// (commit_typed_parts.h), each share is verified in as few device batches as
// the limits allow, the verdicts are scattered back and the reference loop
// is replayed per commit (job_replay). A commit that ends in its preamble
// costs no device work. Outcomes are, commit by commit, those of
// cmtv_verify_commit_typed.
//
//   Ed25519    verify_templated_locked over the template array, split into
//              runs whose sign-bytes span stays below 2 GiB (as commit.cpp
//              batch_verify)
//   secp256k1  verify_secp_templated_bulk_locked: launches of many heights
//              are large enough for the kernel that shares one inversion mod
//              n among the 4 or 8 signatures of a lane
//              (k_verify_secp256k1_keyed_batch); by registered keys when
//              cmtv_keyset_cache is on and the set is all secp256k1 with
//              keys packed at 33 bytes, else by key bytes
//   sr25519    sign-bytes written here on the host, the runtime's host batch
//
// Registered keys: consecutive commits whose sets hold the same keys (the
// pointer compared first, then the bytes, once per new set) form one group
// and one batch. Groups are verified one after another -- each blocking
// batch finishes before the next set is looked up -- so a call with more
// distinct sets than the cache holds never reads an evicted table.
//
// A call with no key of another type is cmtv_verify_commits. Typed calls
// never enter the cross-height pipeline; the runtime function only this file
// names (verify_secp_templated_bulk_locked) lives here only, so commit.cpp,
// commit_typed.cpp and pipeline.cpp link without it.
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <optional>
#include <utility>
#include <vector>

#include "../../include/cmtverify.h"
#include "commit_internal.h"
#include "commit_typed_parts.h"
#include "runtime_internal.h"
#include "signbytes.h"

namespace {

using namespace cmtv;

// every key of the set is secp256k1 and the keys are packed at 33 bytes: the
// set can be registered, a key's index is its validator's
bool registrable(const cmtv_valset* vs, const uint8_t* types) {
  if (!types || vs->n_vals == 0) return false;
  for (uint32_t i = 0; i < vs->n_vals; i++)
    if (types[i] != CMTV_KEY_SECP256K1 || vs->pk_off[i] != 33 * i) return false;
  return vs->pk_off[vs->n_vals] == 33 * vs->n_vals;
}

// [a, b) runs of a share whose sign-bytes span stays `slack` below the
// device's 32-bit offsets (commit.cpp batch_verify's split): f(a, b, off32)
// per run, off32 the b - a + 1 message offsets from the run's start
template <class F>
int for_runs(const Part& P, const SbTemplate* tmpls, uint64_t slack, F f) {
  const size_t m = P.size();
  const uint64_t cap = max_batch_msg_bytes() - slack;
  std::vector<uint32_t> off32;
  for (size_t a = 0; a < m;) {
    off32.assign(1, 0);
    uint64_t span = 0;
    size_t b = a;
    while (b < m) {
      const uint32_t len = sb_msg_len(tmpls[P.tidx[b]], P.flag[b] != 0, P.sec[b], P.nanos[b]);
      if (b > a && span + len >= cap) break;
      span += len;
      off32.push_back((uint32_t)span);
      b++;
    }
    if (span >= cap) return CMTV_EINVAL;  // one message of 2 GiB
    const int rc = f(a, b, off32);
    if (rc != CMTV_OK) return rc;
    a = b;
  }
  return CMTV_OK;
}

int verify_commits_typed(cmtv_ctx* ctx, uint32_t kind, uint32_t mode, const char* chain_id, size_t chain_id_len,
                         size_t n, const cmtv_valset* vals, const uint8_t* const* key_types,
                         const cmtv_block_id* block_ids, const int64_t* heights, const cmtv_commit* commits,
                         uint64_t trust_num, uint64_t trust_den, cmtv_commit_result* results, int* rcs,
                         char* msg_bufs, size_t msg_cap) {
  if (!ctx || mode > CMTV_MODE_ZIP215 || n > (1u << 24)) return CMTV_EINVAL;
  if (n == 0) return CMTV_OK;
  const bool trusting = kind == CMTV_VERIFY_COMMIT_LIGHT_TRUSTING;
  if (!vals || !commits || !results || !rcs || !heights || (!trusting && !block_ids)) return CMTV_EINVAL;
  bool typed = false;
  uint64_t n_sigs = 0;
  for (size_t c = 0; c < n; c++) {
    const int rc =
        job_check_args(kind, chain_id, chain_id_len, &vals[c], block_ids ? &block_ids[c] : nullptr, &commits[c],
                       &results[c]);
    if (rc != CMTV_OK) return rc;
    n_sigs += commits[c].n_sigs;
    const uint8_t* kt = key_types ? key_types[c] : nullptr;
    if (!kt) continue;
    for (uint32_t i = 0; i < vals[c].n_vals; i++) {
      if (kt[i] > CMTV_KEY_SR25519) return CMTV_EINVAL;
      if (kt[i] == CMTV_KEY_SECP256K1 && vals[c].pk_off[i + 1] - vals[c].pk_off[i] == 65) return CMTV_EINVAL;
      typed = typed || kt[i] != CMTV_KEY_ED25519;
    }
  }
  if (!typed)
    return cmtv_verify_commits(ctx, kind, mode, chain_id, chain_id_len, n, vals, block_ids, heights, commits,
                               trust_num, trust_den, results, rcs, msg_bufs, msg_cap);
  if (n_sigs >= (1ull << 32)) return CMTV_EINVAL;  // verdict positions are 32-bit

  const CommitsArgs args{kind, mode, chain_id, chain_id_len, n, vals, block_ids, heights, commits, trust_num,
                         trust_den, results, msg_bufs, msg_cap};
  std::vector<CommitJob> jobs;
  jobs.reserve(n);
  for (size_t c = 0; c < n; c++) {
    jobs.push_back(args.job(c));
    jobs.back().key_types = key_types[c];
  }
  // LightTrusting: one address index per distinct (address array, size)
  std::map<std::pair<const uint8_t*, uint32_t>, AddrIndex> addr;
  if (trusting)
    for (auto& J : jobs) {
      const auto key = std::make_pair(J.vals->addrs, J.vals->n_vals);
      auto it = addr.find(key);
      if (it == addr.end()) {
        it = addr.emplace(key, AddrIndex()).first;
        it->second.build(J.vals->addrs, J.vals->n_vals);
      }
      J.addr = &it->second;
    }
  thread_local Seen seen;
  if (n_sigs <= 4096) note_latency(ctx);  // a small call waits on its verdicts
  std::unique_lock<std::mutex> lk;
  int rc = ctx_lock(ctx, lk);
  if (rc != CMTV_OK) return rc;
  std::optional<LatencyStreams> lat_streams;
  if (n_sigs <= 4096) lat_streams.emplace(ctx);

  uint64_t tp = phase_now(ctx);
  // one template per planned commit, their bytes back to back in the blob
  std::vector<SbTemplate> tmpls(n);
  std::vector<uint8_t> blob;
  std::vector<uint8_t> valid, pv;
  auto scatter = [&](const Part& P, size_t a, size_t b) {
    for (size_t k = a; k < b; k++) valid[P.at[k]] = pv[k - a];
  };
  // The secp256k1 share of the current group, verified when the group ends.
  // group_vs set: consecutive commits of one registrable set (by registered
  // keys when the cache gives the set); null: key bytes. A group ships only
  // its own commits' templates: g_tmpls, over the blob from g_blob0 on.
  Part ed, secp, sr;
  const cmtv_valset* group_vs = nullptr;
  std::vector<SbTemplate> g_tmpls;
  size_t g_blob0 = 0;
  auto flush_secp = [&]() -> int {
    int r = CMTV_OK;
    if (secp.size()) {
      const cmtv_secp_keyset* ks = nullptr;
      if (group_vs) {
        const uint64_t tk = phase_now(ctx);
        ks = secp_keyset_for_locked(ctx, group_vs->pubkeys, group_vs->n_vals);
        phase_add(ctx, kPhKeyset, tk);
      }
      // 32: the runtime wants 16 bytes after the last message below 2 GiB
      r = for_runs(secp, g_tmpls.data(), 32, [&](size_t a, size_t b, const std::vector<uint32_t>&) {
        pv.assign(b - a, 0);
        const int q = verify_secp_templated_bulk_locked(
            ctx, b - a, ks ? nullptr : secp.pk.data() + 33 * a, ks, ks ? secp.kidx.data() + a : nullptr,
            secp.sg.data() + 64 * a, g_tmpls.data(), g_tmpls.size(), blob.data() + g_blob0, blob.size() - g_blob0,
            secp.tidx.data() + a, secp.flag.data() + a, secp.sec.data() + a, secp.nanos.data() + a, pv.data());
        if (q == CMTV_OK) scatter(secp, a, b);
        return q;
      });
    }
    secp.clear();
    g_tmpls.clear();
    g_blob0 = blob.size();
    return r;
  };

  const bool cache_on = keyset_cache_enabled(ctx);
  for (size_t c = 0; c < n; c++) {
    CommitJob& J = jobs[c];
    job_preamble(J);
    J.first = valid.size();
    if (J.early != 1) continue;
    const uint32_t nsig = commits[c].n_sigs;
    J.plan_idx.resize(nsig);
    J.plan_val.resize(nsig);
    const size_t m = job_plan(J, J.plan_idx.data(), J.plan_val.data(), seen);
    J.plan_idx.resize(m);
    J.plan_val.resize(m);
    // the commit's group: the registrable set of the commit before (the same
    // key array, else equal key bytes: same_keys), a new one, or none
    const cmtv_valset* vs = cache_on && registrable(&vals[c], key_types[c]) ? &vals[c] : nullptr;
    const bool same = vs ? group_vs && same_keys(group_vs, vs) : !group_vs;
    // (an all-Ed25519 commit adds nothing to the group and ends none)
    if (!same && key_types[c]) {
      phase_add(ctx, kPhPrepare, tp);
      if ((rc = flush_secp()) != CMTV_OK) return rc;
      tp = phase_now(ctx);
      group_vs = vs;
    }
    const size_t at = blob.size();
    blob.resize(at + put_commit_template(nullptr, 0, chain_id, chain_id_len, &commits[c], nullptr));
    if (blob.size() >= (1ull << 32)) return CMTV_EINVAL;  // template offsets are 32-bit
    put_commit_template(blob.data(), at, chain_id, chain_id_len, &commits[c], &tmpls[c]);
    SbTemplate g = tmpls[c];  // the same template over the group's slice of the blob
    g.pre_commit_off -= (uint32_t)g_blob0;
    g.pre_nil_off -= (uint32_t)g_blob0;
    g.post_off -= (uint32_t)g_blob0;
    valid.resize(valid.size() + m, 0);
    const size_t e0 = ed.size(), r0 = sr.size();
    partition_plan(J, m, J.first, (uint32_t)g_tmpls.size(), ed, secp, sr);
    g_tmpls.push_back(g);
    for (size_t k = e0; k < ed.size(); k++) ed.tidx[k] = (uint32_t)c;
    for (size_t k = r0; k < sr.size(); k++) sr.tidx[k] = (uint32_t)c;
  }
  phase_add(ctx, kPhPrepare, tp);
  if ((rc = flush_secp()) != CMTV_OK) return rc;

  if (ed.size()) {
    rc = for_runs(ed, tmpls.data(), 0, [&](size_t a, size_t b, const std::vector<uint32_t>& off32) {
      pv.assign(b - a, 0);
      const int q = verify_templated_locked(ctx, b - a, ed.pk.data() + 32 * a, ed.sg.data() + 64 * a, off32.data(),
                                            tmpls.data(), n, blob.data(), blob.size(), ed.tidx.data() + a,
                                            ed.flag.data() + a, ed.sec.data() + a, ed.nanos.data() + a, mode,
                                            pv.data());
      if (q == CMTV_OK) scatter(ed, a, b);
      return q;
    });
    if (rc != CMTV_OK) return rc;
  }
  if (sr.size()) {
    rc = for_runs(sr, tmpls.data(), 0, [&](size_t a, size_t b, const std::vector<uint32_t>& off32) {
      pv.assign(b - a, 0);
      std::vector<uint8_t> msgs((size_t)off32.back() + 1);
      for (size_t k = a; k < b; k++) {
        HostBytes out{msgs.data() + off32[k - a]};
        sb_write(out, tmpls[sr.tidx[k]], blob.data(), sr.flag[k] != 0, sr.sec[k], sr.nanos[k]);
      }
      const int q = verify_host_locked(ctx, b - a, sr.pk.data() + 32 * a, sr.sg.data() + 64 * a, msgs.data(),
                                       off32.data(), kModeSr25519, pv.data(), nullptr);
      if (q == CMTV_OK) scatter(sr, a, b);
      return q;
    });
    if (rc != CMTV_OK) return rc;
  }

  const uint64_t t1 = phase_now(ctx);
  for (size_t c = 0; c < n; c++) {
    CommitJob& J = jobs[c];
    const uint8_t* v = valid.data() + J.first;
    rcs[c] = job_replay(J, J.plan_idx.data(), J.plan_idx.size(), [v](size_t j) { return v[j] != 0; }, seen);
  }
  phase_add(ctx, kPhReplay, t1);
  return CMTV_OK;
}

}  // namespace

extern "C" int cmtv_verify_commits_typed(cmtv_ctx* ctx, uint32_t kind, uint32_t mode, const char* chain_id,
                                         size_t chain_id_len, size_t n, const cmtv_valset* vals,
                                         const uint8_t* const* key_types, const cmtv_block_id* block_ids,
                                         const int64_t* heights, const cmtv_commit* commits, uint64_t trust_num,
                                         uint64_t trust_den, cmtv_commit_result* results, int* rcs, char* msg_bufs,
                                         size_t msg_cap) {
  // no C++ exception crosses the C ABI
  try {
    return verify_commits_typed(ctx, kind, mode, chain_id, chain_id_len, n, vals, key_types, block_ids, heights,
                                commits, trust_num, trust_den, results, rcs, msg_bufs, msg_cap);
  } catch (const std::bad_alloc&) {
    return CMTV_ENOMEM;
  } catch (...) {
    return CMTV_EINVAL;
  }
}
