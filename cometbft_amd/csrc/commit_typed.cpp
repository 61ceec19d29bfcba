// commit_typed.cpp -- VerifyCommit* over validator sets of Ed25519, secp256k1
// and sr25519 keys, and sets that mix them (cmtv_verify_commit_typed).
//
// The reference loop calls val.PubKey.VerifySignature(voteSignBytes, sig)
// (types/validator_set.go:695, 751, 812), which dispatches on the key's type.
// Here the commit is planned as commit.cpp plans it (commit_internal.h
// job_preamble / job_plan, with CommitJob::key_types set), the planned
// signatures are split by key type, each part is verified by its own batch,
// the verdicts are scattered back into plan order and the reference loop is
// replayed over them (job_replay), so error, early exit, tally and string are
// the reference's.
//
//   Ed25519    the templated batch of cmtv_verify_commit (key bytes)
//   secp256k1  verify_secp_templated_locked: the kernels build every
//              CanonicalVote from the commit's template on the device; by
//              registered keys when cmtv_keyset_cache is on and the whole set
//              is secp256k1 with keys packed at 33 bytes
//   sr25519    sign-bytes written here on the host from the same template
//              and the runtime's sr25519 host batch: there is no templated
//              sr25519 kernel yet
//
// A set with no key of another type is forwarded to cmtv_verify_commit. Typed
// calls never enter the cross-height pipeline or the speculative path; many
// heights in one call are commits_typed.cpp (cmtv_verify_commits_typed), with
// the partition shared in commit_typed_parts.h. The calls into the runtime that
// commit.cpp does not make live here only: commit.cpp and pipeline.cpp link
// without them.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/cmtverify.h"
#include "commit_internal.h"
#include "commit_typed_parts.h"
#include "runtime_internal.h"
#include "signbytes.h"

namespace {

using namespace cmtv;

int verify_typed(cmtv_ctx* ctx, uint32_t kind, uint32_t mode, const char* chain_id, size_t chain_id_len,
                 const cmtv_valset* vals, const uint8_t* key_types, const cmtv_block_id* block_id, int64_t height,
                 const cmtv_commit* commit, uint64_t trust_num, uint64_t trust_den, cmtv_commit_result* res,
                 char* msg_buf, size_t msg_cap) {
  if (!ctx || mode > CMTV_MODE_ZIP215) return CMTV_EINVAL;
  int rc = job_check_args(kind, chain_id, chain_id_len, vals, block_id, commit, res);
  if (rc != CMTV_OK) return rc;
  bool typed = false, all_secp = vals->n_vals != 0;
  if (key_types)
    for (uint32_t i = 0; i < vals->n_vals; i++) {
      const uint8_t t = key_types[i];
      if (t > CMTV_KEY_SR25519) return CMTV_EINVAL;
      if (t == CMTV_KEY_SECP256K1 && vals->pk_off[i + 1] - vals->pk_off[i] == 65) return CMTV_EINVAL;
      typed = typed || t != CMTV_KEY_ED25519;
      all_secp = all_secp && t == CMTV_KEY_SECP256K1 && vals->pk_off[i] == 33 * i;
    }
  if (!typed)
    return cmtv_verify_commit(ctx, kind, mode, chain_id, chain_id_len, vals, block_id, height, commit, trust_num,
                              trust_den, res, msg_buf, msg_cap);
  all_secp = all_secp && vals->pk_off[vals->n_vals] == 33 * vals->n_vals;

  CommitJob J{kind, chain_id, chain_id_len, vals, block_id, height, commit, trust_num, trust_den, res, msg_buf,
              msg_cap};
  J.key_types = key_types;
  AddrIndex addr;
  const bool trusting = kind == CMTV_VERIFY_COMMIT_LIGHT_TRUSTING;
  if (trusting) {
    addr.build(vals->addrs, vals->n_vals);
    J.addr = &addr;
  }
  thread_local Seen seen;
  note_latency(ctx);
  std::unique_lock<std::mutex> lk;
  rc = ctx_lock(ctx, lk);
  if (rc != CMTV_OK) return rc;
  LatencyStreams lat_streams(ctx);

  const uint64_t t0 = phase_now(ctx);
  job_preamble(J);
  if (J.early != 1) return J.early;
  const uint32_t nsig = commit->n_sigs;
  J.plan_idx.resize(nsig);
  J.plan_val.resize(nsig);
  const size_t m = job_plan(J, J.plan_idx.data(), J.plan_val.data(), seen);
  J.plan_idx.resize(m);
  J.plan_val.resize(m);

  // the commit's template, shared by the three parts
  SbTemplate tmpl{};
  std::vector<uint8_t> blob(put_commit_template(nullptr, 0, chain_id, chain_id_len, commit, nullptr));
  put_commit_template(blob.data(), 0, chain_id, chain_id_len, commit, &tmpl);
  const uint32_t bound = msg_len_bound(TplLens{tmpl.pre_commit_len, tmpl.pre_nil_len, tmpl.post_len});

  std::vector<uint8_t> valid(m, 0), pv;
  // a registered set's key index is the validator index
  auto secp_keyset = [&]() -> const cmtv_secp_keyset* {
    if (!all_secp || !keyset_cache_enabled(ctx)) return nullptr;
    const uint64_t tk = phase_now(ctx);
    const cmtv_secp_keyset* ks = secp_keyset_for_locked(ctx, vals->pubkeys, vals->n_vals);
    phase_add(ctx, kPhKeyset, tk);
    return ks;
  };

  // The common all-secp256k1 VerifyCommit: the plan is every signature in
  // index order, keys packed at 33 bytes and signatures at 64. The caller's
  // key, signature and timestamp arrays are then the batch itself (as
  // commit.cpp job_prepare_identity borrows them): only the flags are written.
  bool identity = all_secp && !trusting && m != 0 && m == nsig && m == vals->n_vals && J.plan_idx[m - 1] == m - 1;
  for (size_t i = 0; identity && i <= m; i++) identity = commit->sig_off[i] == 64 * i;
  if (identity) {
    std::vector<uint8_t> flag(m);
    for (size_t i = 0; i < m; i++) flag[i] = commit->flags[i] == kFlagCommit;
    phase_add(ctx, kPhPrepare, t0);
    const cmtv_secp_keyset* ks = secp_keyset();
    std::vector<uint32_t> kidx;
    if (ks) {
      kidx.resize(m);
      for (size_t i = 0; i < m; i++) kidx[i] = (uint32_t)i;
    }
    rc = verify_secp_templated_locked(ctx, m, ks ? nullptr : vals->pubkeys, ks, ks ? kidx.data() : nullptr,
                                      commit->sigs, &tmpl, 1, blob.data(), blob.size(), nullptr, flag.data(),
                                      commit->ts_seconds, commit->ts_nanos, valid.data());
    if (rc != CMTV_OK) return rc;
  } else {
    // partition (commit_typed_parts.h): a signature that is not 64 bytes, or
    // a secp256k1 key that is not 33, goes to no device: its verdict stays 0
    Part ed, secp, sr;
    size_t count[3] = {0, 0, 0};
    for (size_t j = 0; j < m; j++) count[key_types[J.plan_val[j]]]++;
    ed.reserve(count[CMTV_KEY_ED25519], 32);
    secp.reserve(count[CMTV_KEY_SECP256K1], 33);
    sr.reserve(count[CMTV_KEY_SR25519], 32);
    partition_plan(J, m, 0, 0, ed, secp, sr);
    phase_add(ctx, kPhPrepare, t0);

    auto scatter = [&](const Part& P) {
      for (size_t k = 0; k < P.size(); k++) valid[P.at[k]] = pv[k];
    };
    if (ed.size()) {
      pv.assign(ed.size(), 0);
      rc = verify_templated_locked(ctx, ed.size(), ed.pk.data(), ed.sg.data(), nullptr, &tmpl, 1, blob.data(),
                                   blob.size(), nullptr, ed.flag.data(), ed.sec.data(), ed.nanos.data(), mode,
                                   pv.data(), nullptr, nullptr, bound);
      if (rc != CMTV_OK) return rc;
      scatter(ed);
    }
    if (secp.size()) {
      pv.assign(secp.size(), 0);
      const cmtv_secp_keyset* ks = secp_keyset();
      rc = verify_secp_templated_locked(ctx, secp.size(), ks ? nullptr : secp.pk.data(), ks,
                                        ks ? secp.kidx.data() : nullptr, secp.sg.data(), &tmpl, 1, blob.data(),
                                        blob.size(), nullptr, secp.flag.data(), secp.sec.data(), secp.nanos.data(),
                                        pv.data());
      if (rc != CMTV_OK) return rc;
      scatter(secp);
    }
    if (sr.size()) {
      pv.assign(sr.size(), 0);
      std::vector<uint32_t> off(sr.size() + 1, 0);
      for (size_t k = 0; k < sr.size(); k++)
        off[k + 1] = off[k] + sb_msg_len(tmpl, sr.flag[k] != 0, sr.sec[k], sr.nanos[k]);
      std::vector<uint8_t> msgs(off.back() + 1);
      for (size_t k = 0; k < sr.size(); k++) {
        HostBytes out{msgs.data() + off[k]};
        sb_write(out, tmpl, blob.data(), sr.flag[k] != 0, sr.sec[k], sr.nanos[k]);
      }
      rc = verify_host_locked(ctx, sr.size(), sr.pk.data(), sr.sg.data(), msgs.data(), off.data(), kModeSr25519,
                              pv.data(), nullptr);
      if (rc != CMTV_OK) return rc;
      scatter(sr);
    }
  }

  const uint64_t t1 = phase_now(ctx);
  const uint8_t* v = valid.data();
  rc = job_replay(J, J.plan_idx.data(), m, [v](size_t j) { return v[j] != 0; }, seen);
  phase_add(ctx, kPhReplay, t1);
  return rc;
}

}  // namespace

extern "C" int cmtv_verify_commit_typed(cmtv_ctx* ctx, uint32_t kind, uint32_t mode, const char* chain_id,
                                        size_t chain_id_len, const cmtv_valset* vals, const uint8_t* key_types,
                                        const cmtv_block_id* block_id, int64_t height, const cmtv_commit* commit,
                                        uint64_t trust_num, uint64_t trust_den, cmtv_commit_result* res, char* msg_buf,
                                        size_t msg_cap) {
  // no C++ exception crosses the C ABI
  try {
    return verify_typed(ctx, kind, mode, chain_id, chain_id_len, vals, key_types, block_id, height, commit, trust_num,
                        trust_den, res, msg_buf, msg_cap);
  } catch (const std::bad_alloc&) {
    return CMTV_ENOMEM;
  } catch (...) {
    return CMTV_EINVAL;
  }
}
