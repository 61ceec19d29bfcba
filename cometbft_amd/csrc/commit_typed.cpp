// commit_typed.cpp -- VerifyCommit* over validator sets of Ed25519, secp256k1
// and sr25519 keys, and sets that mix them: one commit
// (cmtv_verify_commit_typed) and many heights in one call
// (cmtv_verify_commits_typed, the typed form of cmtv_verify_commits for
// blocksync and light-client replay: blockchain/v0/reactor.go:349-400,
// light/client.go:613-689), over one engine (TypedCall).
//
// The reference loop calls val.PubKey.VerifySignature(voteSignBytes, sig)
// (types/validator_set.go:695, 751, 812), which dispatches on the key's type.
// Here every commit is planned as commit.cpp plans it (commit_internal.h
// job_preamble / job_plan, with CommitJob::key_types set) and gets one
// sign-bytes template; the planned signatures of ALL commits are split by key
// type, each share is verified by its own batches, the verdicts are scattered
// back into plan order and the reference loop is replayed per commit
// (job_replay), so error, early exit, tally and string are the reference's.
// A commit that ends in its preamble costs no device work.
//
//   Ed25519    verify_templated_locked (key bytes) over the template array
//   secp256k1  verify_secp_templated_locked: the kernels build every
//              CanonicalVote from its commit's template on the device; by
//              registered keys when cmtv_keyset_cache is on and the whole set
//              is secp256k1 with keys packed at 33 bytes, else by key bytes
//   sr25519    sign-bytes written here on the host from the same templates
//              and the runtime's sr25519 host batch: there is no templated
//              sr25519 kernel yet
//
// Registered keys: consecutive commits whose sets hold the same keys (the
// pointer compared first, then the bytes, once per new set) form one group
// and one batch. Groups are verified one after another -- each blocking
// batch finishes before the next set is looked up -- so a call with more
// distinct sets than the cache holds never reads an evicted table.
//
// What the two entry points do differently is TypedOpts. A call with no key
// of another type is forwarded to cmtv_verify_commit / cmtv_verify_commits.
// Typed calls never enter the cross-height pipeline or the speculative path.
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
#include "runtime_internal.h"
#include "signbytes.h"

namespace {

using namespace cmtv;

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
  std::vector<uint32_t> tidx;  // the entry's commit template
  size_t size() const { return at.size(); }
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
           int64_t s, int32_t ns, uint32_t vi, uint32_t ti) {
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

// The planned signatures of J (J.plan_idx / J.plan_val), split by their
// validators' key types; plan item j gets verdict position J.first + j, and
// template ti_secp in the secp256k1 share, ti in the others. A signature that
// is not 64 bytes is wrong for every type before its key is looked at, and a
// secp256k1 key that is not 33 bytes fails ParsePubKey: neither goes to a
// device, their verdict stays 0.
void partition_plan(const CommitJob& J, uint32_t ti, uint32_t ti_secp, Part& ed, Part& secp, Part& sr) {
  const cmtv_valset* vals = J.vals;
  const cmtv_commit* commit = J.commit;
  for (size_t j = 0; j < J.plan_idx.size(); j++) {
    const uint32_t idx = J.plan_idx[j], vi = J.plan_val[j];
    const uint32_t s0 = commit->sig_off[idx], s1 = commit->sig_off[idx + 1];
    if (s1 - s0 != 64) continue;
    const uint8_t* key = vals->pubkeys + vals->pk_off[vi];
    const size_t kl = vals->pk_off[vi + 1] - vals->pk_off[vi];
    const bool for_block = commit->flags[idx] == kFlagCommit;
    const uint8_t t = J.key_type(vi);
    if (t == CMTV_KEY_SECP256K1 && kl != 33) continue;
    const bool is_secp = t == CMTV_KEY_SECP256K1;
    Part& P = t == CMTV_KEY_ED25519 ? ed : is_secp ? secp : sr;
    P.add((uint32_t)(J.first + j), key, kl, is_secp ? 33 : 32, commit->sigs + s0, for_block, commit->ts_seconds[idx],
          commit->ts_nanos[idx], vi, is_secp ? ti_secp : ti);
  }
}

// The key types of one validator set (null: all Ed25519). CMTV_EINVAL for a
// type above CMTV_KEY_SR25519 or a 65-byte secp256k1 key; *typed is set when a
// key is not Ed25519; *registrable: every key is secp256k1 and they are packed
// at 33 bytes, so the set can be registered and a key's index is its validator's
int check_key_types(const cmtv_valset* vs, const uint8_t* types, bool* typed, bool* registrable) {
  *registrable = types && vs->n_vals != 0 && vs->pk_off[vs->n_vals] == 33 * vs->n_vals;
  for (uint32_t i = 0; types && i < vs->n_vals; i++) {
    const uint8_t t = types[i];
    if (t > CMTV_KEY_SR25519) return CMTV_EINVAL;
    if (t == CMTV_KEY_SECP256K1 && vs->pk_off[i + 1] - vs->pk_off[i] == 65) return CMTV_EINVAL;
    *typed = *typed || t != CMTV_KEY_ED25519;
    *registrable = *registrable && t == CMTV_KEY_SECP256K1 && vs->pk_off[i] == 33 * i;
  }
  return CMTV_OK;
}

// What the entry points do differently
struct TypedOpts {
  // the call waits on its verdicts (one commit; many heights of <= 4096
  // signatures): note_latency, LatencyStreams
  bool latency;
  // many heights. Each share is split into runs whose sign-bytes span stays
  // below max_batch_msg_bytes() and ships its message offsets and template
  // indices, and the secp256k1 launches may share one inversion mod n among a
  // lane's signatures (SecpTemplated::bulk). Without it (one commit) a share
  // is one batch, past 2 GiB the runtime's CMTV_EINVAL; its signatures all
  // use template 0 (tidx null), and the Ed25519 share goes without offsets
  // under msg_len_bound, so the fused small-batch path can still run.
  bool many;
};

thread_local Seen seen;

// One typed call: begin(), then per commit plan() and add(), then verify()
// and replay().
struct TypedCall {
  cmtv_ctx* ctx;
  uint32_t mode;
  const char* chain_id;
  size_t chain_id_len;
  TypedOpts opt;
  std::unique_lock<std::mutex> lk;
  std::optional<LatencyStreams> lat;
  bool cache_on = false;
  uint64_t tp = 0;  // kPhPrepare runs since
  // one template per planned commit, their bytes back to back in the blob
  std::vector<SbTemplate> tmpls;
  std::vector<uint8_t> blob, valid, pv;
  // The shares; secp holds the current group only, verified when the group
  // ends. group_vs set: consecutive commits of one registrable set (by
  // registered keys when the cache gives the set); null: key bytes. A group
  // ships only its own commits' templates: g_tmpls, over the blob from
  // g_blob0 on.
  Part ed, secp, sr;
  const cmtv_valset* group_vs = nullptr;
  std::vector<SbTemplate> g_tmpls;
  size_t g_blob0 = 0;

  TypedCall(cmtv_ctx* c, uint32_t mode_, const char* cid, size_t cid_len, TypedOpts o, size_t n)
      : ctx(c), mode(mode_), chain_id(cid), chain_id_len(cid_len), opt(o), tmpls(n) {}

  int begin() {
    if (opt.latency) note_latency(ctx);
    const int rc = ctx_lock(ctx, lk);
    if (rc != CMTV_OK) return rc;
    if (opt.latency) lat.emplace(ctx);
    cache_on = keyset_cache_enabled(ctx);
    tp = phase_now(ctx);
    return CMTV_OK;
  }

  // preamble and plan; J.early != 1 when the preamble ended the commit
  void plan(CommitJob& J) {
    job_preamble(J);
    J.first = valid.size();
    if (J.early != 1) return;
    const uint32_t nsig = J.commit->n_sigs;
    J.plan_idx.resize(nsig);
    J.plan_val.resize(nsig);
    const size_t m = job_plan(J, J.plan_idx.data(), J.plan_val.data(), seen);
    J.plan_idx.resize(m);
    J.plan_val.resize(m);
    valid.resize(valid.size() + m, 0);
  }

  int put_template(const CommitJob& J, size_t c) {
    const size_t at = blob.size();
    blob.resize(at + put_commit_template(nullptr, 0, chain_id, chain_id_len, J.commit, nullptr));
    if (blob.size() >= (1ull << 32)) return CMTV_EINVAL;  // template offsets are 32-bit
    put_commit_template(blob.data(), at, chain_id, chain_id_len, J.commit, &tmpls[c]);
    return CMTV_OK;
  }

  // the registered set of vs's keys (a registered set's key index is the
  // validator index); vs null: none
  const cmtv_secp_keyset* keyset(const cmtv_valset* vs) {
    if (!vs) return nullptr;
    const uint64_t tk = phase_now(ctx);
    const cmtv_secp_keyset* ks = secp_keyset_for_locked(ctx, vs->pubkeys, vs->n_vals);
    phase_add(ctx, kPhKeyset, tk);
    return ks;
  }

  // f(a, b, off32) per run [a, b) of a share, its verdicts from pv into
  // `valid`. offsets: off32 holds the b - a + 1 message offsets from the
  // run's start (else null, and the share is one run). Many heights: a run's
  // sign-bytes span stays `slack` below the device's 32-bit offsets
  // (commit.cpp batch_verify's split).
  template <class F>
  int for_runs(const Part& P, const SbTemplate* tp_, uint64_t slack, bool offsets, F f) {
    const size_t m = P.size();
    const uint64_t cap = opt.many ? max_batch_msg_bytes() - slack : 1ull << 32;
    std::vector<uint32_t> off32;
    for (size_t a = 0; a < m;) {
      off32.assign(1, 0);
      uint64_t span = 0;
      size_t b = offsets ? a : m;
      while (b < m) {
        const uint32_t len = sb_msg_len(tp_[P.tidx[b]], P.flag[b] != 0, P.sec[b], P.nanos[b]);
        if (opt.many && b > a && span + len >= cap) break;
        span += len;
        off32.push_back((uint32_t)span);
        b++;
      }
      if (span >= cap) return CMTV_EINVAL;  // one message of 2 GiB (one commit: offsets past 32 bits)
      pv.assign(b - a, 0);
      const int rc = f(a, b, offsets ? off32.data() : nullptr);
      if (rc != CMTV_OK) return rc;
      for (size_t k = a; k < b; k++) valid[P.at[k]] = pv[k - a];
      a = b;
    }
    return CMTV_OK;
  }

  // verifies the current group's secp256k1 share and starts the next group
  int flush_secp() {
    const cmtv_secp_keyset* ks = secp.size() ? keyset(group_vs) : nullptr;
    // 32: the runtime wants 16 bytes after the last message below 2 GiB
    const int rc = for_runs(secp, g_tmpls.data(), 32, opt.many, [&](size_t a, size_t b, const uint32_t*) {
      const SecpTemplated q{b - a, ks ? nullptr : secp.pk.data() + 33 * a, ks, ks ? secp.kidx.data() + a : nullptr,
                            secp.sg.data() + 64 * a, g_tmpls.data(), g_tmpls.size(), blob.data() + g_blob0,
                            blob.size() - g_blob0, opt.many ? secp.tidx.data() + a : nullptr, secp.flag.data() + a,
                            secp.sec.data() + a, secp.nanos.data() + a, opt.many};
      return verify_secp_templated_locked(ctx, q, pv.data());
    });
    secp.clear();
    g_tmpls.clear();
    g_blob0 = blob.size();
    return rc;
  }

  // commit c (planned) joins the call: its group, its template, its
  // signatures into the three shares
  int add(const CommitJob& J, size_t c, bool registrable) {
    // the commit's group: the registrable set of the commit before (the same
    // key array, else equal key bytes: same_keys), a new one, or none
    const cmtv_valset* vs = cache_on && registrable ? J.vals : nullptr;
    const bool same = vs ? group_vs && same_keys(group_vs, vs) : !group_vs;
    int rc;
    // (an all-Ed25519 commit adds nothing to the group and ends none)
    if (!same && J.key_types) {
      phase_add(ctx, kPhPrepare, tp);
      if ((rc = flush_secp()) != CMTV_OK) return rc;
      tp = phase_now(ctx);
      group_vs = vs;
    }
    if ((rc = put_template(J, c)) != CMTV_OK) return rc;
    SbTemplate g = tmpls[c];  // the same template over the group's slice of the blob
    g.pre_commit_off -= (uint32_t)g_blob0;
    g.pre_nil_off -= (uint32_t)g_blob0;
    g.post_off -= (uint32_t)g_blob0;
    partition_plan(J, (uint32_t)c, (uint32_t)g_tmpls.size(), ed, secp, sr);
    g_tmpls.push_back(g);
    return CMTV_OK;
  }

  // the last group's secp256k1 share, then the Ed25519 and sr25519 shares of the whole call
  int verify() {
    phase_add(ctx, kPhPrepare, tp);
    int rc = flush_secp();
    if (rc != CMTV_OK) return rc;
    const uint32_t bound =
        opt.many ? 0 : msg_len_bound(TplLens{tmpls[0].pre_commit_len, tmpls[0].pre_nil_len, tmpls[0].post_len});
    rc = for_runs(ed, tmpls.data(), 0, opt.many, [&](size_t a, size_t b, const uint32_t* off32) {
      return verify_templated_locked(ctx, b - a, ed.pk.data() + 32 * a, ed.sg.data() + 64 * a, off32, tmpls.data(),
                                     tmpls.size(), blob.data(), blob.size(), opt.many ? ed.tidx.data() + a : nullptr,
                                     ed.flag.data() + a, ed.sec.data() + a, ed.nanos.data() + a, mode, pv.data(),
                                     nullptr, nullptr, bound);
    });
    if (rc != CMTV_OK) return rc;
    return for_runs(sr, tmpls.data(), 0, true, [&](size_t a, size_t b, const uint32_t* off32) {
      std::vector<uint8_t> msgs((size_t)off32[b - a] + 1);
      for (size_t k = a; k < b; k++) {
        HostBytes out{msgs.data() + off32[k - a]};
        sb_write(out, tmpls[sr.tidx[k]], blob.data(), sr.flag[k] != 0, sr.sec[k], sr.nanos[k]);
      }
      return verify_host_locked(ctx, b - a, sr.pk.data() + 32 * a, sr.sg.data() + 64 * a, msgs.data(), off32,
                                kModeSr25519, pv.data(), nullptr);
    });
  }

  // The common all-secp256k1 VerifyCommit: the plan is every signature in
  // index order, keys packed at 33 bytes and signatures at 64. The caller's
  // key, signature and timestamp arrays are then the batch itself (as
  // commit.cpp job_prepare_identity borrows them): only the flags, and with a
  // key set the identity key indices, are written.
  bool identity(const CommitJob& J, bool registrable) const {
    const size_t m = J.plan_idx.size();
    bool id = registrable && J.kind != CMTV_VERIFY_COMMIT_LIGHT_TRUSTING && m != 0 && m == J.commit->n_sigs &&
              m == J.vals->n_vals && J.plan_idx[m - 1] == m - 1;
    for (size_t i = 0; id && i <= m; i++) id = J.commit->sig_off[i] == 64 * i;
    return id;
  }
  int verify_identity(const CommitJob& J) {
    const cmtv_commit* commit = J.commit;
    const size_t m = J.plan_idx.size();
    const int rc = put_template(J, 0);
    if (rc != CMTV_OK) return rc;
    std::vector<uint8_t> flag(m);
    for (size_t i = 0; i < m; i++) flag[i] = commit->flags[i] == kFlagCommit;
    phase_add(ctx, kPhPrepare, tp);
    const cmtv_secp_keyset* ks = keyset(cache_on ? J.vals : nullptr);
    std::vector<uint32_t> kidx(ks ? m : 0);
    for (size_t i = 0; i < kidx.size(); i++) kidx[i] = (uint32_t)i;
    const SecpTemplated q{m, ks ? nullptr : J.vals->pubkeys, ks, ks ? kidx.data() : nullptr, commit->sigs,
                          tmpls.data(), 1, blob.data(), blob.size(), nullptr, flag.data(), commit->ts_seconds,
                          commit->ts_nanos};
    return verify_secp_templated_locked(ctx, q, valid.data());
  }

  void replay(CommitJob* jobs, size_t n, int* rcs) {
    const uint64_t t1 = phase_now(ctx);
    for (size_t c = 0; c < n; c++) {
      const uint8_t* v = valid.data() + jobs[c].first;
      rcs[c] = job_replay(jobs[c], jobs[c].plan_idx.data(), jobs[c].plan_idx.size(),
                          [v](size_t j) { return v[j] != 0; }, seen);
    }
    phase_add(ctx, kPhReplay, t1);
  }
};

int verify_commit_typed(cmtv_ctx* ctx, uint32_t kind, uint32_t mode, const char* chain_id, size_t chain_id_len,
                        const cmtv_valset* vals, const uint8_t* key_types, const cmtv_block_id* block_id,
                        int64_t height, const cmtv_commit* commit, uint64_t trust_num, uint64_t trust_den,
                        cmtv_commit_result* res, char* msg_buf, size_t msg_cap) {
  if (!ctx || mode > CMTV_MODE_ZIP215) return CMTV_EINVAL;
  int rc = job_check_args(kind, chain_id, chain_id_len, vals, block_id, commit, res);
  if (rc != CMTV_OK) return rc;
  bool typed = false, registrable = false;
  if ((rc = check_key_types(vals, key_types, &typed, &registrable)) != CMTV_OK) return rc;
  if (!typed)
    return cmtv_verify_commit(ctx, kind, mode, chain_id, chain_id_len, vals, block_id, height, commit, trust_num,
                              trust_den, res, msg_buf, msg_cap);

  CommitJob J{kind, chain_id, chain_id_len, vals, block_id, height, commit, trust_num, trust_den, res, msg_buf,
              msg_cap};
  J.key_types = key_types;
  AddrIndex addr;
  if (kind == CMTV_VERIFY_COMMIT_LIGHT_TRUSTING) {
    addr.build(vals->addrs, vals->n_vals);
    J.addr = &addr;
  }
  TypedCall T(ctx, mode, chain_id, chain_id_len, TypedOpts{true, false}, 1);
  if ((rc = T.begin()) != CMTV_OK) return rc;
  T.plan(J);
  if (J.early != 1) return J.early;
  if (T.identity(J, registrable))
    rc = T.verify_identity(J);
  else if ((rc = T.add(J, 0, registrable)) == CMTV_OK)
    rc = T.verify();
  if (rc != CMTV_OK) return rc;
  T.replay(&J, 1, &rc);
  return rc;
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
  std::vector<uint8_t> registrable(n);
  int rc;
  for (size_t c = 0; c < n; c++) {
    rc = job_check_args(kind, chain_id, chain_id_len, &vals[c], block_ids ? &block_ids[c] : nullptr, &commits[c],
                        &results[c]);
    if (rc != CMTV_OK) return rc;
    n_sigs += commits[c].n_sigs;
    bool reg = false;
    if ((rc = check_key_types(&vals[c], key_types ? key_types[c] : nullptr, &typed, &reg)) != CMTV_OK) return rc;
    registrable[c] = reg;
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
  // a small call waits on its verdicts
  TypedCall T(ctx, mode, chain_id, chain_id_len, TypedOpts{n_sigs <= 4096, true}, n);
  if ((rc = T.begin()) != CMTV_OK) return rc;
  for (size_t c = 0; c < n; c++) {
    T.plan(jobs[c]);
    if (jobs[c].early == 1 && (rc = T.add(jobs[c], c, registrable[c] != 0)) != CMTV_OK) return rc;
  }
  if ((rc = T.verify()) != CMTV_OK) return rc;
  T.replay(jobs.data(), n, rcs);
  return CMTV_OK;
}

// no C++ exception crosses the C ABI
template <class F>
int no_throw(F f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return CMTV_ENOMEM;
  } catch (...) {
    return CMTV_EINVAL;
  }
}

}  // namespace

extern "C" int cmtv_verify_commit_typed(cmtv_ctx* ctx, uint32_t kind, uint32_t mode, const char* chain_id,
                                        size_t chain_id_len, const cmtv_valset* vals, const uint8_t* key_types,
                                        const cmtv_block_id* block_id, int64_t height, const cmtv_commit* commit,
                                        uint64_t trust_num, uint64_t trust_den, cmtv_commit_result* res, char* msg_buf,
                                        size_t msg_cap) {
  return no_throw([&] {
    return verify_commit_typed(ctx, kind, mode, chain_id, chain_id_len, vals, key_types, block_id, height, commit,
                               trust_num, trust_den, res, msg_buf, msg_cap);
  });
}

extern "C" int cmtv_verify_commits_typed(cmtv_ctx* ctx, uint32_t kind, uint32_t mode, const char* chain_id,
                                         size_t chain_id_len, size_t n, const cmtv_valset* vals,
                                         const uint8_t* const* key_types, const cmtv_block_id* block_ids,
                                         const int64_t* heights, const cmtv_commit* commits, uint64_t trust_num,
                                         uint64_t trust_den, cmtv_commit_result* results, int* rcs, char* msg_bufs,
                                         size_t msg_cap) {
  return no_throw([&] {
    return verify_commits_typed(ctx, kind, mode, chain_id, chain_id_len, n, vals, key_types, block_ids, heights,
                                commits, trust_num, trust_den, results, rcs, msg_bufs, msg_cap);
  });
}
