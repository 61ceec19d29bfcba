// commit.cpp -- host side above the device verifier: CanonicalVote sign-bytes,
// the crypto.BatchVerifier mirror and the VerifyCommit* replay.
//
// The reference verifies a commit with a sequential loop that calls
// PubKey.VerifySignature per CommitSig (types/validator_set.go:667-826). Here
// the signatures that loop could reach are verified in ONE device batch and the
// loop is then replayed in index order over the verdicts, so the returned
// error (first bad signature, early exits, tallies, panics) is exactly the
// reference's. Error strings are produced with the reference's formats.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cinttypes>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <new>
#include <optional>
#include <random>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/cmtverify.h"
#include "commit_internal.h"
#include "runtime_internal.h"
#include "signbytes.h"

namespace cmtv {

uint64_t AddrIndex::key() {
  static const uint64_t k = [] {
    std::random_device rd;
    return ((uint64_t)rd() << 32) ^ rd();
  }();
  return k;
}

// Two validator sets hold the same keys (so one registered key set serves
// both): the same arrays, or equal key bytes.
bool same_keys(const cmtv_valset* a, const cmtv_valset* b) {
  if (a == b) return true;
  if (a->n_vals != b->n_vals) return false;
  if (a->pubkeys == b->pubkeys && a->pk_off == b->pk_off) return true;
  for (uint32_t i = 0; i <= a->n_vals; i++)
    if (a->pk_off[i] != b->pk_off[i]) return false;
  const uint32_t bytes = a->pk_off[a->n_vals];
  return bytes == 0 || std::memcmp(a->pubkeys, b->pubkeys, bytes) == 0;
}

}  // namespace cmtv

namespace {

using namespace cmtv;

// VoteSignBytes (types/vote.go:93): uvarint(len) || CanonicalVote
// (canonical.pb.go:517-567; Timestamp = gogoproto StdTime {1: seconds, 2: nanos})
void put_vote(ByteWriter& w, const char* chain_id, size_t chain_id_len, int32_t vtype, int64_t height, int32_t round,
              const cmtv_block_id* bid, int64_t ts_sec, int32_t ts_nanos) {
  put_vote_prefix(w, vtype, height, round, bid);
  const size_t ts = (ts_sec != 0 ? 1 + uvarint_len((uint64_t)ts_sec) : 0) +
                    (ts_nanos != 0 ? 1 + uvarint_len((uint64_t)(int64_t)ts_nanos) : 0);
  w.byte(0x2A);
  w.uvarint(ts);
  if (ts_sec != 0) {
    w.byte(0x08);
    w.uvarint((uint64_t)ts_sec);
  }
  if (ts_nanos != 0) {
    w.byte(0x10);
    w.uvarint((uint64_t)(int64_t)ts_nanos);
  }
  if (chain_id_len) w.bytes_field(0x32, reinterpret_cast<const uint8_t*>(chain_id), chain_id_len);
}

void vote_sign_bytes(std::string& out, const char* chain_id, size_t chain_id_len, int32_t vtype, int64_t height,
                     int32_t round, const cmtv_block_id* bid, int64_t ts_sec, int32_t ts_nanos) {
  ByteWriter cnt;
  put_vote(cnt, chain_id, chain_id_len, vtype, height, round, bid, ts_sec, ts_nanos);
  const size_t body = cnt.n;
  out.resize(uvarint_len(body) + body);
  ByteWriter w{reinterpret_cast<uint8_t*>(&out[0]), 0};
  w.uvarint(body);
  put_vote(w, chain_id, chain_id_len, vtype, height, round, bid, ts_sec, ts_nanos);
}

// BlockID.String() (types/block.go:1217): "%v:%v" Hash, PartSetHeader
// PartSetHeader.String() (types/part_set.go:103): "%v:%X" Total, Fingerprint(Hash)
std::string block_id_string(const cmtv_block_id* b) {
  uint8_t fp[6] = {0};
  if (b && b->psh_hash_len) std::memcpy(fp, b->psh_hash, b->psh_hash_len < 6 ? b->psh_hash_len : 6);
  std::string s = b ? hex_upper(b->hash, b->hash_len) : std::string();
  s += ":" + std::to_string(b ? b->psh_total : 0) + ":" + hex_upper(fp, 6);
  return s;
}

bool block_id_equals(const cmtv_block_id* a, const cmtv_block_id* b) {
  auto eq = [](const uint8_t* x, uint32_t nx, const uint8_t* y, uint32_t ny) {
    return nx == ny && (nx == 0 || std::memcmp(x, y, nx) == 0);
  };
  return eq(a->hash, a->hash_len, b->hash, b->hash_len) && a->psh_total == b->psh_total &&
         eq(a->psh_hash, a->psh_hash_len, b->psh_hash, b->psh_hash_len);
}

// ------------------------------------------------------------------ VerifyCommit*

// Signatures of one or more commits, gathered for one device batch. Host
// mode: sign-bytes encoded here (needed for the verdict cache's keys).
// Templated mode: one SbTemplate per commit and
// (flag, seconds, nanos) per signature; the device writes the sign-bytes.
// Message offsets are 64-bit here: a cross-height batch can exceed 4 GiB of
// sign-bytes, and batch_verify splits it into device batches below 2 GiB.
struct SigBatch {
  bool templated = false;
  std::vector<uint8_t> pk, sg, msgs, len_ok;
  std::vector<uint64_t> off{0};
  // borrowed (templated, one commit whose plan is every signature in order,
  // keys and signatures packed at 32 / 64 bytes): the caller's arrays are the
  // batch, nothing is copied per signature (job_prepare_identity)
  const uint8_t* pk_src = nullptr;
  const uint8_t* sg_src = nullptr;
  const int64_t* sec_src = nullptr;
  const int32_t* nanos_src = nullptr;
  bool all_len_ok = false;  // every signature is 64 bytes (len_ok unused)
  std::string sb;
  // templated
  std::vector<cmtv::SbTemplate> tmpls;
  std::vector<uint8_t> blob, tflag;
  std::vector<uint32_t> tidx;
  std::vector<int64_t> tsec;
  std::vector<int32_t> tnanos;
  const cmtv_commit* cur = nullptr;  // commit of the last template
  // validator indices, for registered-key verification when every signature
  // comes from validator sets with the same keys (cmtv_keyset_cache)
  std::vector<uint32_t> kidx;
  const cmtv_valset* vs = nullptr;
  const cmtv_valset* last_vs = nullptr;
  bool one_vs = true;

  // the one-pass form of a single commit (job_prepare_fast): no message
  // offsets (the runtime derives them only for a form that reads them), every
  // message at most msg_bound bytes; keys checked packed
  bool fast = false, keys_packed = false;
  uint32_t msg_bound = 0;

  size_t size() const { return fast ? tflag.size() : off.size() - 1; }
  const uint8_t* pk_data() const { return pk_src ? pk_src : pk.data(); }
  const uint8_t* sg_data() const { return sg_src ? sg_src : sg.data(); }
  const int64_t* sec_data() const { return sec_src ? sec_src : tsec.data(); }
  const int32_t* nanos_data() const { return nanos_src ? nanos_src : tnanos.data(); }

  // room for m more signatures (no reallocation inside add); grows
  // geometrically, since a cross-height batch calls it once per commit
  template <class V>
  static void grow(V& v, size_t want) {
    if (v.capacity() < want) v.reserve(std::max(want, 2 * v.capacity()));
  }
  void reserve_more(size_t m) {
    const size_t n = size() + m;
    grow(pk, 32 * n);
    grow(sg, 64 * n);
    grow(len_ok, n);
    grow(off, n + 1);
    grow(kidx, n);
    if (templated) {
      grow(tidx, n);
      grow(tflag, n);
      grow(tsec, n);
      grow(tnanos, n);
    }
  }

  void ensure_template(const char* chain_id, size_t chain_id_len, const cmtv_commit* c) {
    if (cur == c && !tmpls.empty()) return;
    cmtv::SbTemplate t{};
    const size_t at = blob.size();
    blob.resize(at + put_commit_template(nullptr, 0, chain_id, chain_id_len, c, nullptr));
    put_commit_template(blob.data(), at, chain_id, chain_id_len, c, &t);
    tmpls.push_back(t);
    cur = c;
  }

  // key (32 bytes), the CommitSig's signature and the vote's sign-bytes
  void add(const cmtv_valset* vals, uint32_t vi, const uint8_t* sig, uint32_t sig_len, const char* chain_id,
           size_t chain_id_len, const cmtv_commit* c, uint32_t idx) {
    static const cmtv_block_id empty{};
    const uint8_t* key = vals->pubkeys + vals->pk_off[vi];
    if (!vs) vs = last_vs = vals;
    if (one_vs && vals != last_vs) {  // compare each new set once
      one_vs = same_keys(vs, vals);
      last_vs = vals;
    }
    kidx.push_back(vi);
    const size_t ok = pk.size();
    pk.resize(ok + 32);
    std::memcpy(&pk[ok], key, 32);
    const size_t o = sg.size();
    sg.resize(o + 64);
    if (sig_len == 64)
      std::memcpy(&sg[o], sig, 64);
    else
      std::memset(&sg[o], 0, 64);
    len_ok.push_back(sig_len == 64);
    // Commit.GetVote(idx) (types/block.go:784): CommitSig.BlockID(commit.BlockID)
    const bool for_block = c->flags[idx] == kFlagCommit;
    if (templated) {
      ensure_template(chain_id, chain_id_len, c);
      tidx.push_back((uint32_t)tmpls.size() - 1);
      tflag.push_back(for_block ? 1 : 0);
      tsec.push_back(c->ts_seconds[idx]);
      tnanos.push_back(c->ts_nanos[idx]);
      off.push_back(off.back() + cmtv::sb_msg_len(tmpls.back(), for_block, c->ts_seconds[idx], c->ts_nanos[idx]));
      return;
    }
    vote_sign_bytes(sb, chain_id, chain_id_len, kPrecommit, c->height, c->round, for_block ? &c->block_id : &empty,
                    c->ts_seconds[idx], c->ts_nanos[idx]);
    msgs.insert(msgs.end(), sb.begin(), sb.end());
    off.push_back(msgs.size());
  }
};

// CMTV_HOST_SIGNBYTES=1 forces host-side encoding (A/B measurement, tests)
bool templated_enabled() {
  static const bool on = [] {
    const char* v = std::getenv("CMTV_HOST_SIGNBYTES");
    return !(v && v[0] == '1');
  }();
  return on;
}

// A single commit whose plan is a prefix of its signatures (VerifyCommit: no
// absent or unknown flags; VerifyCommitLight: no nil votes before the
// threshold) with keys packed at 32 bytes and signatures at 64: one pass
// plans it and writes the per-signature flag (the caller's key, signature and
// timestamp arrays are the batch; no message offsets: every message is at
// most msg_len_bound bytes, and the fused kernels the runtime picks for such
// a batch build each message from the template -- host_batch.cpp
// verify_templated_locked derives the offsets for any other form).
// False (B left empty) sends it down the general path.
bool job_prepare_fast(CommitJob& J, SigBatch& B) {
  const cmtv_valset* vals = J.vals;
  const cmtv_commit* c = J.commit;
  const uint32_t n = c->n_sigs;
  const bool full = J.kind == CMTV_VERIFY_COMMIT;
  if (J.kind == CMTV_VERIFY_COMMIT_LIGHT_TRUSTING || !B.templated || B.size() != 0 || n == 0 || n != vals->n_vals)
    return false;
  if (vals->pk_off[0] != 0 || c->sig_off[0] != 0) return false;
  SbTemplate t{};
  const size_t tb = put_commit_template(nullptr, 0, J.chain_id, J.chain_id_len, c, &t);
  const TplLens tl{t.pre_commit_len, t.pre_nil_len, t.post_len};
  const uint32_t bound = msg_len_bound(tl);
  if ((uint64_t)bound * n + 16 >= (1ull << 31)) return false;
  B.tflag.resize(n);
  uint8_t* tf = B.tflag.data();
  const uint8_t* fl = c->flags;
  const uint32_t* po = vals->pk_off;
  const uint32_t* so = c->sig_off;
  const int64_t* vp = vals->voting_power;
  int64_t tally = 0;
  uint32_t m = 0;
  auto bail = [&] {  // leave B as it was
    B.tflag.clear();
    return false;
  };
  if (full) {
    // branch-free passes the compiler vectorises: offsets, flags, tally
    uint32_t bad = 0;
    for (uint32_t i = 1; i <= n; i++) bad |= (po[i] ^ (32u * i)) | (so[i] ^ (64u * i));
    for (uint32_t i = 0; i < n; i++) {
      const uint8_t f = fl[i];
      const uint8_t fb = f == kFlagCommit;
      bad |= (uint32_t)(!fb & (f != kFlagNil));
      tf[i] = fb;
      tally += fb ? vp[i] : 0;
    }
    if (bad) return bail();
    m = n;
  } else {
    for (uint32_t i = 0; i < n; i++) {
      if (fl[i] != kFlagCommit) return bail();
      if (po[i + 1] != 32 * (i + 1) || so[i + 1] != 64 * (i + 1)) return bail();
      tf[i] = 1;
      m = i + 1;
      tally += vp[i];
      if (tally > J.needed) break;
    }
  }
  B.tflag.resize(m);
  B.msg_bound = bound;
  B.fast = true;
  B.keys_packed = full;  // every key checked (a light plan stops early)
  // no key index or template index arrays: signature i is by validator i
  // and every one uses template 0 (null key_idx / tidx downstream)
  B.tmpls.assign(1, t);
  B.blob.resize(tb);
  put_commit_template(B.blob.data(), 0, J.chain_id, J.chain_id_len, c, &B.tmpls[0]);
  B.cur = c;
  B.pk_src = vals->pubkeys;
  B.sg_src = c->sigs;
  B.sec_src = c->ts_seconds;
  B.nanos_src = c->ts_nanos;
  B.all_len_ok = true;
  B.vs = B.last_vs = vals;
  B.one_vs = true;
  J.plan_prefix = m;
  J.prefix_tally = tally;
  J.first = 0;
  return true;
}

// The common VerifyCommit case (validator_set.go:685-707): the plan is every
// signature in index order, from validators whose keys are packed at 32 bytes,
// and every signature is 64 bytes. Then the caller's key, signature and
// timestamp arrays are the batch itself (SigBatch's borrowed pointers): only
// the per-signature flag and message offset are written here, and the batch
// goes to the pinned staging in one copy. Applies to a templated batch of
// this one job; false leaves B untouched.
bool job_prepare_identity(CommitJob& J, SigBatch& B, bool prefetch) {
  const cmtv_valset* vals = J.vals;
  const cmtv_commit* c = J.commit;
  const size_t m = J.plan_idx.size();
  if (J.kind == CMTV_VERIFY_COMMIT_LIGHT_TRUSTING) return false;  // its plan maps through addresses
  if (!B.templated || prefetch || B.size() != 0 || m == 0 || m != c->n_sigs || m != vals->n_vals) return false;
  if (J.plan_idx.back() != m - 1) return false;  // the plan is increasing: last == m - 1 <=> identity
  for (size_t i = 0; i <= m; i++)
    if (vals->pk_off[i] != 32 * i || c->sig_off[i] != 64 * i) return false;
  B.pk_src = vals->pubkeys;
  B.sg_src = c->sigs;
  B.sec_src = c->ts_seconds;
  B.nanos_src = c->ts_nanos;
  B.all_len_ok = true;
  B.vs = B.last_vs = vals;
  B.one_vs = true;
  B.ensure_template(J.chain_id, J.chain_id_len, c);
  const cmtv::SbTemplate& t = B.tmpls.back();
  const TplLens tl{t.pre_commit_len, t.pre_nil_len, t.post_len};
  B.tflag.resize(m);
  B.tidx.assign(m, (uint32_t)B.tmpls.size() - 1);
  B.off.resize(m + 1);
  B.kidx.resize(m);
  uint64_t o = 0;
  const uint8_t* fl = c->flags;
  const int64_t* se = c->ts_seconds;
  const int32_t* na = c->ts_nanos;
  uint8_t* tf = B.tflag.data();
  uint32_t* ki = B.kidx.data();
  uint64_t* of = B.off.data();
  for (size_t i = 0; i < m; i++) {
    const bool for_block = fl[i] == kFlagCommit;
    tf[i] = for_block ? 1 : 0;
    ki[i] = (uint32_t)i;
    o += msg_len(tl, for_block, se[i], na[i]);
    of[i + 1] = o;
  }
  return true;
}

}  // namespace

namespace cmtv {

int job_check_args(uint32_t kind, const char* chain_id, size_t chain_id_len, const cmtv_valset* vals,
                   const cmtv_block_id* block_id, const cmtv_commit* commit, cmtv_commit_result* res) {
  if (!vals || !commit || !res || kind > CMTV_VERIFY_COMMIT_LIGHT_TRUSTING) return CMTV_EINVAL;
  if ((!chain_id && chain_id_len) || (vals->n_vals && (!vals->pubkeys || !vals->pk_off || !vals->voting_power)))
    return CMTV_EINVAL;
  const uint32_t nsig = commit->n_sigs;
  if (nsig && (!commit->flags || !commit->ts_seconds || !commit->ts_nanos || !commit->sigs || !commit->sig_off))
    return CMTV_EINVAL;
  if (kind == CMTV_VERIFY_COMMIT_LIGHT_TRUSTING && nsig && (!commit->val_addrs || (vals->n_vals && !vals->addrs)))
    return CMTV_EINVAL;
  if (kind != CMTV_VERIFY_COMMIT_LIGHT_TRUSTING && !block_id) return CMTV_EINVAL;
  return CMTV_OK;
}

void job_preamble(CommitJob& J) {
  const cmtv_valset* vals = J.vals;
  const cmtv_commit* commit = J.commit;
  std::memset(J.res, 0, sizeof(*J.res));
  J.res->sig_index = -1;
  set_msg(J.msg_buf, J.msg_cap, "");
  const uint32_t nsig = commit->n_sigs;
  int64_t total = J.total;
  if (!J.has_total)
    for (uint32_t i = 0; i < vals->n_vals; i++) total += vals->voting_power[i];

  if (J.kind == CMTV_VERIFY_COMMIT_LIGHT_TRUSTING) {
    if (J.trust_den == 0) {
      J.early = J.fail(CMTV_COMMIT_ERR_TRUST_LEVEL, -1, "trustLevel has zero Denominator");
      return;
    }
    // safeMul (types/validator_set.go:1086-1105) with Go's wrapping int64
    // arithmetic: -MinInt64 stays MinInt64, MaxInt64 / MinInt64 == 0
    const int64_t a = total, b = (int64_t)J.trust_num;
    int64_t prod = 0;
    bool overflow = false;
    if (a != 0 && b != 0) {
      const int64_t abs_b = b < 0 ? (int64_t)(0 - (uint64_t)b) : b;
      const int64_t abs_a = a < 0 ? (int64_t)(0 - (uint64_t)a) : a;
      overflow = abs_a > INT64_MAX / abs_b;
      if (!overflow) prod = (int64_t)((uint64_t)a * (uint64_t)b);
    }
    if (overflow) {
      J.early = J.fail(CMTV_COMMIT_ERR_TRUST_LEVEL, -1,
                       "int64 overflow while calculating voting power needed. please provide smaller trustLevel "
                       "numerator");
      return;
    }
    // Go: MinInt64 / -1 == MinInt64 (no trap); the zero denominator is
    // rejected above
    const int64_t den = (int64_t)J.trust_den;
    J.needed = (den == -1) ? (int64_t)(0 - (uint64_t)prod) : prod / den;
  } else {
    if (vals->n_vals != nsig) {
      char b[128];
      std::snprintf(b, sizeof b, "Invalid commit -- wrong set size: %u vs %u", vals->n_vals, nsig);
      J.early = J.fail(CMTV_COMMIT_ERR_SET_SIZE, -1, b);
      return;
    }
    if (J.height != commit->height) {
      char b[128];
      std::snprintf(b, sizeof b, "Invalid commit -- wrong height: %" PRId64 " vs %" PRId64, J.height, commit->height);
      J.early = J.fail(CMTV_COMMIT_ERR_HEIGHT, -1, b);
      return;
    }
    if (!block_id_equals(J.block_id, &commit->block_id)) {
      J.early = J.fail(CMTV_COMMIT_ERR_BLOCK_ID, -1,
                       "invalid commit -- wrong block ID: want " + block_id_string(J.block_id) + ", got " +
                           block_id_string(&commit->block_id));
      return;
    }
    J.needed = total * 2 / 3;
  }
}

// The plan: which signatures the reference loop can reach, assuming every
// verdict is valid (the loop stops at its first error, so nothing beyond the
// plan is ever examined).
size_t job_plan(const CommitJob& J, uint32_t* pidx, uint32_t* pval, Seen& seen) {
  const cmtv_valset* vals = J.vals;
  const cmtv_commit* commit = J.commit;
  const uint32_t nsig = commit->n_sigs;
  const bool trusting = J.kind == CMTV_VERIFY_COMMIT_LIGHT_TRUSTING;
  if (trusting) seen.reset(vals->n_vals);
  int64_t tally = 0;
  size_t m = 0;
  for (uint32_t idx = 0; idx < nsig; idx++) {
    const uint8_t flag = commit->flags[idx];
    uint32_t vi = idx;
    if (J.kind == CMTV_VERIFY_COMMIT) {
      if (flag == kFlagAbsent) continue;
      if (flag != kFlagCommit && flag != kFlagNil) break;  // panics here
    } else {
      if (flag != kFlagCommit) continue;
      if (trusting) {
        const int64_t f = J.addr->find(commit->val_addrs + 20 * (size_t)idx);
        if (f < 0) continue;
        vi = (uint32_t)f;
        uint32_t first = 0;
        if (seen.has(vi, &first)) break;  // double vote error here
        seen.put(vi, idx);
      }
    }
    // panics here (an Ed25519 key only: the other types' VerifySignature
    // returns false for a key it cannot use, a verdict like any other)
    if (J.key_type(vi) == CMTV_KEY_ED25519 && vals->pk_off[vi + 1] - vals->pk_off[vi] != 32) break;
    pidx[m] = idx;
    if (pval) pval[m] = vi;
    m++;
    if (J.kind != CMTV_VERIFY_COMMIT) {
      tally += vals->voting_power[vi];
      if (tally > J.needed) break;
    }
  }
  return m;
}

// Largest message span of one device batch (offsets are 32-bit on the
// device); CMTV_MAX_BATCH_MSG_BYTES lowers it (tests of the split).
uint64_t max_batch_msg_bytes() {
  const char* v = std::getenv("CMTV_MAX_BATCH_MSG_BYTES");
  const uint64_t x = v ? std::strtoull(v, nullptr, 10) : 0;
  return (x && x < (1ull << 31)) ? x : (1ull << 31);
}

}  // namespace cmtv

namespace {

// Preamble, plan and the planned signatures appended to B; with `prefetch`
// a light call also appends its commit's other non-absent signatures
// (verdicts for the verdict cache only).
void job_prepare(CommitJob& J, SigBatch& B, bool prefetch, bool only_job, Seen& seen) {
  const cmtv_valset* vals = J.vals;
  const cmtv_commit* commit = J.commit;
  job_preamble(J);
  if (J.early != 1) {
    J.first = B.size();
    return;
  }
  if (only_job && !prefetch && job_prepare_fast(J, B)) return;
  const uint32_t nsig = commit->n_sigs;
  J.plan_idx.resize(nsig);
  if (J.kind == CMTV_VERIFY_COMMIT_LIGHT_TRUSTING) J.plan_val.resize(nsig);
  const size_t m = job_plan(J, J.plan_idx.data(), J.kind == CMTV_VERIFY_COMMIT_LIGHT_TRUSTING ? J.plan_val.data()
                                                                                              : nullptr, seen);
  J.plan_idx.resize(m);
  const bool trusting = J.kind == CMTV_VERIFY_COMMIT_LIGHT_TRUSTING;
  if (trusting) J.plan_val.resize(m);  // else the validator index is the commit index
  J.first = B.size();
  // borrowing the caller's arrays: only when no other job adds to the batch
  if (only_job && job_prepare_identity(J, B, prefetch)) return;
  B.reserve_more(J.plan_idx.size());
  for (size_t j = 0; j < J.plan_idx.size(); j++) {
    const uint32_t idx = J.plan_idx[j], vi = trusting ? J.plan_val[j] : idx;
    const uint32_t s0 = commit->sig_off[idx], s1 = commit->sig_off[idx + 1];
    B.add(vals, vi, commit->sigs + s0, s1 - s0, J.chain_id, J.chain_id_len, commit, idx);
  }
  if (prefetch && J.kind == CMTV_VERIFY_COMMIT_LIGHT) {
    // the VerifyCommit calls that follow a light call in blocksync verify
    // every non-absent signature: verify the rest now, in the same batch
    std::vector<uint8_t> planned(nsig, 0);
    for (uint32_t idx : J.plan_idx) planned[idx] = 1;
    for (uint32_t idx = 0; idx < nsig; idx++) {
      const uint8_t flag = commit->flags[idx];
      if (planned[idx] || (flag != kFlagCommit && flag != kFlagNil)) continue;
      if (vals->pk_off[idx + 1] - vals->pk_off[idx] != 32) continue;
      const uint32_t s0 = commit->sig_off[idx], s1 = commit->sig_off[idx + 1];
      B.add(vals, idx, commit->sigs + s0, s1 - s0, J.chain_id, J.chain_id_len, commit, idx);
    }
  }
}

int batch_verify(cmtv_ctx* ctx, SigBatch& B, uint32_t mode, std::vector<uint8_t>& valid) {
  const size_t m = B.size();
  valid.assign(m, 0);
  if (!m) return CMTV_OK;
  // one validator set of 32-byte keys: its registered key set (built on
  // first use by cmtv_keyset_cache) replaces decompression and doublings
  const cmtv_keyset* ks = nullptr;
  if (B.templated && cmtv::keyset_cache_enabled(ctx) && B.one_vs && B.vs->n_vals) {
    bool packed = true;
    if (!B.keys_packed)
      for (uint32_t i = 0; i <= B.vs->n_vals && packed; i++) packed = B.vs->pk_off[i] == 32 * i;
    const uint64_t tk = cmtv::phase_now(ctx);
    if (packed) ks = cmtv::keyset_for_locked(ctx, B.vs->pubkeys, B.vs->n_vals);
    cmtv::phase_add(ctx, cmtv::kPhKeyset, tk);
  }
  if (B.fast)  // one device batch, message offsets left to the runtime (job_prepare_fast)
    return cmtv::verify_templated_locked(ctx, m, ks ? nullptr : B.pk_data(), B.sg_data(), nullptr, B.tmpls.data(), 1,
                                         B.blob.data(), B.blob.size(), nullptr, B.tflag.data(), B.sec_data(),
                                         B.nanos_data(), mode, valid.data(), ks, nullptr, B.msg_bound);
  if (!B.templated && B.msgs.empty()) B.msgs.push_back(0);
  std::vector<uint32_t> off32;
  const uint64_t kMaxBatchMsgBytes = max_batch_msg_bytes();
  for (size_t a = 0; a < m;) {
    // [a, b): the longest run whose sign-bytes span < 2 GiB
    size_t b = a + 1;
    while (b < m && B.off[b + 1] - B.off[a] < kMaxBatchMsgBytes) b++;
    if (B.off[b] - B.off[a] >= kMaxBatchMsgBytes) return CMTV_EINVAL;  // one message of >= 2 GiB
    off32.resize(b - a + 1);
    for (size_t i = a; i <= b; i++) off32[i - a] = (uint32_t)(B.off[i] - B.off[a]);
    int rc;
    if (B.templated)
      rc = cmtv::verify_templated_locked(ctx, b - a, ks ? nullptr : B.pk_data() + 32 * a, B.sg_data() + 64 * a,
                                         off32.data(), B.tmpls.data(), B.tmpls.size(), B.blob.data(), B.blob.size(),
                                         B.tidx.data() + a, B.tflag.data() + a, B.sec_data() + a,
                                         B.nanos_data() + a, mode, valid.data() + a, ks, B.kidx.data() + a);
    else
      rc = cmtv::verify_host_locked(ctx, b - a, B.pk.data() + 32 * a, B.sg.data() + 64 * a,
                                    B.msgs.data() + B.off[a], off32.data(), mode, valid.data() + a, nullptr);
    if (rc != CMTV_OK) return rc;
    a = b;
  }
  if (!B.all_len_ok)
    for (size_t j = 0; j < m; j++)
      if (!B.len_ok[j]) valid[j] = 0;  // crypto/ed25519/ed25519.go:150
  return CMTV_OK;
}

// job_replay over a batch's verdict bytes
int job_replay_batch(CommitJob& J, const std::vector<uint8_t>& all_valid, Seen& seen) {
  const uint8_t* v = all_valid.data() + J.first;
  if (J.plan_prefix) {
    // job_prepare_fast checked every flag, key and signature length of the
    // prefix
    if (J.early != 1) return J.early;
    const void* z = std::memchr(v, 0, J.plan_prefix);
    return replay_prefix(J, J.plan_prefix, J.prefix_tally,
                         z ? (size_t)(static_cast<const uint8_t*>(z) - v) : J.plan_prefix);
  }
  return job_replay(J, J.plan_idx.data(), J.plan_idx.size(), [v](size_t j) { return v[j] != 0; }, seen);
}

// Speculative VerifyCommit (round 6, VERDICT r5 item 3: the host share of the
// node's keyset-cache VerifyCommit at configs[1]). A large commit whose set's
// key array is the one the keyset cache matched last time (same pointer and
// count: keyset_guess_locked) launches its registered-key kernel over ALL n
// signatures before anything per signature is checked on the host -- only
// the preamble's height / BlockID / size, the two ends of the key and
// signature offset arrays, and one pass writing each signature's
// Commit-or-not flag. While the kernel runs, the host does what normally
// precedes the launch: the full preamble (total power), job_prepare_fast's
// flag / offset / tally passes, and the byte compare of the keys against the
// guessed set. If all of it holds, the verdicts are the one-batch path's
// (the same kernel over the same bytes; the plan is a prefix of the n) and
// the reference loop is replayed over the prefix; otherwise they are
// discarded (after the kernel finishes) and the normal path runs. Returns
// true with *rc set when the speculation was taken.
bool verify_commit_spec(cmtv_ctx* ctx, const CommitJob& J0, uint32_t mode, Seen& seen, int* rc) {
  // the context's threshold (keyset.cpp spec_min: 0 = off)
  const uint32_t kSpecMin = cmtv::spec_min(ctx);
  const cmtv_valset* vals = J0.vals;
  const cmtv_commit* c = J0.commit;
  const uint32_t n = c->n_sigs;
  if (!kSpecMin || J0.kind == CMTV_VERIFY_COMMIT_LIGHT_TRUSTING || n < kSpecMin || n != vals->n_vals) return false;
  if (J0.height != c->height || !block_id_equals(J0.block_id, &c->block_id)) return false;
  if (c->sig_off[0] != 0 || c->sig_off[n] != 64ull * n || vals->pk_off[0] != 0 || vals->pk_off[n] != 32ull * n)
    return false;
  const cmtv_keyset* ks = cmtv::keyset_guess_locked(ctx, vals->pubkeys, n);
  if (!ks) return false;
  SigBatch B;
  B.templated = true;
  SbTemplate t{};
  const size_t tb = put_commit_template(nullptr, 0, J0.chain_id, J0.chain_id_len, c, &t);
  const uint32_t bound = msg_len_bound(TplLens{t.pre_commit_len, t.pre_nil_len, t.post_len});
  B.tmpls.assign(1, t);
  B.blob.resize(tb);
  put_commit_template(B.blob.data(), 0, J0.chain_id, J0.chain_id_len, c, &B.tmpls[0]);
  B.tflag.resize(n);
  const uint8_t* fl = c->flags;
  uint8_t* tf = B.tflag.data();
  for (uint32_t i = 0; i < n; i++) tf[i] = fl[i] == kFlagCommit;  // vectorised
  // while the kernel runs: everything the launch skipped
  CommitJob J = J0;
  bool ok = false;
  const std::function<bool()> check = [&] {
    job_preamble(J);
    if (J.early != 1) return false;  // its error: the normal path reports it
    SigBatch V;
    V.templated = true;
    if (!job_prepare_fast(J, V)) return false;
    return cmtv::keyset_holds_locked(ks, vals->pubkeys, n);
  };
  std::vector<uint8_t> valid(n);
  const int r = cmtv::verify_templated_locked(ctx, n, nullptr, c->sigs, nullptr, B.tmpls.data(), 1, B.blob.data(),
                                              B.blob.size(), nullptr, B.tflag.data(), c->ts_seconds, c->ts_nanos, mode,
                                              valid.data(), ks, nullptr, bound, &check, &ok);
  if (r != CMTV_OK) {
    *rc = r;  // a library error (the batch's own)
    return true;
  }
  if (!ok) return false;
  J.first = 0;
  *rc = job_replay_batch(J, valid, seen);
  return true;
}

}  // namespace

// ------------------------------------------------------------------ BatchVerifier

struct cmtv_batch {
  cmtv_ctx* ctx;
  uint32_t mode;
  std::vector<uint8_t> pk, sig, msg;
  std::vector<uint32_t> off{0};
  std::vector<uint8_t> forced_invalid;  // bad sig length
  int64_t bad_key = -1;                 // first entry with a bad key length
};

template <class V>
static void grow_for(V& v, size_t extra) {
  if (v.capacity() - v.size() < extra) v.reserve(std::max(v.size() + extra, 2 * v.capacity()));
}

// No C++ exception crosses the C ABI (the vectors, maps and worker threads
// above can throw): a failed allocation is CMTV_ENOMEM, anything else
// CMTV_EINVAL; the context stays usable (its locks are scoped).
template <class F>
static int no_throw(F&& f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return CMTV_ENOMEM;
  } catch (...) {
    return CMTV_EINVAL;
  }
}

extern "C" {

int64_t cmtv_vote_sign_bytes(const char* chain_id, size_t chain_id_len, int32_t vote_type, int64_t height,
                             int32_t round, const cmtv_block_id* block_id, int64_t ts_seconds, int32_t ts_nanos,
                             uint8_t* out, size_t cap) {
  if ((!chain_id && chain_id_len) || (!out && cap)) return CMTV_EINVAL;
  std::string s;
  vote_sign_bytes(s, chain_id, chain_id_len, vote_type, height, round, block_id, ts_seconds, ts_nanos);
  if (s.size() <= cap) std::memcpy(out, s.data(), s.size());
  return (int64_t)s.size();
}

int cmtv_batch_new(cmtv_ctx* ctx, uint32_t mode, cmtv_batch** out) {
  if (!ctx || !out || mode > CMTV_MODE_ZIP215) return CMTV_EINVAL;
  auto* b = new (std::nothrow) cmtv_batch();
  if (!b) return CMTV_ENOMEM;
  b->ctx = ctx;
  b->mode = mode;
  *out = b;
  return CMTV_OK;
}

int cmtv_batch_add(cmtv_batch* b, const uint8_t* pk, size_t pk_len, const uint8_t* msg, size_t msg_len,
                   const uint8_t* sig, size_t sig_len) {
  if (!b || (!pk && pk_len) || (!msg && msg_len) || (!sig && sig_len)) return CMTV_EINVAL;
  if (b->msg.size() + msg_len > 0xFFFFFFFFull) return CMTV_EINVAL;
  const size_t idx = b->off.size() - 1;
  uint8_t kbuf[32] = {0}, sbuf[64] = {0};
  const bool key_ok = pk_len == 32, sig_ok = sig_len == 64;
  if (key_ok) std::memcpy(kbuf, pk, 32);
  if (sig_ok) std::memcpy(sbuf, sig, 64);
  // room first (geometric growth), so a failed allocation leaves the batch
  // as it was and no exception crosses the C ABI
  try {
    grow_for(b->pk, 32);
    grow_for(b->sig, 64);
    grow_for(b->msg, msg_len);
    grow_for(b->off, 1);
    grow_for(b->forced_invalid, 1);
  } catch (...) {
    return CMTV_ENOMEM;
  }
  if (!key_ok && b->bad_key < 0) b->bad_key = (int64_t)idx;
  b->pk.insert(b->pk.end(), kbuf, kbuf + 32);
  b->sig.insert(b->sig.end(), sbuf, sbuf + 64);
  if (msg_len) b->msg.insert(b->msg.end(), msg, msg + msg_len);
  b->off.push_back((uint32_t)b->msg.size());
  b->forced_invalid.push_back(!(key_ok && sig_ok));
  return CMTV_OK;
}

size_t cmtv_batch_len(const cmtv_batch* b) { return b ? b->off.size() - 1 : 0; }

void cmtv_batch_reset(cmtv_batch* b) {
  if (!b) return;
  b->pk.clear();
  b->sig.clear();
  b->msg.clear();
  b->off.assign(1, 0);
  b->forced_invalid.clear();
  b->bad_key = -1;
}

void cmtv_batch_free(cmtv_batch* b) { delete b; }

int cmtv_batch_verify(cmtv_batch* b, uint8_t* out_valid, int* all_ok, int64_t* bad_key_index) {
  if (!b || !all_ok) return CMTV_EINVAL;
  const size_t n = cmtv_batch_len(b);
  if (bad_key_index) *bad_key_index = b->bad_key;
  *all_ok = 0;  // an empty batch verifies nothing
  if (n == 0) return CMTV_OK;
  if (!out_valid) return CMTV_EINVAL;
  std::unique_lock<std::mutex> lk;
  int rc = cmtv::ctx_lock(b->ctx, lk);
  if (rc != CMTV_OK) return rc;
  rc = cmtv::verify_host_locked(b->ctx, n, b->pk.data(), b->sig.data(), b->msg.data(), b->off.data(), b->mode,
                                out_valid, nullptr);
  if (rc != CMTV_OK) return rc;
  int ok = 1;
  for (size_t i = 0; i < n; i++) {
    if (b->forced_invalid[i]) out_valid[i] = 0;
    ok &= out_valid[i] != 0;
  }
  *all_ok = ok;
  return CMTV_OK;
}

// ------------------------------------------------------------------ VerifyCommit*

static int cmtv_verify_commit_impl(cmtv_ctx* ctx, uint32_t kind, uint32_t mode, const char* chain_id, size_t chain_id_len,
                       const cmtv_valset* vals, const cmtv_block_id* block_id, int64_t height,
                       const cmtv_commit* commit, uint64_t trust_num, uint64_t trust_den, cmtv_commit_result* res,
                       char* msg_buf, size_t msg_cap) {
  if (!ctx || mode > CMTV_MODE_ZIP215) return CMTV_EINVAL;
  int rc = job_check_args(kind, chain_id, chain_id_len, vals, block_id, commit, res);
  if (rc != CMTV_OK) return rc;
  CommitJob J{kind, chain_id, chain_id_len, vals, block_id, height, commit, trust_num, trust_den, res, msg_buf,
              msg_cap};
  AddrIndex addr;
  if (kind == CMTV_VERIFY_COMMIT_LIGHT_TRUSTING) {
    addr.build(vals->addrs, vals->n_vals);
    J.addr = &addr;
  }
  thread_local Seen seen;
  cmtv::note_latency(ctx);  // a consensus-path call: pipelines leave it CUs
  const bool traced = cmtv::call_trace_on(ctx);
  const uint64_t t_entry = traced ? cmtv::call_trace_now() : 0;
  std::unique_lock<std::mutex> lk;
  rc = cmtv::ctx_lock(ctx, lk);
  if (rc != CMTV_OK) return rc;
  struct TraceGuard {  // CMTV_CALL_TRACE: recorded before the lock is released
    cmtv_ctx* c;
    uint64_t t_entry, t_locked;
    ~TraceGuard() {
      if (t_locked) cmtv::call_trace_record_locked(c, t_entry, t_locked);
    }
  } trace_guard{ctx, t_entry, traced ? cmtv::call_trace_now() : 0};
  if (traced) cmtv::call_trace_begin_locked(ctx);
  // beside a pipeline call: the CUs its chunks leave free (released before
  // the lock)
  cmtv::LatencyStreams lat_streams(ctx);
  // the early-staged signatures below belong to this call only: forgotten on
  // every exit (a preamble error or an empty plan runs no batch), before the
  // lock is released
  struct EarlyGuard {
    cmtv_ctx* c;
    ~EarlyGuard() { cmtv::clear_early_locked(c); }
  } early_guard{ctx};
  const uint64_t t0 = cmtv::phase_now(ctx);
  SigBatch B;
  const bool cache = cmtv::cache_enabled(ctx);
  B.templated = !cache && templated_enabled();
  // signatures back to back (and, without registered keys, 32-byte keys in
  // validator order): their copy to the device can start now and overlap the
  // plan (used only if the fast form takes exactly these bytes)
  if (B.templated && kind != CMTV_VERIFY_COMMIT_LIGHT_TRUSTING && commit->n_sigs && commit->sig_off[0] == 0 &&
      commit->sig_off[commit->n_sigs] == 64ull * commit->n_sigs) {
    const bool keyed = cmtv::keyset_cache_enabled(ctx);
    const bool packed = vals->n_vals == commit->n_sigs && vals->pk_off[0] == 0 &&
                        vals->pk_off[vals->n_vals] == 32ull * vals->n_vals;
    if (keyed || packed) {
      rc = cmtv::stage_sigs_early_locked(ctx, commit->sigs, commit->n_sigs, keyed ? nullptr : vals->pubkeys);
      if (rc != CMTV_OK) return rc;
    }
  }
  if (B.templated && cmtv::keyset_cache_enabled(ctx) && verify_commit_spec(ctx, J, mode, seen, &rc)) {
    cmtv::phase_add(ctx, cmtv::kPhPrepare, t0);
    return rc;
  }
  job_prepare(J, B, cache, true, seen);
  cmtv::phase_add(ctx, cmtv::kPhPrepare, t0);
  std::vector<uint8_t> valid;
  rc = batch_verify(ctx, B, mode, valid);
  if (rc != CMTV_OK) return rc;
  const uint64_t t1 = cmtv::phase_now(ctx);
  rc = job_replay_batch(J, valid, seen);
  cmtv::phase_add(ctx, cmtv::kPhReplay, t1);
  return rc;
}

static int cmtv_verify_commits_impl(cmtv_ctx* ctx, uint32_t kind, uint32_t mode, const char* chain_id, size_t chain_id_len,
                        size_t n, const cmtv_valset* vals, const cmtv_block_id* block_ids, const int64_t* heights,
                        const cmtv_commit* commits, uint64_t trust_num, uint64_t trust_den,
                        cmtv_commit_result* results, int* rcs, char* msg_bufs, size_t msg_cap) {
  if (!ctx || mode > CMTV_MODE_ZIP215 || n > (1u << 24)) return CMTV_EINVAL;
  if (n == 0) return CMTV_OK;
  if (!vals || !commits || !results || !rcs || !heights ||
      (kind != CMTV_VERIFY_COMMIT_LIGHT_TRUSTING && !block_ids))
    return CMTV_EINVAL;
  uint64_t n_sigs = 0;
  for (size_t c = 0; c < n; c++) {
    const int rc = job_check_args(kind, chain_id, chain_id_len, &vals[c], block_ids ? &block_ids[c] : nullptr,
                                  &commits[c], &results[c]);
    if (rc != CMTV_OK) return rc;
    n_sigs += commits[c].n_sigs;
  }
  const CommitsArgs args{kind, mode, chain_id, chain_id_len, n, vals, block_ids, heights, commits, trust_num,
                         trust_den, results, msg_bufs, msg_cap};
  // large calls: the chunked pipeline (plan / pack / replay on the host
  // workers, per-device lanes; the context lock only around submissions)
  if (cmtv::pipeline_wanted(ctx, n_sigs)) return cmtv::verify_commits_pipeline(ctx, args, rcs);
  if (n_sigs <= 4096) cmtv::note_latency(ctx);  // a small call waits on its verdicts
  std::vector<CommitJob> jobs;
  jobs.reserve(n);
  for (size_t c = 0; c < n; c++) jobs.push_back(args.job(c));
  // LightTrusting: one address index per distinct (address array, size)
  std::map<std::pair<const uint8_t*, uint32_t>, AddrIndex> addr;
  if (kind == CMTV_VERIFY_COMMIT_LIGHT_TRUSTING)
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
  std::unique_lock<std::mutex> lk;
  int rc = cmtv::ctx_lock(ctx, lk);
  if (rc != CMTV_OK) return rc;
  // a small call beside a pipeline call: the CUs its chunks leave free
  std::optional<cmtv::LatencyStreams> lat_streams;
  if (n_sigs <= 4096) lat_streams.emplace(ctx);
  const uint64_t t0 = cmtv::phase_now(ctx);
  SigBatch B;
  const bool prefetch = cmtv::cache_enabled(ctx);
  B.templated = !prefetch && templated_enabled();
  for (auto& J : jobs) job_prepare(J, B, prefetch, n == 1, seen);
  cmtv::phase_add(ctx, cmtv::kPhPrepare, t0);
  std::vector<uint8_t> valid;
  rc = batch_verify(ctx, B, mode, valid);
  if (rc != CMTV_OK) return rc;
  const uint64_t t1 = cmtv::phase_now(ctx);
  for (size_t c = 0; c < n; c++) rcs[c] = job_replay_batch(jobs[c], valid, seen);
  cmtv::phase_add(ctx, cmtv::kPhReplay, t1);
  return CMTV_OK;
}

int cmtv_verify_commit(cmtv_ctx* ctx, uint32_t kind, uint32_t mode, const char* chain_id, size_t chain_id_len,
                       const cmtv_valset* vals, const cmtv_block_id* block_id, int64_t height,
                       const cmtv_commit* commit, uint64_t trust_num, uint64_t trust_den, cmtv_commit_result* res,
                       char* msg_buf, size_t msg_cap) {
  return no_throw([&] {
    return cmtv_verify_commit_impl(ctx, kind, mode, chain_id, chain_id_len, vals, block_id, height, commit, trust_num,
                                   trust_den, res, msg_buf, msg_cap);
  });
}

int cmtv_verify_commits(cmtv_ctx* ctx, uint32_t kind, uint32_t mode, const char* chain_id, size_t chain_id_len,
                        size_t n, const cmtv_valset* vals, const cmtv_block_id* block_ids, const int64_t* heights,
                        const cmtv_commit* commits, uint64_t trust_num, uint64_t trust_den,
                        cmtv_commit_result* results, int* rcs, char* msg_bufs, size_t msg_cap) {
  return no_throw([&] {
    return cmtv_verify_commits_impl(ctx, kind, mode, chain_id, chain_id_len, n, vals, block_ids, heights, commits,
                                    trust_num, trust_den, results, rcs, msg_bufs, msg_cap);
  });
}

}  // extern "C"
