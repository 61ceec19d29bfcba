// typedcommitscheck.cpp -- the cross-height typed commit layer
// (cmtv_verify_commits_typed in cometbft_amd/csrc/commit_typed.cpp, with
// commit.cpp and pipeline.cpp) on the CPU, linked against fake_runtime.cpp
// and fake_typed_runtime.cpp, under AddressSanitizer + UBSan: the grouping of
// commits by registered set, the per-group templates, the partition by key
// type across commits, the scatter and the per-commit replay; every
// secp256k1 batch a bulk one, no Ed25519 batch without message offsets.
//
//   typedcommitscheck FILE
// FILE holds cases written by tests/test_typed_commits_host.py (little-endian):
//   u32 n_cases, then per case
//     u32 kind, u32 keyset_cap, u64 trust_num, u64 trust_den, u32 chain_len, chain,
//     u32 types_mode (0: one type array per commit; 1: the array of arrays is NULL; 2: as 0, plus
//         every all-Ed25519 commit gets explicit zeros instead of NULL), u32 n_commits,
//     i32 want_bulk_calls, i32 want_bulk_keyed (-1: not compared)
//     per commit:
//       i64 height
//       u32 n_vals, per validator: u8 type, u32 key_len, key, i64 power, u8 addr[20]
//       commit: i64 height, i32 round, u8 hash[32], u32 psh_total, u8 psh_hash[32],
//               u32 n_sigs, per signature: u8 flag, u8 addr[20], i64 sec, i32 nanos, u32 sig_len, sig
//       expected: i32 rc, i32 code, i32 sig_index (-2: not compared), u32 msg_len, msg, u32 n_verified
// Every commit's outcome is compared with the expectation and, field by
// field, with cmtv_verify_commit_typed's for that commit alone on a context
// of its own. Prints one line per case and "typedcommitscheck ok (N cases)";
// exit status 1 on a mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/cmtverify.h"
#include "case_reader.h"

extern "C" {
cmtv_ctx* fake_open(size_t n_devs, unsigned threads, size_t pipe_min, size_t chunk, int slots, bool pipe_on,
                    size_t keyset_cap, long fail_dev);
void fake_close(cmtv_ctx* c);
void fake_counts(cmtv_ctx* c, uint64_t* out);
void fake_typed_counts(uint64_t* out);  // [3..7): bulk calls, those by registered keys, signatures, templates shipped
}

namespace {

// One commit's arguments in exact-size arrays, so that AddressSanitizer sees
// any read past them
struct Height {
  int64_t height;
  std::vector<uint8_t> types, keys, addrs, hash, psh, flags, vaddrs, sigs;
  std::vector<uint32_t> pk_off, sig_off;
  std::vector<int64_t> power, prio, sec;
  std::vector<int32_t> nanos;
  bool all_ed = true;
  cmtv_commit cm{};
  cmtv_valset vs{};
  int32_t want_rc, want_code, want_idx;
  std::string want_msg;
  uint32_t want_nv;
};

std::unique_ptr<Height> read_height(Reader& r) {
  static const uint8_t none = 0;
  std::unique_ptr<Height> hp(new Height());
  Height& h = *hp;
  h.height = r.get<int64_t>();
  const uint32_t nv = r.get<uint32_t>();
  h.types.resize(nv);
  h.pk_off.assign(nv + 1, 0);
  h.power.resize(nv);
  h.prio.assign(nv, 0);
  for (uint32_t i = 0; i < nv; i++) {
    h.types[i] = r.get<uint8_t>();
    h.all_ed = h.all_ed && h.types[i] == 0;
    const auto k = r.bytes(r.get<uint32_t>());
    h.keys.insert(h.keys.end(), k.begin(), k.end());
    h.pk_off[i + 1] = (uint32_t)h.keys.size();
    h.power[i] = r.get<int64_t>();
    const auto a = r.bytes(20);
    h.addrs.insert(h.addrs.end(), a.begin(), a.end());
  }
  h.cm.height = r.get<int64_t>();
  h.cm.round = r.get<int32_t>();
  h.hash = r.bytes(32);
  const uint32_t total = r.get<uint32_t>();
  h.psh = r.bytes(32);
  h.cm.block_id = cmtv_block_id{h.hash.data(), 32, total, h.psh.data(), 32};
  const uint32_t ns = r.get<uint32_t>();
  h.flags.resize(ns);
  h.sec.resize(ns);
  h.nanos.resize(ns);
  h.sig_off.assign(ns + 1, 0);
  for (uint32_t i = 0; i < ns; i++) {
    h.flags[i] = r.get<uint8_t>();
    const auto a = r.bytes(20);
    h.vaddrs.insert(h.vaddrs.end(), a.begin(), a.end());
    h.sec[i] = r.get<int64_t>();
    h.nanos[i] = r.get<int32_t>();
    const auto s = r.bytes(r.get<uint32_t>());
    h.sigs.insert(h.sigs.end(), s.begin(), s.end());
    h.sig_off[i + 1] = (uint32_t)h.sigs.size();
  }
  h.cm.n_sigs = ns;
  h.cm.flags = h.flags.data();
  h.cm.ts_seconds = h.sec.data();
  h.cm.ts_nanos = h.nanos.data();
  h.cm.sigs = h.sigs.empty() ? &none : h.sigs.data();
  h.cm.sig_off = h.sig_off.data();
  h.cm.val_addrs = h.vaddrs.data();
  h.vs = cmtv_valset{nv, h.keys.data(), h.pk_off.data(), h.power.data(), h.addrs.data(), h.prio.data()};
  h.want_rc = r.get<int32_t>();
  h.want_code = r.get<int32_t>();
  h.want_idx = r.get<int32_t>();
  const auto wm = r.bytes(r.get<uint32_t>());
  h.want_msg.assign(wm.begin(), wm.end());
  h.want_nv = r.get<uint32_t>();
  return hp;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  Reader r;
  if (!r.load(argv[1])) return 2;
  const uint32_t n_cases = r.get<uint32_t>();
  constexpr size_t kCap = 2048;
  int bad = 0;
  for (uint32_t c = 0; c < n_cases; c++) {
    const uint32_t kind = r.get<uint32_t>(), cap = r.get<uint32_t>();
    const uint64_t num = r.get<uint64_t>(), den = r.get<uint64_t>();
    const auto chain = r.bytes(r.get<uint32_t>());
    const char* cid = reinterpret_cast<const char*>(chain.data());
    const uint32_t types_mode = r.get<uint32_t>(), n = r.get<uint32_t>();
    const int32_t want_bulk = r.get<int32_t>(), want_keyed = r.get<int32_t>();
    std::vector<std::unique_ptr<Height>> hs;
    for (uint32_t i = 0; i < n; i++) hs.push_back(read_height(r));
    std::vector<cmtv_valset> vals(n);
    std::vector<cmtv_commit> commits(n);
    std::vector<cmtv_block_id> bids(n);
    std::vector<int64_t> heights(n);
    std::vector<const uint8_t*> types(n);
    for (uint32_t i = 0; i < n; i++) {
      vals[i] = hs[i]->vs;
      commits[i] = hs[i]->cm;
      bids[i] = hs[i]->cm.block_id;
      heights[i] = hs[i]->height;
      types[i] = hs[i]->all_ed && types_mode != 2 ? nullptr : hs[i]->types.data();
    }
    std::vector<cmtv_commit_result> res(n);
    std::vector<int> rcs(n, 12345);
    std::vector<char> msgs(n * kCap, 'x');

    cmtv_ctx* ctx = fake_open(1, 1, (size_t)1 << 40, 1u << 20, 3, false, cap, -1);
    uint64_t c0[7], c1[7], cnt[9];
    fake_typed_counts(c0);
    const int rc = cmtv_verify_commits_typed(ctx, kind, CMTV_MODE_GO_STDLIB, cid, chain.size(), n, vals.data(),
                                             types_mode == 1 ? nullptr : types.data(), bids.data(), heights.data(),
                                             commits.data(), num, den, res.data(), rcs.data(), msgs.data(), kCap);
    fake_typed_counts(c1);
    fake_counts(ctx, cnt);
    fake_close(ctx);
    bool ok = rc == CMTV_OK;
    const int bulk = (int)(c1[3] - c0[3]), keyed = (int)(c1[4] - c0[4]);
    ok = ok && (want_bulk < 0 || bulk == want_bulk) && (want_keyed < 0 || keyed == want_keyed);
    // every secp256k1 batch is a bulk one, and no templated batch comes without offsets
    ok = ok && c1[0] - c0[0] == c1[3] - c0[3] && cnt[8] == 0;
    // a group ships its own commits' templates only
    ok = ok && c1[6] - c0[6] <= (uint64_t)n;
    std::printf("case %u: rc %d, %u commits, %d bulk calls (%d keyed)%s\n", c, rc, n, bulk, keyed, ok ? "" : " MISMATCH");
    for (uint32_t i = 0; i < n && rc == CMTV_OK; i++) {
      const Height& h = *hs[i];
      const char* msg = &msgs[i * kCap];
      bool good = rcs[i] == h.want_rc && res[i].code == h.want_code &&
                  (h.want_idx == -2 || res[i].sig_index == h.want_idx) && h.want_msg == msg &&
                  res[i].n_verified == h.want_nv;
      // the same commit alone
      cmtv_ctx* one = fake_open(1, 1, (size_t)1 << 40, 1u << 20, 3, false, cap, -1);
      cmtv_commit_result r1{};
      char m1[kCap];
      const int rc1 = cmtv_verify_commit_typed(one, kind, CMTV_MODE_GO_STDLIB, cid, chain.size(), &vals[i],
                                               types_mode == 1 ? nullptr : types[i], &bids[i], heights[i], &commits[i],
                                               num, den, &r1, m1, sizeof m1);
      fake_close(one);
      good = good && rc1 == rcs[i] && r1.code == res[i].code && r1.sig_index == res[i].sig_index &&
             r1.got == res[i].got && r1.needed == res[i].needed && r1.n_verified == res[i].n_verified &&
             std::strcmp(m1, msg) == 0;
      if (!good) {
        std::printf("  commit %u: rc %d code %d index %d verified %u got %lld needed %lld \"%s\"\n"
                    "    want   rc %d code %d index %d verified %u \"%s\"\n"
                    "    alone  rc %d code %d index %d verified %u got %lld needed %lld \"%s\"\n",
                    i, rcs[i], res[i].code, res[i].sig_index, res[i].n_verified, (long long)res[i].got,
                    (long long)res[i].needed, msg, h.want_rc, h.want_code, h.want_idx, h.want_nv, h.want_msg.c_str(), rc1,
                    r1.code, r1.sig_index, r1.n_verified, (long long)r1.got, (long long)r1.needed, m1);
        ok = false;
      }
    }
    if (!ok) bad++;
  }
  // argument errors: the single call's, for the whole call
  {
    cmtv_ctx* ctx = fake_open(1, 1, (size_t)1 << 40, 1u << 20, 3, false, 0, -1);
    cmtv_commit_result res{};
    int rcs = 0;
    if (cmtv_verify_commits_typed(ctx, 0, CMTV_MODE_GO_STDLIB, "c", 1, 1, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                  0, &res, &rcs, nullptr, 0) != CMTV_EINVAL ||
        cmtv_verify_commits_typed(ctx, 0, CMTV_MODE_GO_STDLIB, "c", 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                  0, nullptr, nullptr, nullptr, 0) != CMTV_OK) {
      std::printf("argument checks MISMATCH\n");
      bad++;
    }
    // a type above CMTV_KEY_SR25519, and a 65-byte secp256k1 key, in the second of two commits
    const uint8_t key[65] = {4}, addr[20] = {0}, hash[32] = {1}, flag[1] = {2}, sig[64] = {0};
    const uint32_t off33[2] = {0, 33}, off65[2] = {0, 65}, sig_off[2] = {0, 64};
    const int64_t power[1] = {1}, prio[1] = {0}, sec[1] = {0}, hts[2] = {1, 1};
    const int32_t nanos[1] = {0};
    cmtv_commit cm{};
    cm.height = 1;
    cm.block_id = cmtv_block_id{hash, 32, 1, hash, 32};
    cm.n_sigs = 1;
    cm.flags = flag;
    cm.ts_seconds = sec;
    cm.ts_nanos = nanos;
    cm.sigs = sig;
    cm.sig_off = sig_off;
    cm.val_addrs = addr;
    const cmtv_commit cms[2] = {cm, cm};
    const cmtv_block_id bids[2] = {cm.block_id, cm.block_id};
    const cmtv_valset v33{1, key, off33, power, addr, prio}, v65{1, key, off65, power, addr, prio};
    const uint8_t t1[1] = {CMTV_KEY_SECP256K1}, t3[1] = {3};
    cmtv_commit_result rs[2];
    int rc2[2];
    const cmtv_valset bad_type[2] = {v33, v33}, bad_key[2] = {v33, v65};
    const uint8_t* const types_a[2] = {t1, t3};
    const uint8_t* const types_b[2] = {nullptr, t1};
    if (cmtv_verify_commits_typed(ctx, 0, CMTV_MODE_GO_STDLIB, "c", 1, 2, bad_type, types_a, bids, hts, cms, 0, 0, rs,
                                  rc2, nullptr, 0) != CMTV_EINVAL ||
        cmtv_verify_commits_typed(ctx, 0, CMTV_MODE_GO_STDLIB, "c", 1, 2, bad_key, types_b, bids, hts, cms, 0, 0, rs,
                                  rc2, nullptr, 0) != CMTV_EINVAL) {
      std::printf("key type checks MISMATCH\n");
      bad++;
    }
    fake_close(ctx);
  }
  if (bad) return 1;
  std::printf("typedcommitscheck ok (%u cases)\n", n_cases);
  return 0;
}
