// Host-side build of the secp256k1 templated per-lane functions
// (cometbft_amd/csrc/secp256k1.h secp_verify_tmpl_one and
// secp_verify_keyed_tmpl_one: the lane writes its CanonicalVote from the
// commit's template into its slot, then verifies over it), with the headers'
// operand-bound assertions on. Test infrastructure only: checks the kernel
// source without a GPU.
//
//   input  (stdin):  u32 n, then n x { u8 pk[33], u8 sig[64], u32 pre_commit_len,
//                    u32 pre_nil_len, u32 post_len, u8 blob[sum of the three],
//                    u8 commit_flag, i64 sec, i32 nanos }
//   output (stdout): per record u8 verdict (by key bytes), u8 verdict (by the
//                    key's comb table), u32 message length, u8 message[length]
// The slot is kSbFuseMaxMsg bytes as the kernels' (a longer message exits 4),
// filled with a different junk byte per record so a hash that read past the
// bytes the writer wrote would not repeat.
#define CMTV_HD inline
#define CMTV_BOUNDS_CHECK 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "../../cometbft_amd/csrc/secp256k1.h"

using namespace cmtv;

constexpr uint32_t kSlotBytes = 192;  // kernels.h kSbFuseMaxMsg

struct HostQTab {
  pt256 t[SECP_QTAB_ENTRIES];
  void store(int e, const pt256& p) { t[e] = p; }
  void load(int e, pt256& p) const { p = t[e]; }
};

struct RowTab {
  std::vector<uint32_t> rows;
  void load(int row, pt256& p) const {
    const uint32_t* q = &rows[(size_t)row * SECP_GTAB_ROW_WORDS];
    for (int i = 0; i < 10; i++) {
      p.X.v[i] = q[i];
      p.Y.v[i] = q[10 + i];
      p.Z.v[i] = q[20 + i];
    }
  }
};

struct SlotBytes {
  uint8_t* p;
  uint32_t hi = 0;
  void put(uint32_t pos, uint8_t b) {
    if (pos >= kSlotBytes) exit(4);
    p[pos] = b;
    if (pos + 1 > hi) hi = pos + 1;
  }
  void copy(uint32_t pos, const uint8_t* s, uint32_t len) {
    for (uint32_t i = 0; i < len; i++) put(pos + i, s[i]);
  }
};

static bool rd(void* p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }

int main() {
  RowTab gt;
  gt.rows.resize((size_t)SECP_GTAB_ENTRIES * SECP_GTAB_ROW_WORDS);
  for (int j = 0; j < SECP_GTAB_POS; j++)
    for (int d = 1; d <= SECP_GTAB_PER_POS; d++)
      secp_gtab_row(&gt.rows[(size_t)(j * SECP_GTAB_PER_POS + d - 1) * SECP_GTAB_ROW_WORDS], j, d);
  std::map<std::string, std::pair<RowTab, bool>> combs;  // per key, built once
  uint32_t n;
  if (!rd(&n, 4)) return 1;
  for (uint32_t i = 0; i < n; i++) {
    uint8_t pk[33], sig[64], flag;
    uint32_t lens[3];
    int64_t sec;
    int32_t nanos;
    if (!rd(pk, 33) || !rd(sig, 64) || !rd(lens, 12)) return 1;
    std::vector<uint8_t> blob(lens[0] + lens[1] + lens[2] + 4);
    if (!rd(blob.data(), lens[0] + lens[1] + lens[2]) || !rd(&flag, 1) || !rd(&sec, 8) || !rd(&nanos, 4)) return 1;
    const SbTemplate t{0, lens[0], lens[0], lens[1], lens[0] + lens[1], lens[2]};
    uint8_t out[2];
    uint32_t slot[kSlotBytes / 4], mlen = 0;
    uint8_t msg[kSlotBytes];
    for (int pass = 0; pass < 2; pass++) {
      memset(slot, 0x5A + (int)(i % 97) + pass, sizeof slot);
      SlotBytes w{reinterpret_cast<uint8_t*>(slot)};
      if (pass == 0) {
        HostQTab qt;
        out[0] = secp_verify_tmpl_one(pk, sig, w, w.p, t, blob.data(), flag != 0, sec, nanos, qt, gt) ? 1 : 0;
        mlen = w.hi;
        memcpy(msg, slot, mlen);
      } else {
        const std::string key(reinterpret_cast<const char*>(pk), 33);
        auto it = combs.find(key);
        if (it == combs.end()) {
          RowTab qc;
          qc.rows.resize((size_t)SECP_GTAB_ENTRIES * SECP_GTAB_ROW_WORDS);
          bool ok = true;
          for (int j = 0; j < SECP_GTAB_POS; j++)
            ok = secp_qcomb_position(&qc.rows[(size_t)j * SECP_GTAB_PER_POS * SECP_GTAB_ROW_WORDS], pk, j);
          it = combs.emplace(key, std::make_pair(std::move(qc), ok)).first;
        }
        out[1] = secp_verify_keyed_tmpl_one(it->second.second, sig, w, w.p, t, blob.data(), flag != 0, sec, nanos,
                                            it->second.first, gt)
                     ? 1
                     : 0;
        if (w.hi != mlen || memcmp(msg, slot, mlen) != 0) return 5;
      }
    }
    fwrite(out, 1, 2, stdout);
    fwrite(&mlen, 4, 1, stdout);
    fwrite(msg, 1, mlen, stdout);
  }
  return 0;
}
