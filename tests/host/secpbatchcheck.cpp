// Host-side build of the batched registered-key secp256k1 device code
// (cometbft_amd/csrc/secp256k1.h secp_verify_keyed_batch_lane, the function
// k_verify_secp256k1_keyed_batch<KB> calls) with operand-bound assertions on.
// Test infrastructure only: checks the kernel source without a GPU.
//
//   secpbatchcheck KB LANES        KB = 4 or 8
// Input (stdin):
//   u32 n_keys, then n_keys x u8 pk[33]: the keys, registered in this order
//   (tables built with secp_qcomb_position, as secpkeyedcheck.cpp does)
//   u32 n, then n x { u32 key_idx, u8 sig[64], u32 mlen, u8 msg[mlen] }
//   (a key_idx >= n_keys is allowed: the verdict is 0 and key 0's table is read)
// The n signatures are laid out as the kernel lays them out over LANES lanes
// per launch of LANES x KB signatures: signature s = base + lane + r * LANES
// in round r of its lane; a round past n is inactive and takes signature
// n - 1, whose verdict it must not write.
// Output: n verdict bytes of the batched function, then n verdict bytes of
// secp_verify_keyed_one over the same inputs. Exit status 4 if an inactive
// round wrote a verdict or an active one wrote none or two.
#define CMTV_HD inline
#define CMTV_BOUNDS_CHECK 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../cometbft_amd/csrc/secp256k1.h"

using namespace cmtv;

constexpr size_t kTabWords = (size_t)SECP_GTAB_ENTRIES * SECP_GTAB_ROW_WORDS;

// rows of one table in the kernels' layout
struct HostTab {
  const uint32_t* rows;
  void load(int row, pt256& p) const {
    const uint32_t* q = rows + (size_t)row * SECP_GTAB_ROW_WORDS;
    for (int i = 0; i < 10; i++) {
      p.X.v[i] = q[i];
      p.Y.v[i] = q[10 + i];
      p.Z.v[i] = q[20 + i];
    }
  }
};

struct Entry {
  uint32_t key;
  uint8_t sig[64];
  std::vector<uint32_t> buf;  // the message at an odd offset inside a word-aligned buffer
  const uint8_t* msg;
  uint32_t mlen;
};

// the lane's running products: exactly KB slots, so a sanitizer sees any other
template <int KB>
struct HostPre {
  std::vector<scn> slot = std::vector<scn>(KB);
  void store(int r, const scn& x) { slot.at((size_t)r) = x; }
  void load(int r, scn& x) const { x = slot.at((size_t)r); }
};

struct HostSrc {
  using QTab = HostTab;
  const std::vector<Entry>& in;
  const std::vector<uint32_t>& tab;
  const std::vector<uint8_t>& ok;
  size_t base, lanes, lane, n_keys;
  std::vector<uint8_t>& out;
  std::vector<uint8_t>& writes;
  size_t at(int r) const { return base + lane + (size_t)r * lanes; }
  bool active(int r) const { return at(r) < in.size(); }
  size_t index(int r) const { return active(r) ? at(r) : in.size() - 1; }
  const uint8_t* sig(int r) const { return in[index(r)].sig; }
  bool key(int r, QTab& qt) const {
    const uint32_t k = in[index(r)].key;
    const bool in_set = k < n_keys;
    const size_t key = in_set ? k : 0;
    qt.rows = &tab[key * kTabWords];
    return in_set && ok[key] != 0;
  }
  uint32_t message(int r, const uint8_t*& msg) const {
    msg = in[index(r)].msg;
    return in[index(r)].mlen;
  }
  void verdict(int r, bool v) const {
    if (!active(r)) {
      if (v) std::exit(4);  // an inactive round's verdict is false and goes nowhere
      return;
    }
    out[at(r)] = v ? 1 : 0;
    writes[at(r)]++;
  }
};

static bool rd(void* p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }

template <int KB>
static void run(const std::vector<Entry>& in, const std::vector<uint32_t>& tab, const std::vector<uint8_t>& ok,
                size_t lanes, size_t n_keys, const HostTab& gt, std::vector<uint8_t>& out,
                std::vector<uint8_t>& writes) {
  for (size_t base = 0; base < in.size(); base += lanes * KB)
    for (size_t lane = 0; lane < lanes; lane++) {  // a lane with no active round included, as in the last wave
      HostSrc src{in, tab, ok, base, lanes, lane, n_keys, out, writes};
      HostPre<KB> pre;
      secp_verify_keyed_batch_lane<KB>(src, pre, gt);
    }
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const int kb = std::atoi(argv[1]);
  const size_t lanes = (size_t)std::atol(argv[2]);
  if ((kb != 4 && kb != 8) || lanes == 0) return 2;
  uint32_t n_keys;
  if (!rd(&n_keys, 4) || n_keys == 0 || n_keys > 4096) return 1;
  std::vector<uint8_t> pk(33 * (size_t)n_keys), ok(n_keys);
  if (!rd(pk.data(), pk.size())) return 1;
  std::vector<uint32_t> tab(n_keys * kTabWords, 0xFFFFFFFFu);
  for (uint32_t k = 0; k < n_keys; k++)
    for (int j = 0; j < SECP_GTAB_POS; j++) {
      uint32_t* rows = &tab[k * kTabWords + (size_t)j * SECP_GTAB_PER_POS * SECP_GTAB_ROW_WORDS];
      const bool v = secp_qcomb_position(rows, &pk[33 * (size_t)k], j);
      if (j == 0) ok[k] = v ? 1 : 0;
    }
  std::vector<uint32_t> gtab(kTabWords);
  for (int j = 0; j < SECP_GTAB_POS; j++)
    for (int d = 1; d <= SECP_GTAB_PER_POS; d++)
      secp_gtab_row(&gtab[(size_t)(j * SECP_GTAB_PER_POS + d - 1) * SECP_GTAB_ROW_WORDS], j, d);
  const HostTab gt{gtab.data()};
  uint32_t n;
  if (!rd(&n, 4) || n == 0) return 1;
  std::vector<Entry> in(n);
  for (uint32_t i = 0; i < n; i++) {
    Entry& e = in[i];
    if (!rd(&e.key, 4) || !rd(e.sig, 64) || !rd(&e.mlen, 4)) return 1;
    e.buf.assign((e.mlen + 16) / 4 + 2, 0);
    uint8_t* m = reinterpret_cast<uint8_t*>(e.buf.data()) + 1 + (i % 3);
    if (!rd(m, e.mlen)) return 1;
    e.msg = m;
  }
  std::vector<uint8_t> out(n, 0xEE), writes(n, 0), one(n);
  if (kb == 8)
    run<8>(in, tab, ok, lanes, n_keys, gt, out, writes);
  else
    run<4>(in, tab, ok, lanes, n_keys, gt, out, writes);
  for (uint32_t i = 0; i < n; i++)
    if (writes[i] != 1) return 4;
  for (uint32_t i = 0; i < n; i++) {
    const Entry& e = in[i];
    const bool in_set = e.key < n_keys;
    const HostTab qt{&tab[(in_set ? e.key : 0) * kTabWords]};
    one[i] = secp_verify_keyed_one(in_set && ok[in_set ? e.key : 0] != 0, e.sig, e.msg, e.mlen, qt, gt) ? 1 : 0;
  }
  fwrite(out.data(), 1, n, stdout);
  fwrite(one.data(), 1, n, stdout);
  return 0;
}
