// Host build of cometbft_amd/csrc/verdict_bits.h: reads records of
// (n u64, words x u64 bitmap as a kernel may leave it) on stdin; writes per
// record (invalid u64, words x u64 masked bitmap as bitmap_tail copies it
// out, n verdict bytes padded to 8, words x u64 bitmap_pack of those bytes).
// Test infrastructure only (tests/test_verdict_bits.py holds the reference).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../cometbft_amd/csrc/verdict_bits.h"

int main() {
  uint64_t n;
  while (fread(&n, 8, 1, stdin) == 1) {
    const size_t words = cmtv::bitmap_words(n);
    std::vector<uint64_t> bm(words), out_bm(words, ~0ull), packed(words, ~0ull);
    if (fread(bm.data(), 8, words, stdin) != words) return 1;
    std::vector<uint8_t> valid((n + 7) / 8 * 8, 0);
    const uint64_t invalid = cmtv::bitmap_tail(bm.data(), n, out_bm.data(), valid.data());
    cmtv::bitmap_pack(valid.data(), n, packed.data());
    fwrite(&invalid, 8, 1, stdout);
    fwrite(out_bm.data(), 8, words, stdout);
    fwrite(valid.data(), 1, valid.size(), stdout);
    fwrite(packed.data(), 8, words, stdout);
  }
  return 0;
}
