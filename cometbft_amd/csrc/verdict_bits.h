// verdict_bits.h -- the host side of a verdict bitmap (bit i of word i / 64 =
// signature i valid): the tail every host-buffer call runs on the words its
// kernels wrote, and the reverse pack of the verdict cache's bytes
// (host_batch.cpp). Plain C++, shared with the host test
// (tests/host/bitscheck.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <cstring>

namespace cmtv {

inline size_t bitmap_words(size_t n) { return (n + 63) / 64; }

// Clears the bits at and past n of bm's last word (not every kernel writes
// them) and returns how many of the n verdicts are invalid.
inline uint64_t bitmap_mask_count(uint64_t* bm, size_t n) {
  const size_t words = bitmap_words(n);
  if (n & 63) bm[words - 1] &= (1ull << (n & 63)) - 1;
  uint64_t valid = 0;
  for (size_t w = 0; w < words; w++) valid += (uint64_t)__builtin_popcountll(bm[w]);
  return n - valid;
}

// One verdict byte (0 / 1) per signature.
inline void bitmap_expand(const uint64_t* bm, size_t n, uint8_t* out_valid) {
  for (size_t i = 0; i < n; i++) out_valid[i] = (uint8_t)((bm[i >> 6] >> (i & 63)) & 1);
}

// ... and back: the words of n verdict bytes, the last one's bits past n zero.
inline void bitmap_pack(const uint8_t* valid, size_t n, uint64_t* out_bitmap) {
  for (size_t w = 0; w < bitmap_words(n); w++) {
    uint64_t x = 0;
    for (size_t b = 0; b < 64 && 64 * w + b < n; b++) x |= (uint64_t)(valid[64 * w + b] & 1) << b;
    out_bitmap[w] = x;
  }
}

// The tail of a host-buffer call: masks bm, copies it to out_bitmap and
// expands it to out_valid (either may be null); returns the invalid count
// (cmtv_stats.invalid).
inline uint64_t bitmap_tail(uint64_t* bm, size_t n, uint64_t* out_bitmap, uint8_t* out_valid) {
  const uint64_t invalid = bitmap_mask_count(bm, n);
  if (out_bitmap) std::memcpy(out_bitmap, bm, 8 * bitmap_words(n));
  if (out_valid) bitmap_expand(bm, n, out_valid);
  return invalid;
}

}  // namespace cmtv
