// case_reader.h -- the little-endian case files the Python tests write for the
// stand-alone host checkers (typedcheck.cpp, typedcommitscheck.cpp), read
// field by field; a truncated file ends the program with status 2.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct Reader {
  std::vector<uint8_t> d;
  size_t at = 0;
  bool load(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) d.insert(d.end(), buf, buf + n);
    std::fclose(f);
    return true;
  }
  void need(size_t n) {
    if (at + n > d.size()) {
      std::fprintf(stderr, "truncated input\n");
      std::exit(2);
    }
  }
  template <class T>
  T get() {
    T v;
    need(sizeof(T));
    std::memcpy(&v, &d[at], sizeof(T));
    at += sizeof(T);
    return v;
  }
  std::vector<uint8_t> bytes(size_t n) {
    need(n);
    std::vector<uint8_t> v(d.begin() + (long)at, d.begin() + (long)(at + n));
    at += n;
    return v;
  }
};
