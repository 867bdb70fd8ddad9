// TEST INFRASTRUCTURE -- what the stand-alone programs (*_main.cpp) share: the reader of the length-prefixed blob that
// tests/hostsim/build.py write_blob() writes, and the FNV-1a hash their output lines carry.  Each part lands in a heap
// block of exactly its size, so that a sanitised build sees every byte past it.  Include after the *_host.cpp.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

struct Blob {
  std::vector<std::vector<uint8_t>> parts;
  bool read(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint64_t n = 0;
    while (fread(&n, 8, 1, f) == 1) {
      std::vector<uint8_t> p((size_t)n);
      if (n && fread(p.data(), 1, (size_t)n, f) != (size_t)n) {
        fclose(f);
        return false;
      }
      parts.push_back(std::move(p));
    }
    fclose(f);
    return true;
  }
  void* at(int i) { return parts[i].empty() ? nullptr : parts[i].data(); }   // (an empty part: null)

  // build.py env_parts(): parts[first] Config | the tables, in TablePtrs order | the state, in StatePtrs order
  static constexpr int kEnvParts = 1 + (int)(sizeof(crafter::TablePtrs) / sizeof(void*)) + (int)(sizeof(crafter::StatePtrs) / sizeof(void*));
  bool bind_env(int first, crafter::Config& cfg, crafter::TablePtrs& tb, crafter::StatePtrs& st) {
    if ((int)parts.size() < first + kEnvParts || parts[first].size() != sizeof(cfg)) return false;
    memcpy(&cfg, parts[first].data(), sizeof(cfg));
    void* p[kEnvParts - 1];
    for (int i = 0; i < kEnvParts - 1; i++) p[i] = at(first + 1 + i);
    memcpy(&tb, p, sizeof(tb));
    memcpy(&st, p + sizeof(tb) / sizeof(void*), sizeof(st));
    return true;
  }
};

inline unsigned long long fnv(const void* p, size_t n) {
  const uint8_t* b = (const uint8_t*)p;
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}
