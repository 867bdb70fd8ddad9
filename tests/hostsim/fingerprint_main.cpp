// TEST INFRASTRUCTURE -- hostsim_fingerprint (fingerprint_host.cpp) as a stand-alone program, for builds with
// -fsanitize=address,undefined (sanitised code is never loaded into Python).  Reads one blob written by
// tests/hostsim/fingerprint_build.py dump(): Config | Rules | mat | objs | mt | rec | chunk_order | row mask (empty: none) | the part
// mask (4 bytes), each part in a buffer of exactly its size, so that a read past an end is a finding.  Prints one line per env:
// the key and the seven part hashes in hex ('-' for a row left untouched).
#include "fingerprint_host.cpp"
#include "blob.hpp"

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s blob\n", argv[0]);
    return 2;
  }
  Blob b;
  if (!b.read(argv[1])) return 2;
  std::vector<std::vector<uint8_t>>& parts = b.parts;
  if (parts.size() != 9 || parts[0].size() != sizeof(Config) || parts[1].size() != sizeof(Rules) || parts[8].size() != 4) {
    fprintf(stderr, "bad blob\n");
    return 2;
  }
  Config cfg;
  memcpy(&cfg, parts[0].data(), sizeof(Config));
  uint32_t which;
  memcpy(&which, parts[8].data(), 4);
  TablePtrs tb;
  StatePtrs st;
  memset(&tb, 0, sizeof(tb));
  memset(&st, 0, sizeof(st));
  tb.rules = (const Rules*)parts[1].data();
  st.mat = parts[2].data();
  st.objs = (Obj*)parts[3].data();
  st.mt = (uint32_t*)parts[4].data();
  st.rec = (EnvRec*)parts[5].data();
  st.chunk_order = (uint16_t*)parts[6].data();
  const size_t cells = (size_t)cfg.W * cfg.H, envs = (size_t)cfg.num_envs, nch = (size_t)cfg.nchunk_x * cfg.nchunk_y;
  if (parts[2].size() != envs * cells || parts[3].size() != envs * cfg.max_objects * sizeof(Obj) || parts[4].size() != envs * MT_N * 4 ||
      parts[5].size() != envs * sizeof(EnvRec) || parts[6].size() != envs * nch * 2 || (!parts[7].empty() && parts[7].size() != envs))
    return 2;
  const uint64_t untouched = 0xA5A5A5A5A5A5A5A5ull;
  std::vector<uint64_t> key(envs, untouched), hash(envs * kFpParts, untouched);
  if (hostsim_fingerprint(&cfg, &tb, &st, parts[7].empty() ? nullptr : parts[7].data(), which, key.data(), hash.data())) return 3;
  for (size_t e = 0; e < envs; e++) {
    if (key[e] == untouched) {
      puts("-");
      continue;
    }
    printf("%016llx", (unsigned long long)key[e]);
    for (int p = 0; p < kFpParts; p++) printf(" %016llx", (unsigned long long)hash[e * kFpParts + p]);
    putchar('\n');
  }
  return 0;
}
