// TEST INFRASTRUCTURE -- hostsim_nearby (nearby_host.cpp) as a stand-alone program, for builds with -fsanitize=address,undefined
// (sanitised code is never loaded into Python).  Reads one blob written by tests/hostsim/nearby_build.py dump(): Config | Rules |
// map (4 bytes: the instance that may read objmap) | mat | objmap (empty unless map) | objs | rec | row mask (empty: none) | the
// query (distance, flags, classes, k, walk: 5 words), each part in a buffer of exactly its size, so that a read past an end is a
// finding.  The rows may hold anything: the body bounds what it reads.  Prints one line per env: the class counts, n, then the
// k rows of six ('-' for a row left untouched).
#include "nearby_host.cpp"
#include "blob.hpp"

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s blob\n", argv[0]);
    return 2;
  }
  Blob b;
  if (!b.read(argv[1])) return 2;
  std::vector<std::vector<uint8_t>>& parts = b.parts;
  if (parts.size() != 9 || parts[0].size() != sizeof(Config) || parts[1].size() != sizeof(Rules) || parts[2].size() != 4 || parts[8].size() != 5 * 4) {
    fprintf(stderr, "bad blob\n");
    return 2;
  }
  Config cfg;
  memcpy(&cfg, parts[0].data(), sizeof(Config));
  int32_t map, query[5];
  memcpy(&map, parts[2].data(), 4);
  memcpy(query, parts[8].data(), sizeof(query));
  const int k = query[3];
  TablePtrs tb;
  StatePtrs st;
  memset(&tb, 0, sizeof(tb));
  memset(&st, 0, sizeof(st));
  tb.rules = (const Rules*)parts[1].data();
  st.mat = parts[3].data();
  st.objmap = (uint16_t*)b.at(4);
  st.objs = (Obj*)parts[5].data();
  st.rec = (EnvRec*)parts[6].data();
  const size_t cells = (size_t)cfg.W * cfg.H, envs = (size_t)cfg.num_envs, ncls = (size_t)tb.rules->n_materials + 1 + T_PLANT;
  if (parts[3].size() != envs * cells || parts[4].size() != (map ? envs * cells * 2 : 0) || parts[5].size() != envs * cfg.max_objects * sizeof(Obj) ||
      parts[6].size() != envs * sizeof(EnvRec) || (!parts[7].empty() && parts[7].size() != envs) || k < 0 || k > kNearMaxEnts)
    return 2;
  const int32_t untouched = 0x5A5A5A5A;
  std::vector<int32_t> counts(envs * ncls, untouched), n(k ? envs : 0, untouched);   // exactly the sizes crafter_nearby is given
  std::vector<int16_t> ents(envs * k * kNearRow, (int16_t)0x5A5A);
  if (hostsim_nearby(&cfg, &tb, &st, parts[7].empty() ? nullptr : parts[7].data(), query[0], query[1], (uint32_t)query[2], k, counts.data(),
                     k ? ents.data() : nullptr, k ? n.data() : nullptr, map, query[4]))
    return 3;
  for (size_t e = 0; e < envs; e++) {
    if (counts[e * ncls] == untouched) {
      puts("-");
      continue;
    }
    for (size_t c = 0; c < ncls; c++) printf("%d ", (int)counts[e * ncls + c]);
    printf("%d", k ? (int)n[e] : 0);
    for (size_t i = 0; i < (size_t)k * kNearRow; i++) printf(" %d", (int)ents[e * k * kNearRow + i]);
    putchar('\n');
  }
  return 0;
}
