// TEST INFRASTRUCTURE -- hostsim_navigate (navigate_host.cpp) as a stand-alone program, for builds with
// -fsanitize=address,undefined (sanitised code is never loaded into Python).  Reads one blob written by
// tests/hostsim/navigate_build.py dump(): Config | Rules | mat | objmap | objs | rec | row mask (empty: none) | the query (16 target
// sets, passable, k, the object path: 19 words), each part in a buffer of exactly its size, so that a read past an end is a
// finding.  Prints one line per env: dist, first and facing of each target ('-' for a row left untouched).
#include "navigate_host.cpp"
#include "blob.hpp"

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s blob\n", argv[0]);
    return 2;
  }
  Blob b;
  if (!b.read(argv[1])) return 2;
  std::vector<std::vector<uint8_t>>& parts = b.parts;
  if (parts.size() != 8 || parts[0].size() != sizeof(Config) || parts[1].size() != sizeof(Rules) || parts[7].size() != 19 * 4) {
    fprintf(stderr, "bad blob\n");
    return 2;
  }
  Config cfg;
  memcpy(&cfg, parts[0].data(), sizeof(Config));
  uint32_t query[19];
  memcpy(query, parts[7].data(), sizeof(query));
  const int k = (int)query[17], force_map = (int)query[18];
  TablePtrs tb;
  StatePtrs st;
  memset(&tb, 0, sizeof(tb));
  memset(&st, 0, sizeof(st));
  tb.rules = (const Rules*)parts[1].data();
  st.mat = parts[2].data();
  st.objmap = (uint16_t*)parts[3].data();
  st.objs = (Obj*)parts[4].data();
  st.rec = (EnvRec*)parts[5].data();
  const size_t cells = (size_t)cfg.W * cfg.H, envs = (size_t)cfg.num_envs;
  if (parts[2].size() != envs * cells || parts[3].size() != envs * cells * 2 || parts[4].size() != envs * cfg.max_objects * sizeof(Obj) ||
      parts[5].size() != envs * sizeof(EnvRec) || (!parts[6].empty() && parts[6].size() != envs) || k < 1 || k > kNavMaxTargets)
    return 2;
  const int32_t untouched = -12345;
  std::vector<int32_t> dist(envs * k, untouched), first(envs * k, untouched);
  std::vector<uint8_t> facing(envs * k, 0xEE);
  std::vector<uint32_t> targets(query, query + k);   // exactly k words
  if (hostsim_navigate(&cfg, &tb, &st, parts[6].empty() ? nullptr : parts[6].data(), targets.data(), k, query[16], dist.data(), first.data(),
                       facing.data(), force_map))
    return 3;
  for (size_t e = 0; e < envs; e++) {
    if (dist[e * k] == untouched) {
      puts("-");
      continue;
    }
    for (int t = 0; t < k; t++) printf("%s%d %d %d", t ? " " : "", (int)dist[e * k + t], (int)first[e * k + t], (int)facing[e * k + t]);
    putchar('\n');
  }
  return 0;
}
