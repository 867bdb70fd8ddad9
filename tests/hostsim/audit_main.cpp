// TEST INFRASTRUCTURE -- hostsim_audit (audit_host.cpp) as a stand-alone program, for builds with -fsanitize=address,undefined
// (sanitised code is never loaded into Python).  Reads one blob written by tests/hostsim/audit_build.py dump(): Config | Rules |
// map (4 bytes: objmap is state) | mat | objmap (empty unless map) | objs | rec | chunk_order | chunk_seen | census | row mask
// (empty: none), each part in a buffer of exactly its size, so that a read past an end is a finding.  The body's input is
// untrusted by definition: the rows may hold anything.  Prints one line per env: flags and the four detail words ('-' for a
// row left untouched).
#include "audit_host.cpp"
#include "blob.hpp"

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s blob\n", argv[0]);
    return 2;
  }
  Blob b;
  if (!b.read(argv[1])) return 2;
  std::vector<std::vector<uint8_t>>& parts = b.parts;
  if (parts.size() != 11 || parts[0].size() != sizeof(Config) || parts[1].size() != sizeof(Rules) || parts[2].size() != 4) {
    fprintf(stderr, "bad blob\n");
    return 2;
  }
  Config cfg;
  memcpy(&cfg, parts[0].data(), sizeof(Config));
  int32_t map;
  memcpy(&map, parts[2].data(), 4);
  TablePtrs tb;
  StatePtrs st;
  memset(&tb, 0, sizeof(tb));
  memset(&st, 0, sizeof(st));
  tb.rules = (const Rules*)parts[1].data();
  st.mat = parts[3].data();
  st.objmap = (uint16_t*)b.at(4);
  st.objs = (Obj*)parts[5].data();
  st.rec = (EnvRec*)parts[6].data();
  st.chunk_order = (uint16_t*)parts[7].data();
  st.chunk_seen = parts[8].data();
  st.census = (int32_t*)parts[9].data();
  const size_t cells = (size_t)cfg.W * cfg.H, envs = (size_t)cfg.num_envs, nch = (size_t)cfg.nchunk_x * cfg.nchunk_y;
  if (parts[3].size() != envs * cells || parts[4].size() != (map ? envs * cells * 2 : 0) || parts[5].size() != envs * cfg.max_objects * sizeof(Obj) ||
      parts[6].size() != envs * sizeof(EnvRec) || parts[7].size() != envs * nch * 2 || parts[8].size() != envs * nch ||
      parts[9].size() != envs * nch * 20 || (!parts[10].empty() && parts[10].size() != envs))
    return 2;
  const int32_t untouched = 0x5A5A5A5A;
  std::vector<int32_t> flags(envs, untouched), detail(envs * 4, untouched);
  if (hostsim_audit(&cfg, &tb, &st, map, parts[10].empty() ? nullptr : parts[10].data(), flags.data(), detail.data())) return 3;
  for (size_t e = 0; e < envs; e++) {
    if (flags[e] == untouched) {
      puts("-");
      continue;
    }
    printf("%d %d %d %d %d\n", flags[e], detail[4 * e], detail[4 * e + 1], detail[4 * e + 2], detail[4 * e + 3]);
  }
  return 0;
}
