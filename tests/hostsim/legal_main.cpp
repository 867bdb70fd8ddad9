// TEST INFRASTRUCTURE -- hostsim_legal (legal_host.cpp) as a stand-alone program, for builds with -fsanitize=address,undefined
// (sanitised code is never loaded into Python).  Reads one blob written by tests/hostsim/legal_build.py dump(): Config | Rules |
// mat | objmap | objs | rec | row mask (empty: none), each part in a buffer of exactly its size, so that a read past an end is
// a finding.  Prints the mask, one line of 0 / 1 per env ('-' for a row left untouched).
#include "legal_host.cpp"
#include "blob.hpp"

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s blob\n", argv[0]);
    return 2;
  }
  Blob b;
  if (!b.read(argv[1])) return 2;
  std::vector<std::vector<uint8_t>>& parts = b.parts;
  if (parts.size() != 7 || parts[0].size() != sizeof(Config) || parts[1].size() != sizeof(Rules)) {
    fprintf(stderr, "bad blob\n");
    return 2;
  }
  Config cfg;
  memcpy(&cfg, parts[0].data(), sizeof(Config));
  TablePtrs tb;
  StatePtrs st;
  memset(&tb, 0, sizeof(tb));
  memset(&st, 0, sizeof(st));
  tb.rules = (const Rules*)parts[1].data();
  st.mat = parts[2].data();
  st.objmap = (uint16_t*)parts[3].data();
  st.objs = (Obj*)parts[4].data();
  st.rec = (EnvRec*)parts[5].data();
  const size_t cells = (size_t)cfg.W * cfg.H, envs = (size_t)cfg.num_envs, na = (size_t)tb.rules->n_actions;
  if (parts[2].size() != envs * cells || parts[3].size() != envs * cells * 2 || parts[4].size() != envs * cfg.max_objects * sizeof(Obj) ||
      parts[5].size() != envs * sizeof(EnvRec) || (!parts[6].empty() && parts[6].size() != envs))
    return 2;
  std::vector<uint8_t> legal(envs * na, 0xFF);
  if (hostsim_legal(&cfg, &tb, &st, parts[6].empty() ? nullptr : parts[6].data(), legal.data())) return 3;
  for (size_t e = 0; e < envs; e++) {
    for (size_t a = 0; a < na; a++) putchar(legal[e * na + a] == 0xFF ? '-' : '0' + legal[e * na + a]);
    putchar('\n');
  }
  return 0;
}
