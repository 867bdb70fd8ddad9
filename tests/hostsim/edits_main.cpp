// TEST INFRASTRUCTURE -- hostsim_edit_envs (edits_host.cpp) as a stand-alone program, for builds with
// -fsanitize=address,undefined (sanitised code is never loaded into Python).  Reads one blob written by
// tests/hostsim/edits_build.py dump(): a HostSimEnv -- config, tables, state buffers -- and the call's arguments, each in a heap
// block of exactly its size; runs the call once and prints the verdict, then one line per env,
//   env status fnv(mat row) fnv(objmap row) fnv(objs row) fnv(mt row) fnv(rec row) fnv(chunk_order row) fnv(chunk_seen row) fnv(census row)
// which the test compares with the same call through the shared library.
#include "edits_host.cpp"
#include "blob.hpp"

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s blob\n", argv[0]);
    return 2;
  }
  Blob b;
  // parts: [n, ops_per_env, stamp] int32 | Config, tables, state (blob.hpp bind_env) | idx | ops | mark
  Config cfg;
  TablePtrs tb;
  StatePtrs st;
  if (!b.read(argv[1]) || (int)b.parts.size() != 1 + Blob::kEnvParts + 3 || !b.bind_env(1, cfg, tb, st)) {
    fprintf(stderr, "bad blob\n");
    return 2;
  }
  const int32_t* head = (const int32_t*)b.parts[0].data();
  const int a0 = 1 + Blob::kEnvParts;
  const size_t n = (size_t)cfg.num_envs, cells = (size_t)cfg.W * cfg.H, nch = (size_t)cfg.nchunk_x * cfg.nchunk_y;
  if (b.parts[a0].size() != 4 * (size_t)head[0] || b.parts[a0 + 1].size() != 4 * (size_t)head[0] * head[1] * kEditWords ||
      b.parts[a0 + 2].size() != 4 * (n + 1)) {
    fprintf(stderr, "bad blob\n");
    return 2;
  }
  int rc = hostsim_edit_envs(&cfg, &tb, &st, (const int32_t*)b.at(a0), head[0], (const int32_t*)b.at(a0 + 1), head[1], (int32_t*)b.at(a0 + 2),
                             head[2], nullptr);
  if (rc < 0) return 3;
  printf("%d\n", rc);
  for (size_t i = 0; i < n; i++)
    printf("%d %u %016llx %016llx %016llx %016llx %016llx %016llx %016llx %016llx\n", (int)i, st.rec[i].status, fnv(st.mat + i * cells, cells),
           fnv(st.objmap + i * cells, 2 * cells), fnv(st.objs + i * cfg.max_objects, sizeof(Obj) * (size_t)cfg.max_objects),
           fnv(st.mt + i * MT_N, 4 * MT_N), fnv(st.rec + i, sizeof(EnvRec)), fnv(st.chunk_order + i * nch, 2 * nch),
           fnv(st.chunk_seen + i * nch, nch), fnv(st.census + i * nch * 5, 20 * nch));
  return 0;
}
