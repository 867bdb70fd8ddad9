// TEST INFRASTRUCTURE -- hostsim_reset_worlds (worlds_host.cpp) as a stand-alone program, for builds with
// -fsanitize=address,undefined (sanitised code is never loaded into Python).  Reads one blob written by
// tests/hostsim/worlds_build.py dump(): a HostSimEnv -- config, tables, state buffers -- and the call's arguments, each in a
// heap block of exactly its size; runs the call once and prints one line per env,
//   env status fnv(mat row) fnv(objs row) fnv(mt row) fnv(rec row) fnv(chunk_order row) fnv(census row) fnv(obs row)
// which the test compares with the same call through the shared library.
#include "worlds_host.cpp"
#include "blob.hpp"

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s blob\n", argv[0]);
    return 2;
  }
  Blob b;
  // parts: [n_worlds, bank_max_objects] int32 | Config, tables, state (blob.hpp bind_env)
  //        | mask | world_id | bank_mat | bank_objs | bank_nobj | bank_inv (empty: null)
  Config cfg;
  TablePtrs tb;
  StatePtrs st;
  if (!b.read(argv[1]) || (int)b.parts.size() != 1 + Blob::kEnvParts + 6 || !b.bind_env(1, cfg, tb, st)) {
    fprintf(stderr, "bad blob\n");
    return 2;
  }
  const int32_t* head = (const int32_t*)b.parts[0].data();
  auto at = [&](int i) { return b.at(i); };
  const int a0 = 1 + Blob::kEnvParts;
  const size_t n = (size_t)cfg.num_envs, frame = (size_t)cfg.size_w * cfg.size_h * 3, cells = (size_t)cfg.W * cfg.H;
  const size_t nch = (size_t)cfg.nchunk_x * cfg.nchunk_y;
  std::vector<uint8_t> obs(n * frame);
  const uint8_t* mask = (const uint8_t*)at(a0);
  int rc = hostsim_reset_worlds(&cfg, &tb, &st, mask, (const int32_t*)at(a0 + 1), (const uint8_t*)at(a0 + 2), (const Obj*)at(a0 + 3),
                                (const int32_t*)at(a0 + 4), (const int32_t*)at(a0 + 5), head[0], head[1], obs.data());
  if (rc != 0) return 3;
  for (size_t i = 0; i < n; i++)
    printf("%d %u %016llx %016llx %016llx %016llx %016llx %016llx %016llx\n", (int)i, st.rec[i].status, fnv(st.mat + i * cells, cells),
           fnv(st.objs + i * cfg.max_objects, sizeof(Obj) * (size_t)cfg.max_objects), fnv(st.mt + i * MT_N, 4 * MT_N), fnv(st.rec + i, sizeof(EnvRec)),
           fnv(st.chunk_order + i * nch, 2 * nch), fnv(st.census + i * nch * 5, 20 * nch),
           mask && !mask[i] ? 0ull : fnv(&obs[i * frame], frame));   // (an unnamed row's frame is not this call's)
  return 0;
}
