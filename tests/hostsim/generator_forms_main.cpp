// TEST INFRASTRUCTURE -- the three generator forms of generator_forms_host.cpp as a stand-alone program, for builds with
// -fsanitize=address,undefined (sanitised code is never loaded into Python).  Reads one blob written by
// tests/hostsim/generator_forms_build.py dump(): (env, episode) pairs and a HostSimEnv -- config, tables, state buffers --
// each in a heap block of exactly its size.  Per pair it resets the env into that episode, generates the episode's world
// into its pool entry by the fused form, empties the entry's header and generates it again by the three-stage pipeline,
// and prints one line per form,
//   form env episode nobj mt_pos nchunks_seen fnv(mat) fnv(live slots) fnv(mt) fnv(seen chunk order) fnv(census)
// which the test compares with one another and with the same calls through the shared library.
#include "generator_forms_host.cpp"
#include "blob.hpp"

static void line(const char* form, int env, int episode, int nobj, int mt_pos, int nseen, const Config& cfg, const uint8_t* mat, const Obj* objs,
                 const uint32_t* mt, const uint16_t* order, const int32_t* census) {
  const size_t cells = (size_t)cfg.W * cfg.H, nch = (size_t)cfg.nchunk_x * cfg.nchunk_y;
  printf("%s %d %d %d %d %d %016llx %016llx %016llx %016llx %016llx\n", form, env, episode, nobj, mt_pos, nseen, fnv(mat, cells),
         fnv(objs, sizeof(Obj) * (size_t)nobj), fnv(mt, 4 * MT_N), fnv(order, 2 * (size_t)nseen), fnv(census, 20 * nch));
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s blob\n", argv[0]);
    return 2;
  }
  Blob b;
  // parts: [env, episode] int32 pairs | Config, tables, state (blob.hpp bind_env)
  Config cfg;
  TablePtrs tb;
  StatePtrs st;
  if (!b.read(argv[1]) || (int)b.parts.size() != 1 + Blob::kEnvParts || b.parts[0].size() % 8 != 0 || !b.bind_env(1, cfg, tb, st)) {
    fprintf(stderr, "bad blob\n");
    return 2;
  }
  const int32_t* pairs = (const int32_t*)b.parts[0].data();
  const size_t n = (size_t)cfg.num_envs, frame = (size_t)cfg.size_w * cfg.size_h * 3, cells = (size_t)cfg.W * cfg.H;
  const size_t nch = (size_t)cfg.nchunk_x * cfg.nchunk_y;
  std::vector<uint8_t> obs(n * frame);
  for (size_t k = 0; k < b.parts[0].size() / 8; k++) {
    const int env = pairs[2 * k], episode = pairs[2 * k + 1];
    if (env < 0 || env >= cfg.num_envs || episode < 1) return 3;
    st.rec[env].episode = episode - 1;
    if (hostsim_forms_reset(&cfg, &tb, &st, env, obs.data()) != episode) return 3;
    const EnvRec& r = st.rec[env];
    line("reset", env, episode, r.nobj, r.mt_pos, r.nchunks_seen, cfg, st.mat + env * cells, st.objs + (size_t)env * cfg.max_objects, st.mt + env * MT_N,
         st.chunk_order + env * nch, st.census + env * nch * 5);
    const size_t slot = (size_t)(episode & 1) * n + env;
    PoolHdr* h = st.pool_hdr + slot;
    for (int form = 0; form < 2; form++) {
      memset(h, 0, sizeof(PoolHdr));
      if (form == 0) hostsim_forms_fused(&cfg, &tb, &st, env, episode);
      else hostsim_forms_pipeline(&cfg, &tb, &st, env, episode);
      if (h->ready != ((1ull << 32) | (uint32_t)episode)) return 4;
      line(form == 0 ? "fused" : "pipeline", env, episode, h->nobj, h->mt_pos, h->nchunks_seen, cfg, st.pool_mat + slot * cells,
           st.pool_objs + slot * cfg.max_objects, st.pool_mt + slot * MT_N, st.pool_chunk_order + slot * nch, st.pool_census + slot * nch * 5);
    }
  }
  return 0;
}
