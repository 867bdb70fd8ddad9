// TEST INFRASTRUCTURE -- hostsim_step_final (final_host.cpp) as a stand-alone program, for builds with -fsanitize=address,undefined
// (sanitised code is never loaded into Python).  Reads one blob written by tests/hostsim/final_build.py dump(): a HostSimEnv right
// after reset() -- config, tables, state buffers -- and an action tape; plays the tape and prints one line per env that finished,
//   t env terminated fnv(final_obs row) fnv(final_local row) fnv(final_stats row) fnv(obs row)
// which the test compares with the same run through the shared library.
#include "final_host.cpp"
#include "blob.hpp"

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s blob\n", argv[0]);
    return 2;
  }
  Blob b;
  // parts: [steps, pool_mode, split] int32 | Config, tables, state (blob.hpp bind_env) | actions
  Config cfg;
  TablePtrs tb;
  StatePtrs st;
  if (!b.read(argv[1]) || (int)b.parts.size() != 1 + Blob::kEnvParts + 1 || !b.bind_env(1, cfg, tb, st)) {
    fprintf(stderr, "bad blob\n");
    return 2;
  }
  const int32_t* head = (const int32_t*)b.parts[0].data();
  const int T = head[0], pool_mode = head[1], split = head[2];
  const std::vector<uint8_t>& acts = b.parts[1 + Blob::kEnvParts];
  const size_t n = (size_t)cfg.num_envs;
  if (acts.size() != (size_t)T * n * 4) return 2;
  const size_t frame = (size_t)cfg.size_w * cfg.size_h * 3, nl = 2 * (size_t)cfg.local_gw * cfg.local_gh, ns = (size_t)tb.rules->n_items + 4;
  std::vector<uint8_t> obs(n * frame), done(n), final_obs(n * frame, 0xA5), terminated(n, 0xA5), final_local(n * nl, 0xA5);
  std::vector<float> reward(n), final_stats(n * ns, -7.0f);
  for (int t = 0; t < T; t++) {
    int rc = hostsim_step_final(&cfg, &tb, &st, (const int32_t*)acts.data() + (size_t)t * n, obs.data(), reward.data(), done.data(), pool_mode, split,
                                final_obs.data(), terminated.data(), final_local.data(), final_stats.data());
    if (rc < 0) return 3;
    for (size_t i = 0; i < n; i++)
      if (done[i])
        printf("%d %d %d %016llx %016llx %016llx %016llx\n", t, (int)i, (int)terminated[i], fnv(&final_obs[i * frame], frame), fnv(&final_local[i * nl], nl),
               fnv(&final_stats[i * ns], ns * 4), fnv(&obs[i * frame], frame));
  }
  return 0;
}
