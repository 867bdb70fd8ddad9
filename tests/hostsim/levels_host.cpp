// TEST INFRASTRUCTURE -- crafter_reseed's body (csrc/env_levels.hpp) on the CPU through WaveHost (see wave_host.hpp).
#include "wave_host.hpp"
#include "../../crafter_amd/csrc/env_levels.hpp"

using namespace crafter;

extern "C" {

// cfg / st: a HostSimEnv's, or hand-made ones.  As the kernel's grid: whole workgroups of kReseedThreads threads, so the
// threads beyond the batch run too and must return without touching anything.
int hostsim_reseed(const Config* cfg, const StatePtrs* st, const uint8_t* mask, const uint64_t* seed_lane, const int32_t* episode) {
  const int threads = (cfg->num_envs + kReseedThreads - 1) / kReseedThreads * kReseedThreads;
  for (int env = 0; env < threads; env++) reseed_body<WaveHost>(env, *cfg, *st, mask, seed_lane, episode);
  return 0;
}

}  // extern "C"
