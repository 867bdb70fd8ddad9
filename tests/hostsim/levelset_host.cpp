// TEST INFRASTRUCTURE -- level sets (csrc/env_levels.hpp: level_pick, set_levels_body, level_ids_body) on the CPU through WaveHost
// (see wave_host.hpp), and Env.reset / a step with auto-reset / the pool's three generation stages WITH a level table: the
// walks of hostsim.cpp's hostsim_reset and hostsim_step, handing the table to the bodies as the library's kernels do.
#include "walks.hpp"
#include "../../crafter_amd/csrc/env_levels.hpp"

using namespace crafter;

extern "C" {

long long hostsim_level_table_bytes() { return (long long)sizeof(LevelTable); }

// the grid of crafter_set_levels_kernel: whole workgroups over max(n, num_envs), so threads beyond both run too
int hostsim_set_levels(const Config* cfg, const StatePtrs* st, LevelTable* table, const uint64_t* seed_lane, const int32_t* episode,
                       const uint32_t* cum, int n, uint64_t key) {
  const int most = n > cfg->num_envs ? n : cfg->num_envs;
  const int threads = (most + kLevelThreads - 1) / kLevelThreads * kLevelThreads;
  for (int i = 0; i < threads; i++) set_levels_body<WaveHost>(i, *cfg, *st, table, seed_lane, episode, n > 0 ? cum : nullptr, n, key);
  return 0;
}

int hostsim_level_ids(const Config* cfg, const StatePtrs* st, const LevelTable* table, const uint8_t* mask, int32_t* ids) {
  const int threads = (cfg->num_envs + kLevelThreads - 1) / kLevelThreads * kLevelThreads;
  for (int env = 0; env < threads; env++) level_ids_body(env, *cfg, *st, table, mask, ids);
  return 0;
}

// pick over hand-made (lane, k) pairs under `table` (n >= 1)
void hostsim_level_pick(const LevelTable* table, const uint64_t* lanes, const int32_t* k, int32_t* out, int count) {
  for (int i = 0; i < count; i++) out[i] = level_pick(table, lanes[i], k[i]);
}

uint32_t hostsim_level_seed(const LevelTable* table, uint64_t lane, int k) { return level_seed(table, lane, k); }

int hostsim_levelset_reset(const Config* cfg, const TablePtrs* tb, const StatePtrs* st, const LevelTable* table, const uint8_t* mask,
                           int pool_mode, uint8_t* obs) {
  FakeLds lds = step_lds(*cfg);
  for (int env = 0; env < cfg->num_envs; env++) {
    if (mask && !mask[env]) continue;
    WaveHost w;
    reset_body(w, lds.fresh(), env, *cfg, *tb, *st, obs, pool_mode ? 0 : -1, table);
  }
  if (pool_mode) run_generation(*cfg, *tb, *st, lds, table);
  return 0;
}

// the fused step of the default geometry (one-byte slot ids; 1 for any other instance), the regeneration queue, then (pool on)
// the generation batch
int hostsim_levelset_step(const Config* cfg, const TablePtrs* tb, const StatePtrs* st, const LevelTable* table, const int32_t* actions,
                          uint8_t* obs, float* reward, uint8_t* done, int pool_mode) {
  FakeLds lds = split_step_lds(*cfg);
  const LaunchPlan plan = launch_plan(*cfg, is_default_rules(*tb->rules));
  if (plan.instance != kInstance111 && plan.instance != kInstance110) return 1;
  static CtlScratch scratch;
  const StepCtls c = make_ctls(*cfg, scratch, pool_mode ? 0 : -1, 1, true, false);
  for (int env = 0; env < cfg->num_envs; env++) step_env(plan, false, c, lds, env, *cfg, *tb, *st, actions, obs, reward, done);
  if (cfg->auto_reset) {
    drain_reset_q(*st, [&](int env) {
      WaveHost w;
      reset_body(w, lds.fresh(), env, *cfg, *tb, *st, obs, c.ctl.gen_parity, table);
    });
    if (pool_mode) run_generation(*cfg, *tb, *st, lds, table);
  }
  return 0;
}

}  // extern "C"
