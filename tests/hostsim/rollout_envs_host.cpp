// TEST INFRASTRUCTURE -- crafter_step_n_envs on the CPU through WaveHost (see wave_host.hpp): the index check's body, the
// rollout body and the regeneration body (csrc/crafter_rollout_subset.hpp) as crafter_rollout_subset.hip runs them, stretch by
// stretch as hostsim_step_n (hostsim.cpp) runs crafter_step_n, then (pool on) the generation batch.
#include "walks.hpp"
#include "../../crafter_amd/csrc/crafter_rollout_subset.hpp"

using namespace crafter;

extern "C" {

// actions [steps][n], obs [steps][n][h][w][3] or null, reward / done [steps][n]: compact rows.  mark: int32[num_envs + 1] kept
// by the caller between calls (the handle's marks, then the verdict word); stamp: the call's number.  pool_mode, stretch as
// hostsim_step_n.  Returns the verdict (0: stepped, 1: refused) or -1 for what the library refuses on the host.
int hostsim_step_n_envs(const Config* cfg, const TablePtrs* tb, const StatePtrs* st, const int32_t* idx, int n, int steps,
                        const int32_t* actions, uint8_t* obs, float* reward, uint8_t* done, int pool_mode, int stretch, int32_t* mark,
                        int32_t stamp) {
  if (n < 0 || n > cfg->num_envs) return -1;
  if (n == 0) return 0;
  if (!idx || !actions || !reward || !done || steps < 1) return -1;
  FakeLds lds = step_lds(*cfg);
  std::vector<int32_t> stalled_at((size_t)cfg->num_envs, -1);
  std::vector<int32_t> row_of((size_t)cfg->num_envs, -1);   // (an unnamed env's row would be no row)
  const LaunchPlan plan = launch_plan(*cfg, is_default_rules(*tb->rules));
  RolloutEnvsCheck c;
  c.idx = idx; c.n = n; c.stamp = stamp; c.mark = mark; c.verdict = mark + cfg->num_envs;
  c.rec = (EnvRec*)st->rec; c.rows = cfg->num_envs; c.row_of = row_of.data();
  rollout_envs_check_body(CheckThreadsHost{}, c, (int*)lds.fresh());
  CtlScratch scratch;
  const StepCtls ctls = make_ctls(*cfg, scratch, pool_mode ? 0 : -1, 0, false, plan.night_px != 0);
  const size_t rows = (size_t)n, obs_stride = rows * (size_t)cfg->size_w * cfg->size_h * 3;
  for (int t0 = 0; t0 < steps; t0 += stretch) {
    int T = steps - t0 < stretch ? steps - t0 : stretch;
    const int32_t* a = actions + (size_t)t0 * rows;
    uint8_t* o = obs ? obs + (size_t)t0 * obs_stride : nullptr;
    float* r = reward + (size_t)t0 * rows;
    uint8_t* d = done + (size_t)t0 * rows;
    for (int b = 0; b < n; b++) {   // workgroup b of the rollout launch
      const int env = step_envs_env(idx, c.verdict, b);
      if (env < 0) continue;
      WaveHost w;
      uint8_t* l = lds.fresh();
      with_instance(plan, ctls, [&](auto inst, const StepCtl& ctl) {   // crafter_rollout_subset_kernel<LM, GEO, RUL>
        using I = decltype(inst);
        rollout_envs_body<WaveHost, I::LM, I::RUL, typename I::Slot>(w, l, env, b, n, *cfg, *tb, *st, a, o, r, d, ctl, T, stalled_at.data());
      });
    }
    if (cfg->auto_reset) {   // the queue walk of crafter_requeue_rollout_subset_kernel: a refused call walks nothing and leaves the queue
      drain_reset_q(*st, [&](int env) {
        WaveHost w;
        requeue_rollout_envs_body(w, lds.fresh(), env, row_of[env], n, *cfg, *tb, *st, a, o, r, d, ctls.ctl, T, stalled_at.data());
      }, *c.verdict != 0);
      if (pool_mode) run_generation(*cfg, *tb, *st, lds);
    }
  }
  return *c.verdict;
}

}  // extern "C"
