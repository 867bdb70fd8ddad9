// TEST INFRASTRUCTURE -- crafter_step_envs on the CPU through WaveHost (see wave_host.hpp): the index check's body and the
// subset kernel's body (csrc/crafter_subset.hpp) as crafter_subset.hip runs them, the step bodies instance by instance as
// hostsim_step (hostsim.cpp) picks them, then the regeneration queue and (pool on) the generation batch.  And the launch
// rule's choose_step_envs (csrc/launch_plan.hpp) as it is.
#include "walks.hpp"
#include "../../crafter_amd/csrc/crafter_subset.hpp"

using namespace crafter;

extern "C" {

// launch_plan.hpp choose_step_envs for a handle with this config and these rules: 0 the fused instance, 1 the wide kernel;
// out_instance: the plan's instance.  wide: CRAFTER_STEP_WIDE as the library reads it (-1: unset).
int hostsim_choose_step_envs(const Config* cfg, int default_rules, int n, int frames, int wide, int32_t* out_instance) {
  const LaunchPlan p = launch_plan(*cfg, default_rules != 0);
  if (out_instance) *out_instance = p.instance;
  return (int)choose_step_envs(p, n, frames != 0, wide);
}

// mark: int32[num_envs + 1] kept by the caller between calls (the handle's marks, then the verdict word); stamp: the call's
// number.  pool_mode as hostsim_step.  Returns the verdict (0: stepped, 1: refused) or -1 for what the library refuses on the host.
int hostsim_step_envs(const Config* cfg, const TablePtrs* tb, const StatePtrs* st, const int32_t* idx, int n, const int32_t* actions,
                      uint8_t* obs, float* reward, uint8_t* done, int pool_mode, int32_t* mark, int32_t stamp) {
  if (!idx || n < 0 || n > cfg->num_envs) return -1;
  if (n == 0) return 0;
  FakeLds lds = step_lds(*cfg);
  const LaunchPlan plan = launch_plan(*cfg, is_default_rules(*tb->rules));
  std::vector<int32_t> scattered((size_t)cfg->num_envs, -1);   // (an action read from an unnamed row would be a bad action)
  SubsetCheck c;
  c.idx = idx; c.actions = actions; c.n = n; c.stamp = stamp; c.mark = mark; c.verdict = mark + cfg->num_envs;
  c.rec = (EnvRec*)st->rec; c.rows = cfg->num_envs; c.scattered = scattered.data();
  step_envs_check_body(CheckThreadsHost{}, c, (int*)lds.fresh());
  static CtlScratch scratch;
  const StepCtls ctls = make_ctls(*cfg, scratch, pool_mode ? 0 : -1, 0, true);   // early_frame 0, as crafter_step_envs sets it
  for (int b = 0; b < n; b++) {   // workgroup b of the subset launch
    const int env = step_envs_env(idx, c.verdict, b);
    if (env < 0) continue;
    step_env(plan, false, ctls, lds, env, *cfg, *tb, *st, scattered.data(), obs, reward, done);
  }
  if (cfg->auto_reset) {   // the queue walk of crafter_requeue_reset_kernel, as behind crafter_step
    drain_reset_q(*st, [&](int env) {
      WaveHost w;
      reset_body(w, lds.fresh(), env, *cfg, *tb, *st, obs, ctls.ctl.gen_parity);
    });
    if (pool_mode) run_generation(*cfg, *tb, *st, lds);
  }
  return *c.verdict;
}

}  // extern "C"
