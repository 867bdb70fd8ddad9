// TEST INFRASTRUCTURE -- crafter_step_final on the CPU through WaveHost (see wave_host.hpp): the step bodies as hostsim_step
// (hostsim.cpp) runs them, but with StepCtl::gen_parity = -1 as crafter_step_final launches them, and behind them the queue walk
// of crafter_requeue_final_kernel with final_reset_body (csrc/reset_bodies.hpp).
#include "walks.hpp"

using namespace crafter;

extern "C" {

// pool_mode: 0 = world pool off (every finished env regenerates inline), 1 = pool on, generation right after every call.
// split: the rule half / frame half pair where the library would run it.  final_obs / final_local / final_stats may be null.
// Returns the number of envs that came through the queue, or -1 (no auto_reset: the library refuses the call).
int hostsim_step_final(const Config* cfg, const TablePtrs* tb, const StatePtrs* st, const int32_t* actions, uint8_t* obs, float* reward,
                       uint8_t* done, int pool_mode, int split_on, uint8_t* final_obs, uint8_t* terminated, uint8_t* final_local,
                       float* final_stats) {
  if (!cfg->auto_reset || !st->reset_q || !terminated) return -1;
  FakeLds lds = split_step_lds(*cfg);
  const LaunchPlan plan = launch_plan(*cfg, is_default_rules(*tb->rules));
  static CtlScratch scratch;
  const StepCtls c = make_ctls(*cfg, scratch, -1, 1, true);   // gen_parity -1: crafter_step_final's step kernels see the pool as off
  step_batch(plan, step_is_split(*cfg, plan, obs, split_on), c, lds, *cfg, *tb, *st, actions, obs, reward, done);
  // the queue walk of crafter_requeue_final_kernel
  FinalOut fo;
  fo.obs = cfg->render_obs ? final_obs : nullptr;
  fo.terminated = terminated;
  fo.local = final_local;
  fo.stats = final_stats;
  const int count = drain_reset_q(*st, [&](int env) {
    WaveHost w;
    final_reset_body(w, lds.fresh(), env, *cfg, *tb, *st, obs, pool_mode ? 0 : -1, c.ctl.safe_seq, (int32_t*)nullptr, fo);
  });
  if (pool_mode) run_generation(*cfg, *tb, *st, lds);
  return count;
}

}  // extern "C"
