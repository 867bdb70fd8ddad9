// TEST INFRASTRUCTURE -- crafter_step_final on the CPU through WaveHost (see wave_host.hpp): the step bodies as hostsim_step
// (hostsim.cpp) runs them, but with StepCtl::gen_parity = -1 as crafter_step_final launches them, and behind them the queue walk
// of crafter_requeue_final_kernel with final_reset_body (csrc/env_kernels.hpp).
#include <string.h>

#include <vector>

#include "wave_host.hpp"
#include "../../crafter_amd/csrc/env_kernels.hpp"
#include "../../crafter_amd/csrc/launch_plan.hpp"

using namespace crafter;

namespace {

// the world pool's three-kernel pipeline over the request queue, as hostsim.cpp's: always trusted (batch sequence 1)
void run_generation(const Config* cfg, const TablePtrs* tb, const StatePtrs* st, std::vector<uint8_t>& lds) {
  int32_t* q = st->gen_q;
  int count = q ? q[0] : 0;
  if (count > gen_q_capacity(*cfg)) count = gen_q_capacity(*cfg);
  for (int k = 0; k < count; k++) {
    int env = q[4 + 2 * k], episode = q[4 + 2 * k + 1];
    WaveHost w;
    memset(lds.data(), 0xCD, lds.size());
    gen_seed_body(w, lds.data(), env, episode, *cfg, *tb, *st);
    for (int part = 0, parts = gen_classify_parts(*cfg); part < parts; part++) {
      memset(lds.data(), 0xCD, lds.size());
      gen_classify_body(w, lds.data(), env, episode, part, parts, *cfg, *tb, *st);
    }
    memset(lds.data(), 0xCD, lds.size());
    gen_resolve_body(w, lds.data(), env, episode, 1u, *cfg, *tb, *st);
  }
  if (q) q[0] = 0;
}

}  // namespace

extern "C" {

// pool_mode: 0 = world pool off (every finished env regenerates inline), 1 = pool on, generation right after every call.
// split: the rule half / frame half pair where the library would run it.  final_obs / final_local / final_stats may be null.
// Returns the number of envs that came through the queue, or -1 (no auto_reset: the library refuses the call).
int hostsim_step_final(const Config* cfg, const TablePtrs* tb, const StatePtrs* st, const int32_t* actions, uint8_t* obs, float* reward,
                       uint8_t* done, int pool_mode, int split_on, uint8_t* final_obs, uint8_t* terminated, uint8_t* final_local,
                       float* final_stats) {
  if (!cfg->auto_reset || !st->reset_q || !terminated) return -1;
  std::vector<uint8_t> lds(lds_layout(*cfg).total + frame_layout(*cfg).total + 64);
  const LaunchPlan plan = launch_plan(*cfg, is_default_rules(*tb->rules));
  bool split = lane_layout_ok(*cfg) && is_split(choose_step(plan, cfg->num_envs, cfg->render_obs && obs, false, split_on ? 1 : 0, 0, 1));
  StepCtl ctl;
  ctl.parity = 0;
  ctl.gen_parity = -1;   // crafter_step_final: the step kernels see the pool as off
  ctl.safe_seq = 0xffffffffu;
  ctl.early_frame = 1;
  static std::vector<uint32_t> night_px;
  night_px.resize((size_t)cfg->num_envs * frame_night_px_words(*cfg));
  static std::vector<uint32_t> noise_raw;
  noise_raw.resize((size_t)cfg->num_envs * kNoiseStates * MT_N);
  ctl.noise_raw = noise_raw.data();
  bool frames = split && cfg->render_obs && obs;
  for (int env = 0; env < cfg->num_envs; env++) {
    memset(lds.data(), 0xCD, lds.size());
    WaveHost w;
    StepCtl big = ctl;
    big.night_px = night_px.data();
    if (split) {
      step_body<WaveHost, -1, 1, LaneSlots, 1>(w, lds.data(), env, *cfg, *tb, *st, actions, obs, reward, done, ctl);
    } else switch (plan.instance) {
      case kInstance111:
      case kInstance110:
        step_body<WaveHost, -1, 0, uint8_t>(w, lds.data(), env, *cfg, *tb, *st, actions, obs, reward, done, ctl);
        break;
      case kInstance100:
        step_body<WaveHost, -1, 0, uint16_t>(w, lds.data(), env, *cfg, *tb, *st, actions, obs, reward, done, ctl);
        break;
      case kInstance021:
        step_body<WaveHost, 0, 1, FarSlot>(w, lds.data(), env, *cfg, *tb, *st, actions, obs, reward, done, big);
        break;
      case kInstance000:
        step_body<WaveHost, 0, 0, FarSlot>(w, lds.data(), env, *cfg, *tb, *st, actions, obs, reward, done, big);
        break;
    }
  }
  if (frames) {
    for (int env = 0; env < cfg->num_envs; env++) {
      memset(lds.data(), 0xCD, lds.size());
      WaveHost wf;
      frame_body(wf, lds.data(), env, *cfg, *tb, *st, obs, night_px.data());
    }
  }
  // the queue walk of crafter_requeue_final_kernel
  FinalOut fo;
  fo.obs = cfg->render_obs ? final_obs : nullptr;
  fo.terminated = terminated;
  fo.local = final_local;
  fo.stats = final_stats;
  int32_t* q = st->reset_q;
  int count = q[0];
  for (int k = 0; k < count; k++) {
    memset(lds.data(), 0xCD, lds.size());
    WaveHost w;
    final_reset_body(w, lds.data(), q[4 + k], *cfg, *tb, *st, obs, pool_mode ? 0 : -1, ctl.safe_seq, (int32_t*)nullptr, fo);
  }
  q[0] = 0;
  if (pool_mode) run_generation(cfg, tb, st, lds);
  return count;
}

}  // extern "C"
