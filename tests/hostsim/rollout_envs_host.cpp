// TEST INFRASTRUCTURE -- crafter_step_n_envs on the CPU through WaveHost (see wave_host.hpp): the index check's body, the
// rollout body and the regeneration body (csrc/crafter_rollout_subset.hpp) as crafter_rollout_subset.hip runs them, stretch by
// stretch as hostsim_step_n (hostsim.cpp) runs crafter_step_n, then (pool on) the generation batch.
#include <string.h>

#include <vector>

#include "wave_host.hpp"
#include "../../crafter_amd/csrc/crafter_rollout_subset.hpp"

using namespace crafter;

namespace {

// the check's workgroup played by one host thread
struct CheckThreadsHost {
  int first() const { return 0; }
  int stride() const { return 1; }
  void sync() const { asm volatile("" ::: "memory"); }
  int32_t exchange(int32_t* p, int32_t v) const { int32_t old = *p; *p = v; return old; }
  void or_bits(uint32_t* p, uint32_t v) const { *p |= v; }
};

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

// actions [steps][n], obs [steps][n][h][w][3] or null, reward / done [steps][n]: compact rows.  mark: int32[num_envs + 1] kept
// by the caller between calls (the handle's marks, then the verdict word); stamp: the call's number.  pool_mode, stretch as
// hostsim_step_n.  Returns the verdict (0: stepped, 1: refused) or -1 for what the library refuses on the host.
int hostsim_step_n_envs(const Config* cfg, const TablePtrs* tb, const StatePtrs* st, const int32_t* idx, int n, int steps,
                        const int32_t* actions, uint8_t* obs, float* reward, uint8_t* done, int pool_mode, int stretch, int32_t* mark,
                        int32_t stamp) {
  if (n < 0 || n > cfg->num_envs) return -1;
  if (n == 0) return 0;
  if (!idx || !actions || !reward || !done || steps < 1) return -1;
  std::vector<uint8_t> lds(lds_layout(*cfg).total + 64);
  std::vector<int32_t> stalled_at((size_t)cfg->num_envs, -1);
  std::vector<int32_t> row_of((size_t)cfg->num_envs, -1);   // (an unnamed env's row would be no row)
  const LaunchPlan plan = launch_plan(*cfg, is_default_rules(*tb->rules));
  std::vector<uint32_t> night_px(plan.night_px ? (size_t)cfg->num_envs * frame_night_px_words(*cfg) : 0);   // (big_layout)
  RolloutEnvsCheck c;
  c.idx = idx; c.n = n; c.stamp = stamp; c.mark = mark; c.verdict = mark + cfg->num_envs;
  c.rec = (EnvRec*)st->rec; c.rows = cfg->num_envs; c.row_of = row_of.data();
  memset(lds.data(), 0xCD, lds.size());
  rollout_envs_check_body(CheckThreadsHost{}, c, (int*)lds.data());
  StepCtl ctl;
  ctl.parity = 0;
  ctl.gen_parity = pool_mode ? 0 : -1;
  ctl.safe_seq = 0xffffffffu;
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
      memset(lds.data(), 0xCD, lds.size());
      WaveHost w;
      StepCtl big = ctl;
      big.night_px = night_px.data();
      switch (plan.instance) {   // crafter_rollout_subset_kernel<LM, GEO, RUL>, the template arguments as in hostsim_step_n
        case kInstance111:
        case kInstance110:
          rollout_envs_body<WaveHost, -1, 0, uint8_t>(w, lds.data(), env, b, n, *cfg, *tb, *st, a, o, r, d, ctl, T, stalled_at.data());
          break;
        case kInstance100:
          rollout_envs_body<WaveHost, -1, 0, uint16_t>(w, lds.data(), env, b, n, *cfg, *tb, *st, a, o, r, d, ctl, T, stalled_at.data());
          break;
        case kInstance021:
          rollout_envs_body<WaveHost, 0, 1, FarSlot>(w, lds.data(), env, b, n, *cfg, *tb, *st, a, o, r, d, big, T, stalled_at.data());
          break;
        case kInstance000:
          rollout_envs_body<WaveHost, 0, 0, FarSlot>(w, lds.data(), env, b, n, *cfg, *tb, *st, a, o, r, d, big, T, stalled_at.data());
          break;
      }
    }
    if (cfg->auto_reset) {   // the queue walk of crafter_requeue_rollout_subset_kernel
      int32_t* q = st->reset_q;
      int count = (*c.verdict || !q) ? 0 : q[0];
      for (int k = 0; k < count; k++) {
        memset(lds.data(), 0xCD, lds.size());
        WaveHost w;
        const int env = q[4 + k];
        requeue_rollout_envs_body(w, lds.data(), env, row_of[env], n, *cfg, *tb, *st, a, o, r, d, ctl, T, stalled_at.data());
      }
      if (q && !*c.verdict) q[0] = 0;
      if (pool_mode) run_generation(cfg, tb, st, lds);
    }
  }
  return *c.verdict;
}

}  // extern "C"
