// TEST INFRASTRUCTURE -- crafter_step_envs on the CPU through WaveHost (see wave_host.hpp): the index check's body and the
// subset kernel's body (csrc/crafter_subset.hpp) as crafter_subset.hip runs them, the step bodies instance by instance as
// hostsim_step (hostsim.cpp) picks them, then the regeneration queue and (pool on) the generation batch.  And the launch
// rule's choose_step_envs (csrc/launch_plan.hpp) as it is.
#include <string.h>

#include <vector>

#include "wave_host.hpp"
#include "../../crafter_amd/csrc/crafter_subset.hpp"

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
  std::vector<uint8_t> lds(lds_layout(*cfg).total + 64);
  const LaunchPlan plan = launch_plan(*cfg, is_default_rules(*tb->rules));
  std::vector<int32_t> scattered((size_t)cfg->num_envs, -1);   // (an action read from an unnamed row would be a bad action)
  SubsetCheck c;
  c.idx = idx; c.actions = actions; c.n = n; c.stamp = stamp; c.mark = mark; c.verdict = mark + cfg->num_envs;
  c.rec = (EnvRec*)st->rec; c.rows = cfg->num_envs; c.scattered = scattered.data();
  memset(lds.data(), 0xCD, lds.size());
  step_envs_check_body(CheckThreadsHost{}, c, (int*)lds.data());
  StepCtl ctl;
  ctl.parity = 0;
  ctl.gen_parity = pool_mode ? 0 : -1;
  ctl.safe_seq = 0xffffffffu;
  ctl.early_frame = 0;   // as crafter_step_envs sets it
  static std::vector<uint32_t> night_px;
  night_px.resize((size_t)cfg->num_envs * frame_night_px_words(*cfg));
  static std::vector<uint32_t> noise_raw;
  noise_raw.resize((size_t)cfg->num_envs * kNoiseStates * MT_N);
  ctl.noise_raw = noise_raw.data();
  for (int b = 0; b < n; b++) {   // workgroup b of the subset launch
    const int env = step_envs_env(idx, c.verdict, b);
    if (env < 0) continue;
    memset(lds.data(), 0xCD, lds.size());
    WaveHost w;
    StepCtl big = ctl;
    big.night_px = night_px.data();
    const int32_t* a = scattered.data();
    switch (plan.instance) {   // the template arguments as in hostsim_step
      case kInstance111:
      case kInstance110:
        step_body<WaveHost, -1, 0, uint8_t>(w, lds.data(), env, *cfg, *tb, *st, a, obs, reward, done, ctl);
        break;
      case kInstance100:
        step_body<WaveHost, -1, 0, uint16_t>(w, lds.data(), env, *cfg, *tb, *st, a, obs, reward, done, ctl);
        break;
      case kInstance021:
        step_body<WaveHost, 0, 1, FarSlot>(w, lds.data(), env, *cfg, *tb, *st, a, obs, reward, done, big);
        break;
      case kInstance000:
        step_body<WaveHost, 0, 0, FarSlot>(w, lds.data(), env, *cfg, *tb, *st, a, obs, reward, done, big);
        break;
    }
  }
  if (cfg->auto_reset) {   // the queue walk of crafter_requeue_reset_kernel, as behind crafter_step
    int32_t* q = st->reset_q;
    int count = q ? q[0] : 0;
    for (int k = 0; k < count; k++) {
      memset(lds.data(), 0xCD, lds.size());
      WaveHost w;
      reset_body(w, lds.data(), q[4 + k], *cfg, *tb, *st, obs, ctl.gen_parity);
    }
    if (q) q[0] = 0;
    if (pool_mode) run_generation(cfg, tb, st, lds);
  }
  return *c.verdict;
}

}  // extern "C"
