// TEST INFRASTRUCTURE -- CPU execution of the kernel bodies through WaveHost (see wave_host.hpp).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "walks.hpp"

using namespace crafter;

extern "C" {

void hostsim_struct_sizes(int32_t* out) {
  out[0] = sizeof(Obj);
  out[1] = sizeof(EnvRec);
  out[2] = sizeof(Rules);
  out[3] = sizeof(Config);
  out[4] = sizeof(StatePtrs);
  out[5] = sizeof(TablePtrs);
}

int hostsim_lds_bytes(const Config* cfg) { return lds_layout(*cfg).total; }
int hostsim_slot_map_derived(const Config* cfg) { return launch_plan(*cfg, false).maps_in_lds; }

// The library's launch rule (launch_plan.hpp) and nothing else: the plan of a handle with this config and these rules, and the
// choice one crafter_step call with these arguments makes.  order_env / split / wide / early: CRAFTER_ORDER, CRAFTER_SPLIT,
// CRAFTER_STEP_WIDE, CRAFTER_STEP_EARLY as the library reads them (-1: unset).
int hostsim_is_default_rules(const Rules* rules) { return is_default_rules(*rules); }
void hostsim_launch_plan(const Config* cfg, int have_tables, int default_rules, int num_envs, int frames, int order_env, int split, int wide,
                         int early, int lds_pad, int rollout_lds_pad, int32_t out[12]) {
  const LaunchPlan p = launch_plan(*cfg, have_tables && default_rules, lds_pad, rollout_lds_pad);
  const bool ordered = keeps_dispatch_order(num_envs, order_env);
  const StepKernel k = choose_step(p, num_envs, frames != 0, ordered, split, wide, early);
  const int32_t v[12] = {p.instance, p.maps_in_lds, p.gen_geo, p.step_lds, p.rollout_lds, p.render_lds, p.reset_lds, p.night_px, p.opt_in_lds,
                         (int32_t)k, ordered && !is_split(k), step_early_frame(num_envs, early)};
  memcpy(out, v, sizeof(v));
}
// LDS per workgroup of the step kernel's default instance, and of the two kernels of the split step
int hostsim_step_lds_bytes(const Config* cfg) { return lds_layout(*cfg, 1).total; }
int hostsim_rules_lds_bytes(const Config* cfg) { return lane_layout(*cfg).total; }
int hostsim_frame_lds_bytes(const Config* cfg) { return frame_layout(*cfg).total; }

// the renderer's static block (the library builds it on the device when the tables are uploaded)
long long hostsim_render_static_bytes(const Config* cfg) { return (long long)render_static_total_bytes(*cfg); }
void hostsim_build_static(const Config* cfg, const TablePtrs* tb, uint8_t* dst) {
  WaveHost w;
  Env<WaveHost> e(w, *cfg, *tb);
  RenderTarget rt = obs_target<WaveHost>(*cfg, *tb, nullptr, 0);
  Renderer<WaveHost> r(e, rt, dst, nullptr, nullptr);
  r.build_static(dst);
  r.build_lit_sprites(dst, 0, 1);
}

// The kernels' noise3 on its own: perm8[256] is the OpenSimplex permutation (oracle/noise.py builds the same one).
void hostsim_noise3(const uint8_t* perm8, const double* xs, const double* ys, const double* zs, double* out, int n) {
  uint8_t pg3[256];
  for (int i = 0; i < 256; i++) pg3[i] = (uint8_t)(perm8[i] % 24);
  static SimplexLds tab;
  simplex_fill_tables(&tab, [&](int n, auto body) { for (int i = 0; i < n; i++) body(i); });
  Simplex<WaveHost> sx{perm8, pg3, &tab};
  for (int i = 0; i < n; i++) out[i] = sx.noise3(xs[i], ys[i], zs[i]);
}

uint32_t hostsim_world_seed(uint64_t seed_lane, uint64_t episode) { return world_seed(seed_lane, episode); }

// the kernels' pinned exponential (worldgen.hpp exp_cr), compiled for the host: same operations as oracle/exp_cr.py
void hostsim_exp_cr(const double* x, double* out, int n) {
  for (int i = 0; i < n; i++) out[i] = exp_cr(x[i]);
}

// pool_mode: 0 = world pool off, 1 = pool on with generation right after every call (always trusted)
int hostsim_reset(const Config* cfg, const TablePtrs* tb, const StatePtrs* st, const uint8_t* mask,
                  int pool_mode, uint8_t* obs) {
  FakeLds lds = step_lds(*cfg);
  for (int env = 0; env < cfg->num_envs; env++) {
    if (mask && !mask[env]) continue;
    WaveHost w;
    reset_body(w, lds.fresh(), env, *cfg, *tb, *st, obs, pool_mode ? 0 : -1);
  }
  if (pool_mode) run_generation(*cfg, *tb, *st, lds);
  return 0;
}

// 1: steps run as the split pair rules half / frame half (crafter_rules_kernel + crafter_frame_kernel) where the library would
static int g_split = 0;
void hostsim_set_split(int on) { g_split = on; }
// 1 (default, as the library): the fused step generates a night frame's noise states ahead of the rules (noise_chain)
static int g_noise_ahead = 1;
void hostsim_set_noise_ahead(int on) { g_noise_ahead = on; }

int hostsim_step(const Config* cfg, const TablePtrs* tb, const StatePtrs* st, const int32_t* actions,
                 uint8_t* obs, float* reward, uint8_t* done, int pool_mode) {
  FakeLds lds = split_step_lds(*cfg);
  const LaunchPlan plan = launch_plan(*cfg, is_default_rules(*tb->rules));
  static CtlScratch scratch;
  // early_frame 1 (the library: batches larger than the chip holds at once; here always, so that the path is covered)
  const StepCtls c = make_ctls(*cfg, scratch, pool_mode ? 0 : -1, 1, g_noise_ahead != 0);
  step_batch(plan, step_is_split(*cfg, plan, obs, g_split), c, lds, *cfg, *tb, *st, actions, obs, reward, done);
  if (cfg->auto_reset) {
    // same queue walk as crafter_requeue_reset_kernel
    drain_reset_q(*st, [&](int env) {
      WaveHost w;
      reset_body(w, lds.fresh(), env, *cfg, *tb, *st, obs, c.ctl.gen_parity);
    });
    if (pool_mode) run_generation(*cfg, *tb, *st, lds);
  }
  return 0;
}

// crafter_step_n as the library runs it: stretches of at most `stretch` steps (the generation period), every env through
// rollout_body, then the regeneration queue through requeue_rollout_body, then (pool on) the generation batch.
int hostsim_step_n(const Config* cfg, const TablePtrs* tb, const StatePtrs* st, int steps, const int32_t* actions,
                   uint8_t* obs, float* reward, uint8_t* done, int pool_mode, int stretch) {
  FakeLds lds = step_lds(*cfg);
  std::vector<int32_t> stalled_at((size_t)cfg->num_envs, -1);
  const LaunchPlan plan = launch_plan(*cfg, is_default_rules(*tb->rules));
  CtlScratch scratch;
  const StepCtls c = make_ctls(*cfg, scratch, pool_mode ? 0 : -1, 0, false, plan.night_px != 0);
  size_t n = (size_t)cfg->num_envs, obs_stride = n * (size_t)cfg->size_w * cfg->size_h * 3;
  for (int t0 = 0; t0 < steps; t0 += stretch) {
    int T = steps - t0 < stretch ? steps - t0 : stretch;
    const int32_t* a = actions + (size_t)t0 * n;
    uint8_t* o = obs ? obs + (size_t)t0 * obs_stride : nullptr;
    float* r = reward + (size_t)t0 * n;
    uint8_t* d = done + (size_t)t0 * n;
    for (int env = 0; env < cfg->num_envs; env++) {
      WaveHost w;
      uint8_t* l = lds.fresh();
      with_instance(plan, c, [&](auto inst, const StepCtl& ctl) {   // crafter_rollout_kernel<LM, GEO, RUL>
        using I = decltype(inst);
        rollout_body<WaveHost, I::LM, I::RUL, typename I::Slot>(w, l, env, *cfg, *tb, *st, a, o, r, d, ctl, T, obs_stride, stalled_at.data());
      });
    }
    if (cfg->auto_reset) {
      drain_reset_q(*st, [&](int env) {
        WaveHost w;
        requeue_rollout_body(w, lds.fresh(), env, *cfg, *tb, *st, a, o, r, d, c.ctl, T, obs_stride, stalled_at.data());
      });
      if (pool_mode) run_generation(*cfg, *tb, *st, lds);
    }
  }
  return 0;
}

int hostsim_render(const Config* cfg, const TablePtrs* tb, const StatePtrs* st, const uint8_t* mask, uint8_t* out) {
  FakeLds lds = step_lds(*cfg);
  for (int env = 0; env < cfg->num_envs; env++) {
    if (mask && !mask[env]) continue;
    WaveHost w;
    render_body(w, lds.fresh(), env, *cfg, *tb, *st, out);
  }
  return 0;
}

}  // extern "C"
