// TEST INFRASTRUCTURE -- what the CPU entry points (the *_host.cpp files) share: the poisoned "LDS", the launch-plan
// instance dispatcher, the StepCtl set-up, the step of one env, the reset_q drain and the world pool's generation walk,
// all over the kernel bodies run through WaveHost (see wave_host.hpp).  One shared object is built per *_host.cpp, so the
// function-local statics below exist once per library.
#pragma once
#include <string.h>

#include <vector>

#include "wave_host.hpp"
#include "../../crafter_amd/csrc/env_kernels.hpp"
#include "../../crafter_amd/csrc/launch_plan.hpp"

namespace crafter {

// a workgroup's LDS played by host memory: every body starts in bytes poisoned afresh
struct FakeLds {
  std::vector<uint8_t> bytes;
  explicit FakeLds(size_t n) : bytes(n) {}
  uint8_t* fresh() {
    memset(bytes.data(), 0xCD, bytes.size());
    return bytes.data();
  }
};
inline FakeLds step_lds(const Config& cfg) { return FakeLds(lds_layout(cfg).total + 64); }
inline FakeLds split_step_lds(const Config& cfg) { return FakeLds(lds_layout(cfg).total + frame_layout(cfg).total + 64); }   // (room for the frame half)

// the index checks' workgroup (crafter_subset.hpp, crafter_rollout_subset.hpp) played by one host thread
struct CheckThreadsHost {
  int first() const { return 0; }
  int stride() const { return 1; }
  void sync() const { asm volatile("" ::: "memory"); }
  int32_t exchange(int32_t* p, int32_t v) const { int32_t old = *p; *p = v; return old; }
  void or_bits(uint32_t* p, uint32_t v) const { *p |= v; }
};

// The StepCtl pair of a walk: `ctl` for the instances whose maps live in LDS, `big` (ctl + night_px) for the two FarSlot
// instances (big_layout: census in place, night pixels in global scratch).
struct StepCtls {
  StepCtl ctl, big;
};
// The scratch behind them.  The step walks keep theirs `static` (it outlives a call, as the library's per-handle scratch
// does); the rollout walks allocate theirs per call.
struct CtlScratch {
  std::vector<uint32_t> night_px, noise_raw;
};
// gen_parity: the gen_q segment that collects requests (-1: the bodies see the pool as off).  early_frame: StepCtl's.
// noise_ahead: the fused step generates a night frame's noise states ahead of the rules (noise_chain); off: the in-frame pass.
// with_night_px: off for a plan that keeps night pixels in LDS (the rollout walks size the scratch by LaunchPlan::night_px).
inline StepCtls make_ctls(const Config& cfg, CtlScratch& s, int gen_parity, int early_frame, bool noise_ahead, bool with_night_px = true) {
  StepCtls c;
  c.ctl.parity = 0;
  c.ctl.gen_parity = gen_parity;
  c.ctl.safe_seq = 0xffffffffu;
  c.ctl.early_frame = early_frame;
  if (noise_ahead) {
    s.noise_raw.resize((size_t)cfg.num_envs * kNoiseStates * MT_N);
    c.ctl.noise_raw = s.noise_raw.data();
  }
  s.night_px.resize(with_night_px ? (size_t)cfg.num_envs * frame_night_px_words(cfg) : 0);
  c.big = c.ctl;
  c.big.night_px = s.night_px.data();
  return c;
}

// The template arguments <LM, RUL, Slot> of crafter_step_kernel / crafter_rollout_kernel / crafter_rollout_subset_kernel for
// each instance of the launch plan; here LM -1 for maps in "LDS", and the staged rules where they are.
template <int LM_, int RUL_, class Slot_>
struct Instance {
  static constexpr int LM = LM_, RUL = RUL_;
  using Slot = Slot_;
};
// f(Instance<...>{}, the StepCtl that instance runs under)
template <class F>
inline void with_instance(const LaunchPlan& plan, const StepCtls& c, F&& f) {
  switch (plan.instance) {
    case kInstance111:
    case kInstance110:   // one-byte slot ids for crafter.Env()'s defaults
      f(Instance<-1, 0, uint8_t>{}, c.ctl);
      break;
    case kInstance100:
      f(Instance<-1, 0, uint16_t>{}, c.ctl);
      break;
    case kInstance021:   // the default rules compiled in
      f(Instance<0, 1, FarSlot>{}, c.big);
      break;
    case kInstance000:
      f(Instance<0, 0, FarSlot>{}, c.big);
      break;
  }
}

// the library splits the default instance only (choose_step); no dispatch order here, and always the early frame
inline bool step_is_split(const Config& cfg, const LaunchPlan& plan, const uint8_t* obs, int split_on) {
  return lane_layout_ok(cfg) && is_split(choose_step(plan, cfg.num_envs, cfg.render_obs && obs, false, split_on ? 1 : 0, 0, 1));
}

// One env through the plan's fused step instance, or (split) through the rules half, crafter_rules_kernel.
inline void step_env(const LaunchPlan& plan, bool split, const StepCtls& c, FakeLds& lds, int env, const Config& cfg, const TablePtrs& tb,
                     const StatePtrs& st, const int32_t* actions, uint8_t* obs, float* reward, uint8_t* done) {
  WaveHost w;
  uint8_t* l = lds.fresh();
  if (split) {
    step_body<WaveHost, -1, 1, LaneSlots, 1>(w, l, env, cfg, tb, st, actions, obs, reward, done, c.ctl);
    return;
  }
  with_instance(plan, c, [&](auto inst, const StepCtl& ctl) {
    using I = decltype(inst);
    step_body<WaveHost, I::LM, I::RUL, typename I::Slot>(w, l, env, cfg, tb, st, actions, obs, reward, done, ctl);
  });
}

// crafter_step's launch over the whole batch: every env through step_env, then (split, and frames are drawn) every env
// through the frame half, crafter_frame_kernel.  lds: split_step_lds.
inline void step_batch(const LaunchPlan& plan, bool split, const StepCtls& c, FakeLds& lds, const Config& cfg, const TablePtrs& tb, const StatePtrs& st,
                       const int32_t* actions, uint8_t* obs, float* reward, uint8_t* done) {
  for (int env = 0; env < cfg.num_envs; env++) step_env(plan, split, c, lds, env, cfg, tb, st, actions, obs, reward, done);
  if (!(split && cfg.render_obs && obs)) return;
  for (int env = 0; env < cfg.num_envs; env++) {
    WaveHost w;
    frame_body(w, lds.fresh(), env, cfg, tb, st, obs, c.big.night_px);
  }
}

// The queue walk of the crafter_requeue_* kernels: body(env) for every env in reset_q, then the queue is emptied.
// refused: the call's index check said no (hostsim_step_n_envs) -- nothing is walked and the queue stays as it is.
// Returns the number of envs walked.
template <class F>
inline int drain_reset_q(const StatePtrs& st, F&& body, bool refused = false) {
  int32_t* q = st.reset_q;
  const int count = (refused || !q) ? 0 : q[0];
  for (int k = 0; k < count; k++) body(q[4 + k]);
  if (q && !refused) q[0] = 0;
  return count;
}

// The world pool's three-kernel pipeline (seed -> classify -> resolve) over the request queue, each stage in freshly
// poisoned "LDS"; always trusted (batch sequence 1).  levels: the level table the seed stage draws from, or null.
inline void run_generation(const Config& cfg, const TablePtrs& tb, const StatePtrs& st, FakeLds& lds, const LevelTable* levels = nullptr) {
  int32_t* q = st.gen_q;
  int count = q ? q[0] : 0;
  if (count > gen_q_capacity(cfg)) count = gen_q_capacity(cfg);
  for (int k = 0; k < count; k++) {
    const int env = q[4 + 2 * k], episode = q[4 + 2 * k + 1];
    WaveHost w;
    gen_seed_body(w, lds.fresh(), env, episode, cfg, tb, st, levels);
    for (int part = 0, parts = gen_classify_parts(cfg); part < parts; part++) gen_classify_body(w, lds.fresh(), env, episode, part, parts, cfg, tb, st);
    gen_resolve_body(w, lds.fresh(), env, episode, 1u, cfg, tb, st);
  }
  if (q) q[0] = 0;
}

}  // namespace crafter
