// Which kernel a call launches, and with how much LDS: the ONE statement of that rule.  Plain C++17 without a HIP runtime
// call -- hipcc compiles it into the library (crafter_hip.hip, crafter_rollout.hip expand their launch switches and LDS
// opt-in lists from the instance list below), g++ into the CPU harness (tests/hostsim), and tests/test_launch_plan.py
// checks it there without a GPU.
//
//   launch_plan()          per handle: crafter_create (rules unknown yet), again in crafter_upload_tables (rules known)
//   choose_step()          per crafter_step call: which of the step kernels of the plan's instance
//   choose_step_envs()     per crafter_step_envs call: which of the subset kernels
//   step_early_frame()     per call: StepCtl::early_frame
//   keeps_dispatch_order() per handle: whether the launches are ordered slow envs first
#pragma once
#include <string.h>

#include "env_kernels.hpp"

namespace crafter {

// The template instances of crafter_step_kernel / crafter_rollout_kernel: X(id, LM, GEO, RUL), id as crafter_step_instance
// reports it (maps in LDS * 4 + default geometry * 2 + default rules, and 8 + 1 for the default view and rules compiled in
// on a world whose maps stay in global memory).  LM 1: maps staged in LDS, 0: large world, maps and slot table in global
// memory (big_layout); GEO 1: crafter.Env()'s geometry compiled in, 2: its view on a world of any size; RUL 1: the uploaded
// rules equal the compiled-in kDefaultRules.
#define CRAFTER_STEP_INSTANCES(X) \
  X(0, 0, 0, 0)                   \
  X(9, 0, 2, 1)                   \
  X(4, 1, 0, 0)                   \
  X(7, 1, 1, 1)                   \
  X(6, 1, 1, 0)

enum StepInstance {
#define CRAFTER_X(id, LM, GEO, RUL) kInstance##LM##GEO##RUL = id,
  CRAFTER_STEP_INSTANCES(CRAFTER_X)
#undef CRAFTER_X
};

// Waves per SIMD that crafter_step_kernel and its subset twin (crafter_subset.hip) are bounded to, instance by instance.  LM 0 --
// maps and slot table in global memory: 19 KB of LDS, registers decide how many share a CU -- takes CRAFTER_BIG_WAVES.
#ifndef CRAFTER_BIG_WAVES
#define CRAFTER_BIG_WAVES 6
#endif
constexpr int step_min_waves(int LM) { return LM == 0 ? CRAFTER_BIG_WAVES : 1; }

constexpr int kEarlyMinEnvs = 8 * 256;   // crafter_step_early_kernel from this many envs on (same-box A/B, profiles/r6_early_frame_ab.txt: 1536 envs -1.0 %, 2048 / 3072 +0.3 %, 4096 +0.1 ... +1.0 %, 8192 +1.2 %)
// crafter_step_wide_kernel for batches of at most two envs per CU (one GPU's share of configs[2]).  Measured
// (profiles/r4zy_wide_ab.txt): kernel 27.8 -> 26.3 us at 512 envs (+4.8 % env-steps/s), +5 % at 256; at 768 envs -5 %, at
// 1024 -18 % (the frame's phases are barrier to barrier: eight waves shorten them far less than they crowd a CU that holds
// three or four envs).
constexpr int kWideMaxEnvs = 2 * 256;
constexpr int kOrderMinEnvs = 5 * 256;   // the dispatch order can only matter when a launch has more workgroups than the chip holds at once (5 per CU)
constexpr int kOrderMaxEnvs = 64 * 256;  // build_order sorts in one workgroup: 64 envs per thread at the most
constexpr int kOptInLds = 64 * 1024;     // dynamic LDS beyond this needs hipFuncAttributeMaxDynamicSharedMemorySize

inline bool is_default_rules(const Rules& r) { return memcmp(&r, &kDefaultRules, sizeof(Rules)) == 0; }

struct LaunchPlan {
  int instance;      // StepInstance
  int maps_in_lds;   // 0: the maps and the cell -> slot map are state in global memory
  int gen_geo;       // GEO of the world pool's generation kernels: 1 = the default geometry compiled in
  int step_lds;      // LDS of a crafter_step launch (fused / early / wide; the split pair has layouts of its own)
  int rollout_lds;   // ... of a crafter_rollout_kernel launch
  int render_lds;    // crafter_render_kernel, crafter_requeue_rollout_kernel: the whole env (lds_layout)
  int reset_lds;     // crafter_reset_kernel, crafter_requeue_reset_kernel (= render_lds unless the maps stay in global memory)
  int night_px;      // big_layout instances: a drawing launch keeps a night frame's pixels in global scratch (StepCtl::night_px)
  int opt_in_lds;    // render_lds > kOptInLds: the generic instances must be allowed that much (large worlds only)
};

// default_rules: tables uploaded AND byte-identical to kDefaultRules (false until crafter_upload_tables: the instance is then
// the one of other rules).  lds_pad / rollout_lds_pad: unused extra LDS per workgroup (occupancy experiments of probe builds).
// Nothing here depends on Config::n_daylight, the one field crafter_extend_daylight changes.
inline LaunchPlan launch_plan(const Config& c, bool default_rules, int lds_pad = 0, int rollout_lds_pad = 0) {
  LaunchPlan p;
  const LdsLayout L = lds_layout(c);
  const bool geo = is_default_geometry(c);   // (implies LDS-resident maps)
  p.maps_in_lds = L.maps_in_lds;
  p.gen_geo = geo ? 1 : 0;
  p.render_lds = L.total;
  p.reset_lds = big_reset_layout(c).total;
  p.opt_in_lds = p.render_lds > kOptInLds;
  p.instance = geo ? (default_rules ? kInstance111 : kInstance110)
             : L.maps_in_lds ? kInstance100
             : (is_default_view(c) && default_rules) ? kInstance021 : kInstance000;
  p.night_px = !L.maps_in_lds;
  switch (p.instance) {
    // The fused instances that run the compiled-in rules stage none: their layout is 280 bytes shorter (lds_layout with_rules
    // false) -- 24,848 B, which lets a SIXTH workgroup onto a CU (round 5; the step kernel's 61 VGPRs allow seven).  Same-box
    // A/B of the closed loop, CRAFTER_LDS_PAD=280 (five) against 0 (six): step kernel 60.9 -> 58.6 us, env-steps/s 62.07 -> 62.23 M
    // at 4096 envs, equal at 1024, no inline regeneration either way (profiles/r5_closed_occupancy_ab.txt): the kernel is
    // shorter, the world pool's kernels get their turn in the gaps instead of beside it.
    case kInstance111:
      p.step_lds = lds_layout(c, 1, false, false).total + lds_pad;
      p.rollout_lds = lds_layout(c, 1, false, false).total + rollout_lds_pad;   // (the resident rollout has a pad of its own)
      break;
    case kInstance110:   // one-byte slot ids (max_objects == 256)
      p.step_lds = p.rollout_lds = lds_layout(c, 1).total + lds_pad;
      break;
    case kInstance100:
      p.step_lds = L.total + lds_pad;
      p.rollout_lds = L.total;
      break;
    default:   // maps and slot table in global memory
      p.step_lds = p.rollout_lds = big_layout(c).total + lds_pad;
      break;
  }
  return p;
}

// The kernels one crafter_step can launch.  Only the default instance has more than the fused one.
enum StepKernel {
  kStepFused,        // crafter_step_kernel<LM, GEO, RUL> of the plan's instance
  kStepEarly,        // crafter_step_early_kernel: batches larger than the chip holds at once
  kStepWide,         // crafter_step_wide_kernel: 512 threads per env, batches of at most two envs per CU
  kStepRules,        // crafter_rules_kernel alone: no frame is drawn
  kStepRulesFrame,   // crafter_rules_kernel + crafter_frame_kernel
};
inline bool is_split(StepKernel k) { return k == kStepRules || k == kStepRulesFrame; }

// StepCtl::early_frame, set on every call whichever kernel runs.  early: CRAFTER_STEP_EARLY (-1 unset, 0 never, 1 always)
inline int step_early_frame(int num_envs, int early) { return early < 0 ? (num_envs >= kEarlyMinEnvs ? 1 : 0) : early; }

// frames: an observation is drawn (cfg.render_obs && obs != nullptr); ordered: the handle keeps a dispatch order (only the
// fused and early kernels follow one; the wide kernel is for batches far too small to have one); split / wide / early: the
// overrides CRAFTER_SPLIT, CRAFTER_STEP_WIDE, CRAFTER_STEP_EARLY (-1 unset, 0 never, 1 always).
// The split pair by default only when no frame is drawn: with frames the fused kernel is faster at every batch size
// measured (round 3, 4096 envs: fused 55.4 M, split pair 42-43 M, overlapped pair 31.5 M env-steps/s).
inline StepKernel choose_step(const LaunchPlan& p, int num_envs, bool frames, bool ordered, int split, int wide, int early) {
  if (p.instance != kInstance111) return kStepFused;
  if (split < 0 ? !frames : split != 0) return frames ? kStepRulesFrame : kStepRules;
  if (!frames) return kStepFused;
  if (!ordered && (wide < 0 ? num_envs <= kWideMaxEnvs : wide != 0)) return kStepWide;
  return step_early_frame(num_envs, early) ? kStepEarly : kStepFused;
}

// The kernels one crafter_step_envs can launch (crafter_subset.hip): n workgroups, one per named env.
enum StepEnvsKernel {
  kSubsetFused,   // crafter_step_subset_kernel<LM, GEO, RUL> of the plan's instance
  kSubsetWide,    // crafter_step_subset_wide_kernel: 512 threads per env, at most two named envs per CU
};

// n: the envs the call names (what fills the chip is the launch, not the batch); frames, wide: as for choose_step.
// No split pair and no early-frame kernel for subsets (StepCtl::early_frame is 0): the measurements behind those two were
// made for launches that fill the chip -- the pair wins only where no frame is drawn over a whole batch, the early frame from
// 2048 workgroups on -- and a subset launch is the case where few workgroups run.  No dispatch order either: the launch
// follows none and builds none (it keeps StepCtl::next_step current for the full launches that do).
inline StepEnvsKernel choose_step_envs(const LaunchPlan& p, int n, bool frames, int wide) {
  if (p.instance != kInstance111 || !frames) return kSubsetFused;
  return (wide < 0 ? n <= kWideMaxEnvs : wide != 0) ? kSubsetWide : kSubsetFused;
}

// Whether a handle orders its launches, slow envs first (crafter_handle::order).  order_env: CRAFTER_ORDER, -1 unset,
// 0 never, > 0 whenever possible.
inline bool keeps_dispatch_order(int num_envs, int order_env) {
  return num_envs <= kOrderMaxEnvs && (order_env > 0 || (order_env < 0 && num_envs > kOrderMinEnvs));
}

}  // namespace crafter
