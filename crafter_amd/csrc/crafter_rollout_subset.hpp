// crafter_step_n_envs: crafter_step_n for a chosen subset of the batch, with COMPACT outputs -- step t of the call's i-th env
// writes row t * n + i of obs / reward / done and reads actions[t * n + i] (a [steps][num_envs] frame buffer for 64 scratch rows
// of a 4096-env batch would be 64 x too large).  Three kernels, in a translation unit of their own (crafter_rollout_subset.hip,
// compiled like crafter_rollout.hip: it is a loop around the step): the index check, one workgroup, which records each named
// env's row in a handle-owned [num_envs] scratch; the rollout, n workgroups that each fetch their env from the index list and
// run the resident step on it in rollout_body's loop; and the regeneration kernel behind each stretch, whose queue holds env
// numbers and which finds an env's row in that scratch.
//
// step_body, reset_body and obs_target address actions[env], reward + env, done + env and obs + env * frame.  They are the
// bodies crafter_step and crafter_step_n run, unchanged: they are handed base pointers rebased by (t * n + i) - env.
//
// The bodies below are plain C++ (the CPU harness runs them: tests/hostsim/rollout_envs_host.cpp); the launch functions need hipcc.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "crafter_subset.hpp"
#include "env_kernels.hpp"
#include "launch_plan.hpp"

namespace crafter {

struct RolloutEnvsCheck {
  const int32_t* idx;   // [n] the envs to roll out
  int n;
  int32_t stamp;        // this call's number in mark[] (crafter_handle::copy_stamp: shared with the other index checks)
  int32_t* mark;        // [rows] one word per env
  int32_t* verdict;     // 0: the list is good, the rollout kernels step; 1: refused, they return at once
  EnvRec* rec;
  int rows;             // num_envs
  int32_t* row_of;      // [rows] out: row_of[idx[i]] = i
};

// step_envs_check_body's check (crafter_subset.hpp: every entry in range, no env named twice; a refused call sets *verdict and
// ST_BAD_COPY in the status of every named row that exists, row 0 if none does) -- with the env's row recorded where that one
// scatters the action.  P, flags: as there.
template <class P>
__device__ __forceinline__ void rollout_envs_check_body(const P& p, const RolloutEnvsCheck& c, int* flags) {
  if (p.first() == 0) flags[0] = flags[1] = 0;   // bad, named
  p.sync();
  for (int i = p.first(); i < c.n; i += p.stride()) {
    const int e = c.idx[i];
    if (e < 0 || e >= c.rows) {
      flags[0] = 1;
    } else {
      if (p.exchange(c.mark + e, c.stamp) == c.stamp) flags[0] = 1;   // the second claim of an env
      c.row_of[e] = i;   // (scratch: what a refused call leaves here nobody reads)
    }
  }
  p.sync();
  if (flags[0]) {
    for (int i = p.first(); i < c.n; i += p.stride()) {
      const int e = c.idx[i];
      if (e >= 0 && e < c.rows) {
        p.or_bits(&c.rec[e].status, (uint32_t)ST_BAD_COPY);
        flags[1] = 1;
      }
    }
    p.sync();
    if (p.first() == 0 && !flags[1]) p.or_bits(&c.rec[0].status, (uint32_t)ST_BAD_COPY);
  }
  if (p.first() == 0) *c.verdict = flags[0];
}

// `base` as a body that addresses base[env] has to be given it to reach element `row` of the caller's array (elems: elements
// per row).  Whole-number arithmetic: the rebased pointer may lie outside the array, what the body adds to it does not.
template <class T>
__device__ __forceinline__ T* rebase_row(T* base, int row, int env, size_t elems = 1) {
  return (T*)((uintptr_t)base + (uintptr_t)((ptrdiff_t)(row - env) * (ptrdiff_t)(elems * sizeof(T))));
}

// rollout_body (step_body.hpp) for the call's row-th env: the state staged once, resident over the T steps, the next action
// fetched a step ahead, the env handed to the regeneration kernel when it stops for want of a world.  The one difference is
// where a step's outputs go: row t * n + row of the compact arrays.
template <class W, int LM, int RUL, class S>
__device__ __forceinline__ void rollout_envs_body(W& w, uint8_t* smem, int env, int row, int n, const Config& cfg, const TablePtrs& tb,
                                         const StatePtrs& st, const int32_t* actions, uint8_t* obs, float* reward, uint8_t* done,
                                         const StepCtl& ctl, int T, int32_t* stalled_at) {
  const size_t frame = (size_t)cfg.size_w * cfg.size_h * 3;
  uint32_t carry = 0;   // what the step before left: kResLoaded | kResMapsGone
  int action_next = 0;  // the action of the step after the one running, fetched while that one runs
  uint64_t* prof = st.prof ? st.prof + (size_t)env * 16 : nullptr;   // (stamps 14 / 15: as rollout_body)
  if (prof && w.leader()) prof[14] = w.clock();
#pragma clang loop unroll(disable)
  for (int t = 0; t < T; t++) {
    w.refresh();   // (every step a new thread index and a new env as far as the optimiser can tell: see rollout_body)
    int env_t = W::opaque(env);
    int row_t = t * n + W::opaque(row);
    uint32_t res = carry | (t + 1 < T ? (uint32_t)kResKeep : 0u);
    int action_now = action_next;
    action_next = actions[(size_t)(t + 1 < T ? row_t + n : row_t)];
    uint32_t got = step_body<W, LM, RUL, S, 0, 1>(w, smem, env_t, cfg, tb, st, rebase_row(actions, row_t, env_t),
                                                   obs ? rebase_row(obs, row_t, env_t, frame) : nullptr, rebase_row(reward, row_t, env_t),
                                                   rebase_row(done, row_t, env_t), ctl, res, action_now);
    if (got & kStepStopped) {   // (its state went to global memory: the regeneration kernel takes the env from there)
      if (w.leader()) stalled_at[env_t] = t;
      return;
    }
    carry = kResLoaded | ((got & kStepMapsGone) ? (uint32_t)kResMapsGone : 0u);
  }
  if (prof && w.leader()) prof[15] = w.clock();
}

// requeue_rollout_body (reset_bodies.hpp) for an env of a subset rollout: stopped at step stalled_at[env]; row: row_of[env].
template <class W>
__device__ __forceinline__ void requeue_rollout_envs_body(W& w, uint8_t* smem, int env, int row, int n, const Config& cfg,
                                                 const TablePtrs& tb, const StatePtrs& st, const int32_t* actions, uint8_t* obs,
                                                 float* reward, uint8_t* done, const StepCtl& ctl, int T, const int32_t* stalled_at,
                                                 const LevelTable* levels = nullptr) {
  StatePtrs sq = st;
  sq.reset_q = nullptr;   // an env that stops again is not queued: it is regenerated right here
  const size_t frame = (size_t)cfg.size_w * cfg.size_h * 3;
  int t = stalled_at[env];
  for (;;) {
    reset_body<W>(w, smem, env, cfg, tb, st, obs ? rebase_row(obs, t * n + row, env, frame) : nullptr, ctl.gen_parity, levels);
    w.sync();
    bool stopped = false;
    for (t = t + 1; t < T; t++) {
      const int row_t = t * n + row;
      stopped = (step_body<W, -1, 0, uint16_t>(w, smem, env, cfg, tb, sq, rebase_row(actions, row_t, env),
                                               obs ? rebase_row(obs, row_t, env, frame) : nullptr, rebase_row(reward, row_t, env),
                                               rebase_row(done, row_t, env), ctl) & kStepStopped) != 0;
      w.sync();
      if (stopped) {
        if (st.pool_stats && ctl.gen_parity >= 0 && w.leader()) w.global_add(st.pool_stats + 1, 1);
        break;
      }
    }
    if (!stopped) return;
  }
}

}  // namespace crafter

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace crafter {

struct RolloutEnvsArgs {
  const int32_t* idx;       // [n] workgroup b rolls out env idx[b]
  const int32_t* verdict;   // the check's (one check per call: it stays valid for the call's later stretches)
  const int32_t* row_of;    // [num_envs] the check's output
  int n;
  int T;
  int32_t* stalled_at;      // [num_envs] the step an env stopped at for want of a world (crafter_rollout.hpp RolloutArgs)
};

void launch_rollout_envs_check(const RolloutEnvsCheck& c, hipStream_t stream, hipEvent_t start, hipEvent_t stop);
// instance: LaunchPlan::instance; actions / obs / reward / done: the stretch's first step, compact rows
void launch_rollout_envs(int instance, size_t lds, hipStream_t stream, hipEvent_t start, hipEvent_t stop, const Config& cfg,
                         const TablePtrs& tb, const StatePtrs& st, const int32_t* actions, uint8_t* obs, float* reward, uint8_t* done,
                         const StepCtl& ctl, const RolloutEnvsArgs& ra);
void launch_requeue_rollout_envs(int grid, size_t lds, hipStream_t stream, hipEvent_t start, hipEvent_t stop, const Config& cfg,
                                 const TablePtrs& tb, const StatePtrs& st, const int32_t* actions, uint8_t* obs, float* reward,
                                 uint8_t* done, const StepCtl& ctl, const RolloutEnvsArgs& ra, const LevelTable* levels);
// large worlds (LaunchPlan::opt_in_lds): lets the generic instances take `bytes` of dynamic LDS
hipError_t rollout_envs_allow_lds(int bytes);

}  // namespace crafter
#endif
