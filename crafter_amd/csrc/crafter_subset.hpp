// crafter_step_envs: a step of a chosen subset of the batch.  Two kernels, in a translation unit of their own
// (crafter_subset.hip) so that the units keep compiling side by side: the index check, one workgroup, which also scatters
// the call's n actions into a handle-owned [num_envs] scratch, and the subset step, n workgroups that each fetch their env
// from the index list and run step_body on it with that scratch as `actions` -- step_body reads actions[env], so the body
// is the one crafter_step runs, unchanged, and the launch costs what a batch of n envs costs.
//
// The bodies below are plain C++ (the CPU harness runs them: tests/hostsim/subset_host.cpp); the launch functions need hipcc.
#pragma once
#include <stdint.h>

#include "env_kernels.hpp"
#include "launch_plan.hpp"

namespace crafter {

constexpr int kSubsetCheckThreads = 1024;   // the check's one workgroup

struct SubsetCheck {
  const int32_t* idx;       // [n] the envs to step
  const int32_t* actions;   // [n] actions[i] is the action of env idx[i]
  int n;
  int32_t stamp;            // this call's number in mark[] (crafter_handle::copy_stamp: shared with the copy calls' check)
  int32_t* mark;            // [rows] one word per env
  int32_t* verdict;         // 0: the list is good, the subset kernel steps; 1: refused, it returns at once
  EnvRec* rec;
  int rows;                 // num_envs
  int32_t* scattered;       // [rows] out: scattered[idx[i]] = actions[i]
};

// Validates the index list before any env steps (one workgroup, no host read-back -- as crafter_copy_check_kernel does for the
// copy calls): every entry in range and no env named twice, since two workgroups would step that env at once.  The same pass
// scatters the actions.  A refused call sets *verdict and ST_BAD_COPY in the status of every named row that exists (row 0 if
// none does).  P: the workgroup's threads (first / stride of a thread's share, barrier, the two global atomics); flags: two
// ints of LDS.
template <class P>
__device__ __forceinline__ void step_envs_check_body(const P& p, const SubsetCheck& c, int* flags) {
  if (p.first() == 0) flags[0] = flags[1] = 0;   // bad, named
  p.sync();
  for (int i = p.first(); i < c.n; i += p.stride()) {
    const int e = c.idx[i];
    if (e < 0 || e >= c.rows) {
      flags[0] = 1;
    } else {
      if (p.exchange(c.mark + e, c.stamp) == c.stamp) flags[0] = 1;   // the second claim of an env
      c.scattered[e] = c.actions[i];   // (scratch: what a refused call leaves here nobody reads)
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

// The env workgroup `block` of a subset launch steps, or -1: the check refused the list.
__device__ __forceinline__ int step_envs_env(const int32_t* __restrict__ idx, const int32_t* __restrict__ verdict, int block) {
  return *verdict ? -1 : idx[block];
}

}  // namespace crafter

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace crafter {

void launch_step_envs_check(const SubsetCheck& c, hipStream_t stream, hipEvent_t start, hipEvent_t stop);
// kernel: choose_step_envs(); instance: LaunchPlan::instance; scattered: the check's output, the step's `actions`
void launch_step_subset(StepEnvsKernel kernel, int instance, int n, size_t lds, hipStream_t stream, hipEvent_t start, hipEvent_t stop,
                        const Config& cfg, const TablePtrs& tb, const StatePtrs& st, const int32_t* idx, const int32_t* verdict,
                        const int32_t* scattered, uint8_t* obs, float* reward, uint8_t* done, const StepCtl& ctl);
// large worlds (LaunchPlan::opt_in_lds): lets the generic instances take `bytes` of dynamic LDS
hipError_t subset_allow_lds(int bytes);

}  // namespace crafter
#endif
