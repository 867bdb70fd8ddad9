// crafter_step_n's kernels live in a translation unit of their own (crafter_rollout.hip) because they are compiled with
// one more flag: -mllvm -disable-machine-licm.  A rollout is a loop around the step; the machine-level loop-invariant code
// motion pass moves every constant and address a step materialises out of that loop and keeps it in registers across the
// steps (234 VGPRs against the step kernel's 71, two workgroups per CU instead of five); without it the loop costs 9 VGPRs.
// The step kernel itself must not be compiled that way (its inner loops want the pass), hence the second unit.
#pragma once
#include <hip/hip_runtime.h>

#include "env_kernels.hpp"
#include "launch_plan.hpp"

namespace crafter {

// Workgroup sizes both units launch with (compile-time: see WaveGfx950)
constexpr int kStepThreads = 256;      // step / render / rollout workgroup
constexpr int kRequeueThreads = 256;   // inline regeneration (rare): sized like a step workgroup, NOT like crafter_reset_kernel -- a
                                       // 1024-thread workgroup needs a CU with all registers free, and with the world pool's kernels
                                       // resident next to the step kernel even the EMPTY queue check would wait for one (measured: 32 us / step)

// Waves per SIMD that crafter_rollout_kernel and its subset twin (crafter_rollout_subset.hip) are bounded to, instance by
// instance.  The default geometry's instances: six waves per SIMD -- 80 VGPRs -- are what their 26.9 KB of LDS allow per CU;
// left to itself the register allocator takes 83 and loses the sixth workgroup.  GEO 2 (the default view on a world of any
// size, entry_kernels.hpp) likewise; the generic instances need what they need.
constexpr int rollout_min_waves(int LM, int GEO) { return GEO == 1 ? 6 : LM == 0 ? (GEO == 2 ? 6 : 4) : 1; }

// A launch with start / stop events attached (timing mode: hipExtLaunchKernelGGL) or a plain one -- the plain launch is
// the cheaper call on the host, which is what bounds small batches (tools/host_overhead.py).
#define CRAFTER_LAUNCH(kernel, grid, block, lds, stream, start, stop, ...)                                          \
  do {                                                                                                              \
    if ((start) != nullptr || (stop) != nullptr)                                                                    \
      hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, start, stop, 0, __VA_ARGS__);                         \
    else                                                                                                            \
      hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                                            \
  } while (0)

struct RolloutArgs {
  int T;
  size_t obs_stride;      // bytes between the observations of consecutive steps
  int32_t* stalled_at;    // [N] the step an env stopped at for want of a world (valid for the envs in the regeneration queue)
};

// instance: LaunchPlan::instance (launch_plan.hpp CRAFTER_STEP_INSTANCES)
void launch_rollout(int instance, int num_envs, size_t lds, hipStream_t stream, hipEvent_t start, hipEvent_t stop, const Config& cfg,
                    const TablePtrs& tb, const StatePtrs& st, const int32_t* actions, uint8_t* obs, float* reward, uint8_t* done,
                    const StepCtl& ctl, const RolloutArgs& ra);
void launch_requeue_rollout(int grid, size_t lds, hipStream_t stream, hipEvent_t start, hipEvent_t stop, const Config& cfg,
                            const TablePtrs& tb, const StatePtrs& st, const int32_t* actions, uint8_t* obs, float* reward,
                            uint8_t* done, const StepCtl& ctl, const RolloutArgs& ra, const LevelTable* levels);   // levels: env_levels.hpp, null: none
// large worlds (LaunchPlan::opt_in_lds): lets the generic instances take `bytes` of dynamic LDS
hipError_t rollout_allow_lds(int bytes);

}  // namespace crafter
