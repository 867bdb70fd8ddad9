// The kernels of crafter_step_n_envs (an open-loop rollout of a chosen subset of the batch, compact outputs): see
// crafter_rollout_subset.hpp for what they do.  Compiled with the rollout unit's flags (crafter_rollout.hpp: a loop around the step).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <vector>

#include "crafter_rollout.hpp"
#include "crafter_rollout_subset.hpp"
#include "wave_gfx950.hpp"

namespace crafter {
namespace {

// the check's workgroup (as crafter_step_envs_check_kernel's, crafter_subset.hip)
struct CheckThreads {
  __device__ __forceinline__ int first() const { return (int)threadIdx.x; }
  __device__ __forceinline__ int stride() const { return kSubsetCheckThreads; }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
  __device__ __forceinline__ int32_t exchange(int32_t* p, int32_t v) const { return atomicExch(p, v); }
  __device__ __forceinline__ void or_bits(uint32_t* p, uint32_t v) const { atomicOr(p, v); }
};

__global__ void __launch_bounds__(kSubsetCheckThreads)
crafter_rollout_envs_check_kernel(RolloutEnvsCheck c) {
  __shared__ int flags[2];
  rollout_envs_check_body(CheckThreads{}, c, flags);
}

// T steps of env idx[blockIdx.x] in one launch: crafter_rollout_kernel's launch bounds (crafter_rollout.hip), instance by instance
template <int LM, int GEO, int RUL>
__global__ void __launch_bounds__(kStepThreads, rollout_min_waves(LM, GEO))
crafter_rollout_subset_kernel(Config cfg_in, TablePtrs tb, StatePtrs st, const int32_t* __restrict__ actions,
                              uint8_t* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ done,
                              StepCtl ctl, RolloutEnvsArgs ra) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  WaveGfx950<kStepThreads, 1> w;
  const Config cfg = GEO == 1 ? with_default_geometry(cfg_in) : GEO == 2 ? with_default_view(cfg_in) : cfg_in;
  const int row = (int)blockIdx.x;
  const int env = step_envs_env(ra.idx, ra.verdict, row);
  if (env < 0) return;   // the list was refused: no row changes
  if constexpr (GEO == 1)   // max_objects == 256: one-byte slot ids, as in crafter_step_kernel
    rollout_envs_body<WaveGfx950<kStepThreads, 1>, LM, RUL, uint8_t>(w, smem, env, row, ra.n, cfg, tb, st, actions, obs, reward, done, ctl,
                                                                     ra.T, ra.stalled_at);
  else
    rollout_envs_body<WaveGfx950<kStepThreads, 1>, LM, RUL, typename StepSlot<LM>::type>(w, smem, env, row, ra.n, cfg, tb, st, actions, obs,
                                                                                         reward, done, ctl, ra.T, ra.stalled_at);
}

// ... and the regeneration kernel behind it: crafter_requeue_rollout_kernel's walk of the queue and its bounds (four waves per
// SIMD: see there).  The queue holds env numbers; an env's row of the compact outputs is row_of[env].  Behind a refused call
// the queue is empty (nothing stepped, and the launch before cleared this half).
__global__ void __launch_bounds__(kRequeueThreads, 4)
crafter_requeue_rollout_subset_kernel(Config cfg, TablePtrs tb, StatePtrs st, const int32_t* __restrict__ actions, uint8_t* __restrict__ obs,
                                      float* __restrict__ reward, uint8_t* __restrict__ done, StepCtl ctl, RolloutEnvsArgs ra,
                                      const LevelTable* __restrict__ levels) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int32_t* q = st.reset_q + (size_t)ctl.parity * (cfg.num_envs + 4);
  int count = *ra.verdict ? 0 : q[0];
  if (count > ra.n) count = ra.n;   // (only named envs are queued)
  if (blockIdx.x == 0 && threadIdx.x == 0) st.reset_q[(size_t)(1 - ctl.parity) * (cfg.num_envs + 4)] = 0;
  for (int k = (int)blockIdx.x; k < count; k += (int)gridDim.x) {
    WaveGfx950<kRequeueThreads> w;
    const int env = q[4 + k];
    if (env >= 0 && env < cfg.num_envs) {
      const int row = ra.row_of[env];
      if (row >= 0 && row < ra.n)
        requeue_rollout_envs_body(w, smem, env, row, ra.n, cfg, tb, st, actions, obs, reward, done, ctl, ra.T, ra.stalled_at, levels);
    }
    __syncthreads();
  }
}

}  // namespace

void launch_rollout_envs_check(const RolloutEnvsCheck& c, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
  CRAFTER_LAUNCH(crafter_rollout_envs_check_kernel, dim3(1), dim3(kSubsetCheckThreads), 0, stream, start, stop, c);
}

void launch_rollout_envs(int instance, size_t lds, hipStream_t stream, hipEvent_t start, hipEvent_t stop, const Config& cfg,
                         const TablePtrs& tb, const StatePtrs& st, const int32_t* actions, uint8_t* obs, float* reward, uint8_t* done,
                         const StepCtl& ctl, const RolloutEnvsArgs& ra) {
  dim3 grid(ra.n), block(kStepThreads);
  switch (instance) {
#define CRAFTER_X(id, LM, GEO, RUL)                                                                                                                          \
    case id:                                                                                                                                                 \
      CRAFTER_LAUNCH((crafter_rollout_subset_kernel<LM, GEO, RUL>), grid, block, lds, stream, start, stop, cfg, tb, st, actions, obs, reward, done, ctl, ra); \
      break;
    CRAFTER_STEP_INSTANCES(CRAFTER_X)
#undef CRAFTER_X
  }
}

void launch_requeue_rollout_envs(int grid, size_t lds, hipStream_t stream, hipEvent_t start, hipEvent_t stop, const Config& cfg,
                                 const TablePtrs& tb, const StatePtrs& st, const int32_t* actions, uint8_t* obs, float* reward,
                                 uint8_t* done, const StepCtl& ctl, const RolloutEnvsArgs& ra, const LevelTable* levels) {
  CRAFTER_LAUNCH(crafter_requeue_rollout_subset_kernel, dim3(grid), dim3(kRequeueThreads), lds, stream, start, stop, cfg, tb, st, actions,
                 obs, reward, done, ctl, ra, levels);
}

hipError_t rollout_envs_allow_lds(int bytes) {
  std::vector<const void*> big = {(const void*)crafter_requeue_rollout_subset_kernel};
#define CRAFTER_X(id, LM, GEO, RUL) \
  if constexpr (GEO != 1) big.push_back((const void*)crafter_rollout_subset_kernel<LM, GEO, RUL>);   // (the default geometry needs 25 KB)
  CRAFTER_STEP_INSTANCES(CRAFTER_X)
#undef CRAFTER_X
  for (const void* f : big) {
    hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace crafter
