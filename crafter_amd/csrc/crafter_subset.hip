// The kernels of crafter_step_envs (a step of a chosen subset of the batch): see crafter_subset.hpp for what they do and why
// they are a translation unit of their own.  Compiled with the step kernel's flags (NOT the rollout unit's).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <vector>

#include "crafter_rollout.hpp"
#include "crafter_subset.hpp"
#include "wave_gfx950.hpp"

namespace crafter {
namespace {

// the check's workgroup (sized like the copy calls' check, env_copy.hpp)
struct CheckThreads {
  __device__ __forceinline__ int first() const { return (int)threadIdx.x; }
  __device__ __forceinline__ int stride() const { return kSubsetCheckThreads; }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
  __device__ __forceinline__ int32_t exchange(int32_t* p, int32_t v) const { return atomicExch(p, v); }
  __device__ __forceinline__ void or_bits(uint32_t* p, uint32_t v) const { atomicOr(p, v); }
};

__global__ void __launch_bounds__(kSubsetCheckThreads)
crafter_step_envs_check_kernel(SubsetCheck c) {
  __shared__ int flags[2];
  step_envs_check_body(CheckThreads{}, c, flags);
}

// Workgroup b steps env idx[b]: crafter_step_kernel's body (entry_kernels.hpp) and launch bounds, instance by instance.
template <int LM, int GEO, int RUL>
__global__ void __launch_bounds__(kStepThreads, step_min_waves(LM))
crafter_step_subset_kernel(Config cfg_in, TablePtrs tb, StatePtrs st, const int32_t* __restrict__ idx, const int32_t* __restrict__ verdict,
                           const int32_t* __restrict__ actions, uint8_t* __restrict__ obs, float* __restrict__ reward,
                           uint8_t* __restrict__ done, StepCtl ctl) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  typedef WaveGfx950<kStepThreads> WS;
  WS w;
  const Config cfg = GEO == 1 ? with_default_geometry(cfg_in) : GEO == 2 ? with_default_view(cfg_in) : cfg_in;
  const int env = step_envs_env(idx, verdict, (int)blockIdx.x);
  if (env < 0) return;   // the list was refused: no row changes
  if constexpr (GEO == 1)
    step_body<WS, LM, RUL, uint8_t>(w, smem, env, cfg, tb, st, actions, obs, reward, done, ctl);
  else
    step_body<WS, LM, RUL, typename StepSlot<LM>::type>(w, smem, env, cfg, tb, st, actions, obs, reward, done, ctl);
}

// The default instance for calls that name at most two envs per CU (launch_plan.hpp kWideMaxEnvs): 512 threads per env, as
// crafter_step_wide_kernel.  Same body, same LDS layout.
constexpr int kSubsetWideThreads = 512;
__global__ void __launch_bounds__(kSubsetWideThreads, 6)
crafter_step_subset_wide_kernel(Config cfg_in, TablePtrs tb, StatePtrs st, const int32_t* __restrict__ idx, const int32_t* __restrict__ verdict,
                                const int32_t* __restrict__ actions, uint8_t* __restrict__ obs, float* __restrict__ reward,
                                uint8_t* __restrict__ done, StepCtl ctl) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  typedef WaveGfx950<kSubsetWideThreads> WS;
  WS w;
  const Config cfg = with_default_geometry(cfg_in);
  const int env = step_envs_env(idx, verdict, (int)blockIdx.x);
  if (env < 0) return;
  step_body<WS, 1, 1, uint8_t>(w, smem, env, cfg, tb, st, actions, obs, reward, done, ctl);
}

}  // namespace

void launch_step_envs_check(const SubsetCheck& c, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
  CRAFTER_LAUNCH(crafter_step_envs_check_kernel, dim3(1), dim3(kSubsetCheckThreads), 0, stream, start, stop, c);
}

void launch_step_subset(StepEnvsKernel kernel, int instance, int n, size_t lds, hipStream_t stream, hipEvent_t start, hipEvent_t stop,
                        const Config& cfg, const TablePtrs& tb, const StatePtrs& st, const int32_t* idx, const int32_t* verdict,
                        const int32_t* scattered, uint8_t* obs, float* reward, uint8_t* done, const StepCtl& ctl) {
  const dim3 grid(n);
  if (kernel == kSubsetWide) {
    CRAFTER_LAUNCH(crafter_step_subset_wide_kernel, grid, dim3(kSubsetWideThreads), lds, stream, start, stop, cfg, tb, st, idx, verdict,
                   scattered, obs, reward, done, ctl);
    return;
  }
  switch (instance) {
#define CRAFTER_X(id, LM, GEO, RUL)                                                                                                    \
    case id:                                                                                                                           \
      CRAFTER_LAUNCH((crafter_step_subset_kernel<LM, GEO, RUL>), grid, dim3(kStepThreads), lds, stream, start, stop, cfg, tb, st, idx, \
                     verdict, scattered, obs, reward, done, ctl);                                                                      \
      break;
    CRAFTER_STEP_INSTANCES(CRAFTER_X)
#undef CRAFTER_X
  }
}

hipError_t subset_allow_lds(int bytes) {
  std::vector<const void*> big;
#define CRAFTER_X(id, LM, GEO, RUL) \
  if constexpr (GEO != 1) big.push_back((const void*)crafter_step_subset_kernel<LM, GEO, RUL>);   // (the default geometry needs 25 KB)
  CRAFTER_STEP_INSTANCES(CRAFTER_X)
#undef CRAFTER_X
  for (const void* f : big) {
    hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace crafter
