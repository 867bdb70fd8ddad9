// libcrafter_hip.so: gfx950 kernels + the C ABI of include/crafter_hip.h.
//
// Build (see __graft_entry__.build):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared
// -ffp-contract=off is part of the numerical contract: the render filters, the terrain noise and
// the balance thresholds are float expressions the reference evaluates operation by operation.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/crafter_hip.h"
#include "crafter_rollout.hpp"
#include "crafter_rollout_subset.hpp"
#include "crafter_subset.hpp"
#include "dispatch_order.hpp"
#include "env_copy.hpp"
#include "env_kernels.hpp"
#include "env_levels.hpp"
#include "env_worlds.hpp"
#include "launch_plan.hpp"
#include "legal.hpp"
#include "symbolic.hpp"
#include "wave_gfx950.hpp"

using namespace crafter;

namespace {

constexpr int kResetThreads = 1024;  // reset / generation workgroup (kStepThreads, kRequeueThreads: crafter_rollout.hpp)
constexpr int kRequeueGrid = 256;
constexpr int kRequeueGridPooled = 8;
constexpr int kGenSeedThreads = 64;       // world pool: seeding, one wave per world
constexpr int kGenClassifyThreads = 256;  // terrain classification, four waves per world
constexpr int kGenResolveThreads = 64;    // ordered draws, one wave per world
constexpr int kGenSerialGrid = 2048;      // at most this many single-wave workgroups per batch kernel (they loop over the queue)
constexpr int kGenClassifyGridStep = 304; // ... behind a closed-loop step of the default geometry (round 6, final kernels: a batch's latency is what a device-wide
                                          // synchronize behind a few steps waits for -- the driver's 20-step window 56.3 -> 61.0 M env-steps/s on one box, the
                                          // steady state 65.81 -> 65.58 M; 272: 59.3 / 65.69 M; profiles/r6_headline_grid2.txt -- behind a rollout stretch 256 stays:
                                          // 320 workgroups cost the open loop 3 %, profiles/r6_classify_grid_probe.txt)
constexpr int kGenClassifyGrid = 256;     // workgroups of the classification kernel (they loop over the batch: a world is gen_classify_parts items).
                                          // About one per CU: a classification wave holds 136 VGPRs, and a batch launched at its full width (780
                                          // workgroups at 4096 envs) takes every SIMD's registers, leaving the step kernel one wave slot per SIMD
                                          // instead of five (same-box A/B: 45.0 -> 48.6 M env-steps/s going from 4096 to 256; 128: 47.3, 512: 47.0)
constexpr int kDefaultGenPeriod = 16;  // steps between generation batches (same-box A/B at 4096 envs: 8: 48.5 M, 16: 50.6 M, 32: 36.7 M env-steps/s)
constexpr int kUnpooledStretch = 16;   // crafter_step_n without the world pool: steps per launch
constexpr int kGenRing = 8;   // request-queue segments / batch events
constexpr int kGenLag = 3;    // the launch stream waits for batch j - kGenLag when batch j is launched (<= kGenRing - 2)
constexpr int kGenStreams = 2; // batches alternate between side streams, so two can be in flight
constexpr int kMaxLds = 160 * 1024;

template <int LM, int GEO, int RUL>   // LM 1: maps staged in LDS, 0: large world, maps stay in HBM (env_kernels.hpp bind_lds);
                                     // RUL 1: the uploaded rules equal the compiled-in kDefaultRules (types.hpp)
#ifndef CRAFTER_BIG_WAVES
#define CRAFTER_BIG_WAVES 6
#endif
__global__ void __launch_bounds__(kStepThreads, LM == 0 ? CRAFTER_BIG_WAVES : 1)   // (maps and slot table in global memory: 19 KB of LDS, registers decide how many share a CU)
crafter_step_kernel(Config cfg_in, TablePtrs tb, StatePtrs st, const int32_t* __restrict__ actions,
                    uint8_t* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ done,
                    StepCtl ctl) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  typedef WaveGfx950<kStepThreads> WS;
  WS w;
  const Config cfg = GEO == 1 ? with_default_geometry(cfg_in) : GEO == 2 ? with_default_view(cfg_in) : cfg_in;   // (GEO 2: the default view on a world of any size)
  int env = (int)blockIdx.x;
  if (ctl.order_build) {   // dispatch order in use: block 0 sorts for the launch after this one, block b + 1 steps env order[b]
    if (env == 0) {
      build_order(cfg, tb, ctl.order_build, ctl.next_step, (uint32_t*)smem);
      return;
    }
    env -= 1;
    if (ctl.order) env = ctl.order[env];
  }
  if constexpr (GEO == 1)   // max_objects == 256: one-byte slot ids, 4 KB less LDS per environment
    step_body<WS, LM, RUL, uint8_t>(w, smem, env, cfg, tb, st, actions, obs, reward, done, ctl);
  else
    step_body<WS, LM, RUL, typename StepSlot<LM>::type>(w, smem, env, cfg, tb, st, actions, obs, reward, done, ctl);
}


// The default instance for batches well beyond what the chip holds at once (kEarlyMinEnvs): the same body on a wave policy that
// lets the frame begin before the rules end (wave_gfx950.hpp kEarlyFrame, render.hpp early_frame).
__global__ void __launch_bounds__(kStepThreads)
crafter_step_early_kernel(Config cfg_in, TablePtrs tb, StatePtrs st, const int32_t* __restrict__ actions,
                          uint8_t* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ done, StepCtl ctl) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  typedef WaveGfx950<kStepThreads, 0, 1> WS;
  WS w;
  const Config cfg = with_default_geometry(cfg_in);
  int env = (int)blockIdx.x;
  if (ctl.order_build) {   // (dispatch order: as crafter_step_kernel)
    if (env == 0) {
      build_order(cfg, tb, ctl.order_build, ctl.next_step, (uint32_t*)smem);
      return;
    }
    env -= 1;
    if (ctl.order) env = ctl.order[env];
  }
  step_body<WS, 1, 1, uint8_t>(w, smem, env, cfg, tb, st, actions, obs, reward, done, ctl);
}

// The default instance for batches of at most two envs per CU (launch_plan.hpp kWideMaxEnvs -- one GPU's share of configs[2]):
// 512 threads per env.  A launch of so few envs lasts as long as its slowest env's step, most of the CUs' wave slots are empty,
// and the frame is drawn by eight waves instead of four.  Same body, same LDS layout.
constexpr int kWideThreads = 512;
__global__ void __launch_bounds__(kWideThreads, 6)
crafter_step_wide_kernel(Config cfg_in, TablePtrs tb, StatePtrs st, const int32_t* __restrict__ actions,
                         uint8_t* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ done, StepCtl ctl) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  typedef WaveGfx950<kWideThreads> WS;
  WS w;
  const Config cfg = with_default_geometry(cfg_in);
  step_body<WS, 1, 1, uint8_t>(w, smem, (int)blockIdx.x, cfg, tb, st, actions, obs, reward, done, ctl);
}

// Split step of the default instance (env_kernels.hpp "Split step"): the rule half, one wave per env ...
constexpr int kRulesThreads = 64;
__global__ void __launch_bounds__(kRulesThreads)
crafter_rules_kernel(Config cfg_in, TablePtrs tb, StatePtrs st, const int32_t* __restrict__ actions,
                     uint8_t* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ done, StepCtl ctl) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  WaveGfx950<kRulesThreads> w;
  const Config cfg = with_default_geometry(cfg_in);
  step_body<WaveGfx950<kRulesThreads>, 1, 1, LaneSlots, 1>(w, smem, (int)blockIdx.x, cfg, tb, st, actions, obs, reward, done, ctl);
}

// ... and the frame half, four waves per env, from the frame record the rule half left behind.
__global__ void __launch_bounds__(kStepThreads)
crafter_frame_kernel(Config cfg_in, TablePtrs tb, StatePtrs st, uint8_t* __restrict__ obs, uint32_t* __restrict__ night_px) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  WaveGfx950<kStepThreads> w;
  const Config cfg = with_default_geometry(cfg_in);
  frame_body(w, smem, (int)blockIdx.x, cfg, tb, st, obs, night_px);
}

// One queue entry each.  Kept inlined on purpose: as real functions they need stack copies of the
// argument structs, and that scratch set-up costs the (almost always empty) requeue kernel +10 us
// per step -- measured 10.8 M vs 12.8 M env-steps/s; the spills of the inlined loop only hurt the
// rare fallback path.
__device__ __forceinline__ void gen_one(uint8_t* smem, int env, int episode, uint32_t seq, const Config& cfg,
                                                  const TablePtrs& tb, const StatePtrs& st, const LevelTable* levels) {
  WaveGfx950<kResetThreads> w;
  gen_body(w, smem, env, episode, seq, cfg, tb, st, levels);
}

__device__ __forceinline__ int reset_one(uint8_t* smem, int env, const Config& cfg, const TablePtrs& tb,
                                                   const StatePtrs& st, uint8_t* obs, int gen_parity, const LevelTable* levels) {
  WaveGfx950<kResetThreads> w;
  return reset_body(w, smem, env, cfg, tb, st, obs, gen_parity, levels);
}

// Regenerates the envs queued by the step kernel (auto-reset without a ready pooled world): a small
// grid walks the queue of this step's parity and clears the other parity's counter for the next step.
// levels (here and in the other kernels that seed a world): the handle's level table, null before the first crafter_set_levels.
__global__ void __launch_bounds__(kRequeueThreads, 5)
crafter_requeue_reset_kernel(Config cfg, TablePtrs tb, StatePtrs st, int parity, int gen_parity,
                             uint8_t* __restrict__ obs, const LevelTable* __restrict__ levels) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int32_t* q = st.reset_q + (size_t)parity * (cfg.num_envs + 4);
  int count = q[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) st.reset_q[(size_t)(1 - parity) * (cfg.num_envs + 4)] = 0;
  for (int k = (int)blockIdx.x; k < count; k += (int)gridDim.x) {
    WaveGfx950<kRequeueThreads> w;
    reset_body(w, smem, q[4 + k], cfg, tb, st, obs, gen_parity, levels);
    __syncthreads();
  }
}

// crafter_step_final: takes the place of crafter_requeue_reset_kernel behind a step launch that ran with StepCtl::gen_parity = -1,
// so that EVERY env that finished is in the queue with its terminal state complete in global memory and no frame drawn.  Per
// env: terminated, the terminal state's symbolic pair and frame, then Env.reset from the pool or inline (final_reset_body).
__global__ void __launch_bounds__(kRequeueThreads, 2)
crafter_requeue_final_kernel(Config cfg, TablePtrs tb, StatePtrs st, int parity, int gen_parity, uint32_t safe_seq,
                             uint8_t* __restrict__ obs, int32_t* __restrict__ next_step, FinalOut fo, const LevelTable* __restrict__ levels) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int32_t* q = st.reset_q + (size_t)parity * (cfg.num_envs + 4);
  int count = q[0];
  if (count > cfg.num_envs) count = cfg.num_envs;
  if (blockIdx.x == 0 && threadIdx.x == 0) st.reset_q[(size_t)(1 - parity) * (cfg.num_envs + 4)] = 0;
  for (int k = (int)blockIdx.x; k < count; k += (int)gridDim.x) {
    WaveGfx950<kRequeueThreads> w;
    int env = q[4 + k];
    if (env >= 0 && env < cfg.num_envs) final_reset_body(w, smem, env, cfg, tb, st, obs, gen_parity, safe_seq, next_step, fo, levels);
    __syncthreads();
  }
}

// What a reset kernel's workgroup does to its env's pool entries once the env stands in `episode` (crafter_reset_kernel,
// crafter_reset_worlds_kernel): with the world pool on (gen_parity >= 0) it goes on to generate the NEXT episode's world into
// the env's pool entry, stamped with batch sequence 1 (trusted from the start: the kernel precedes every later step in
// stream order) -- that world may be needed a few dozen steps from now, earlier than any batch could deliver it.
__device__ __forceinline__ void reset_pool_tail(uint8_t* smem, int env, int episode, int gen_parity, const Config& cfg, const TablePtrs& tb,
                                                const StatePtrs& st, const LevelTable* levels) {
  if (gen_parity < 0) return;
  using WR = WaveGfx950<kResetThreads>;
  if (threadIdx.x == 0 && WR::agent_load(st.gen_latest + env) < episode + 1) WR::agent_store(st.gen_latest + env, (int32_t)(episode + 1));
  __threadfence();
  __syncthreads();
  // (not if the entry already holds that world -- a batch delivered it before a reset in mid-episode -- or if an older
  // generation into the entry is still queued: the env then regenerates inline when it gets there.  crafter_reset has
  // ordered this kernel behind every batch in flight, so whatever is stamped is complete.)
  PoolHdr* next = st.pool_hdr + pool_slot(cfg, env, episode + 1);
  int32_t pend = WR::agent_load(&next->pending);
  bool have = gen_done_already<WR>(cfg, st, env, episode + 1), busy = pend != 0 && pend != episode + 1;
  __syncthreads();
  if (!have && !busy) gen_one(smem, env, episode + 1, 1u, cfg, tb, st, levels);
  // ... and asks the pool for the one after it right away (it is due two episodes from now; waiting for the first
  // auto-reset to ask would leave a short second episode without its successor)
  WaveGfx950<kResetThreads> w;
  request_generation(w, cfg, st, gen_parity, env, episode + 2);
}

// Env.reset.  Then reset_pool_tail.
__global__ void __launch_bounds__(kResetThreads)
crafter_reset_kernel(Config cfg, TablePtrs tb, StatePtrs st, const uint8_t* __restrict__ mask,
                     int gen_parity, uint8_t* __restrict__ obs, const LevelTable* __restrict__ levels) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  int env = (int)blockIdx.x;
  if (mask && !mask[env]) return;
  int episode = reset_one(smem, env, cfg, tb, st, obs, -1, levels);
  reset_pool_tail(smem, env, episode, gen_parity, cfg, tb, st, levels);
}

// Env.reset into an authored world of the bank (env_worlds.hpp), one workgroup per env with crafter_reset_kernel's threads and
// LDS; then the same tail: the episode after an authored one is an ordinary generated one.  An env whose world id names no
// world is left alone (its pool entries too).
__global__ void __launch_bounds__(kResetThreads)
crafter_reset_worlds_kernel(Config cfg, TablePtrs tb, StatePtrs st, const uint8_t* __restrict__ mask, WorldBank bank,
                            int gen_parity, uint8_t* __restrict__ obs, const LevelTable* __restrict__ levels) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  int env = (int)blockIdx.x;
  if (mask && !mask[env]) return;
  int episode;
  {
    WaveGfx950<kResetThreads> w;
    episode = reset_world_body(w, smem, env, cfg, tb, st, bank, obs, levels);
  }
  if (episode < 0) return;
  reset_pool_tail(smem, env, episode, gen_parity, cfg, tb, st, levels);
}

// World pool generation (side streams): three kernels per batch, each walking the batch's segment of the request queue
// (env_kernels.hpp gen_seed_body / gen_classify_body / gen_resolve_body).  GEO as for the step kernel.
template <int GEO>
__global__ void __launch_bounds__(kGenSeedThreads)
crafter_gen_seed_kernel(Config cfg_in, TablePtrs tb, StatePtrs st, int parity, int prio, const LevelTable* __restrict__ levels) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  WaveGfx950<kGenSeedThreads>::set_priority(prio);   // (pool_schedule: one wave per world, a chain -- see there)
  const Config cfg = GEO ? with_default_geometry(cfg_in) : cfg_in;
  const int32_t* q = st.gen_q + (size_t)parity * gen_q_stride(cfg);
  int count = q[0];
  if (count > gen_q_capacity(cfg)) count = gen_q_capacity(cfg);
  WaveGfx950<kGenSeedThreads> w;
  for (int k = (int)blockIdx.x; k < count; k += (int)gridDim.x) {
    gen_seed_body(w, smem, q[4 + 2 * k], q[4 + 2 * k + 1], cfg, tb, st, levels);
    __syncthreads();
  }
}

#ifndef CRAFTER_CLASSIFY_WAVES
#define CRAFTER_CLASSIFY_WAVES 6
#endif
template <int GEO>
__global__ void __launch_bounds__(kGenClassifyThreads, GEO ? CRAFTER_CLASSIFY_WAVES : 1)   // (the default geometry only: configs[3] is bound by its generator, profiles/r6_classify_bounds.txt)
crafter_gen_classify_kernel(Config cfg_in, TablePtrs tb, StatePtrs st, int parity, int prio) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  WaveGfx950<kGenClassifyThreads>::set_priority(prio);
  const Config cfg = GEO ? with_default_geometry(cfg_in) : cfg_in;
  const int32_t* q = st.gen_q + (size_t)parity * gen_q_stride(cfg);
  int count = q[0];
  if (count > gen_q_capacity(cfg)) count = gen_q_capacity(cfg);
  WaveGfx950<kGenClassifyThreads> w;
  const int parts = gen_classify_parts(cfg);
  for (int item = (int)blockIdx.x; item < count * parts; item += (int)gridDim.x) {
    int k = item / parts;
    gen_classify_body(w, smem, q[4 + 2 * k], q[4 + 2 * k + 1], item - k * parts, parts, cfg, tb, st);
    __syncthreads();
  }
}

template <int GEO>
__global__ void __launch_bounds__(kGenResolveThreads)
crafter_gen_resolve_kernel(Config cfg_in, TablePtrs tb, StatePtrs st, int parity, uint32_t seq, int prio) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  WaveGfx950<kGenResolveThreads>::set_priority(prio);
  const Config cfg = GEO ? with_default_geometry(cfg_in) : cfg_in;
  const int32_t* q = st.gen_q + (size_t)parity * gen_q_stride(cfg);
  int count = q[0];
  if (count > gen_q_capacity(cfg)) count = gen_q_capacity(cfg);
  WaveGfx950<kGenResolveThreads> w;
  for (int k = (int)blockIdx.x; k < count; k += (int)gridDim.x) {
    gen_resolve_body(w, smem, q[4 + 2 * k], q[4 + 2 * k + 1], seq, cfg, tb, st);
    __syncthreads();
  }
}

#ifdef CRAFTER_PROBES
// TIMING PROBE (CRAFTER_PROBE_FREE_GEN=2): workgroups that only OCCUPY what a generation kernel's workgroups occupy -- threads,
// registers (the launch bound's share), LDS -- for `us` microseconds each, asleep: what does the generator cost the step loop by
// being resident, as opposed to by what it executes?
template <int BIG>   // BIG: the wave holds 112 vector registers (a classification wave's allocation), else a handful
__global__ void __launch_bounds__(kStepThreads)
crafter_gen_occupy_kernel(int us, int items, uint32_t* sink) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  if (BIG) asm volatile("v_mov_b32 v111, 0" ::: "v111");
  for (int k = (int)blockIdx.x; k < items; k += (int)gridDim.x) {
    uint64_t t0 = wall_clock64();
    while ((long long)(wall_clock64() - t0) < (long long)us * 100) __builtin_amdgcn_s_sleep(32);   // 100 MHz constant clock
  }
  if (sink && threadIdx.x == 0 && smem[0] == 0xA5) sink[0] = 1;   // (keeps the LDS allocation alive)
}

// TIMING PROBE (CRAFTER_PROBE_FREE_GEN=1, probe builds only -- results are WRONG by construction): what would the step loop
// do with a generator that costs nothing?  Instead of the three generation kernels a batch launches this one, which stamps every
// requested pool entry as ready without generating it: the entry keeps whatever world it held (an entry that never held one
// takes a copy of its env's other entry first -- crafter_reset_kernel filled that), so finished envs adopt worlds of the right
// shape and every step does its usual work, while no generation kernel runs beside it (VERDICT r5 #1a).
template <int GEO>
__global__ void __launch_bounds__(kStepThreads)
crafter_gen_stamp_kernel(Config cfg_in, TablePtrs tb, StatePtrs st, int parity, uint32_t seq) {
  typedef WaveGfx950<kStepThreads> WS;
  const Config cfg = GEO ? with_default_geometry(cfg_in) : cfg_in;
  const int32_t* q = st.gen_q + (size_t)parity * gen_q_stride(cfg);
  int count = q[0];
  if (count > gen_q_capacity(cfg)) count = gen_q_capacity(cfg);
  const int cells = cfg.W * cfg.H, nch = cfg.nchunk_x * cfg.nchunk_y;
  for (int k = (int)blockIdx.x; k < count; k += (int)gridDim.x) {
    int env = q[4 + 2 * k], episode = q[4 + 2 * k + 1];
    size_t slot = pool_slot(cfg, env, episode), other = pool_slot(cfg, env, episode + 1);
    PoolHdr* h = st.pool_hdr + slot;
    bool skip = !gen_wanted<WS>(st, env, episode) || gen_done_already<WS>(cfg, st, env, episode);
    bool never = (WS::agent_load(&h->ready) >> 32) == 0;
    __syncthreads();
    if (!skip && never) {
      const uint4* a = (const uint4*)(st.pool_mat + other * cells);
      uint4* b = (uint4*)(st.pool_mat + slot * cells);
      for (int i = (int)threadIdx.x; i < cells / 16; i += kStepThreads) b[i] = a[i];
      const uint4* oa = (const uint4*)(st.pool_objs + other * cfg.max_objects);
      uint4* ob = (uint4*)(st.pool_objs + slot * cfg.max_objects);
      for (int i = (int)threadIdx.x; i < cfg.max_objects; i += kStepThreads) ob[i] = oa[i];
      for (int i = (int)threadIdx.x; i < MT_N; i += kStepThreads) st.pool_mt[slot * MT_N + i] = st.pool_mt[other * MT_N + i];
      for (int i = (int)threadIdx.x; i < nch; i += kStepThreads) st.pool_chunk_order[slot * nch + i] = st.pool_chunk_order[other * nch + i];
      for (int i = (int)threadIdx.x; i < nch * 5; i += kStepThreads) st.pool_census[slot * nch * 5 + i] = st.pool_census[other * nch * 5 + i];
      if (threadIdx.x == 0) {
        const PoolHdr* o = st.pool_hdr + other;
        h->mt_pos = o->mt_pos; h->nobj = o->nobj; h->nchunks_seen = o->nchunks_seen; h->pad = o->pad;
      }
    }
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
      if (!skip) WS::agent_store(&h->ready, ((uint64_t)seq << 32) | (uint32_t)episode);
      gen_retire<WS>(cfg, st, env, episode);
    }
    __syncthreads();
  }
}
#endif

__global__ void __launch_bounds__(kStepThreads)
crafter_render_kernel(Config cfg, TablePtrs tb, StatePtrs st, const uint8_t* __restrict__ mask,
                      uint8_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  int env = (int)blockIdx.x;
  if (mask && !mask[env]) return;
  WaveGfx950<kStepThreads> w;
  render_body(w, smem, env, cfg, tb, st, out);
}

// crafter_symbolic (symbolic.hpp): one wave per env, kSymbolicEnvs envs per workgroup, each wave in its own LDS strip.  No
// barrier: the waves of the batch tail and of masked rows leave at once.  MAP: the cell -> slot map is state (maps in global memory).
template <int MAP>
__global__ void __launch_bounds__(kSymbolicThreads)
crafter_symbolic_kernel(Config cfg, TablePtrs tb, StatePtrs st, const uint8_t* __restrict__ mask, uint8_t* __restrict__ local,
                        float* __restrict__ stats, int strip_bytes) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  typedef WaveGfx950<kSymbolicThreads> WS;
  WS w;
  const int wave = WS::uni((int)(threadIdx.x >> 6));
  symbolic_body<WS, MAP>(w, smem + wave * strip_bytes, (int)blockIdx.x * kSymbolicEnvs + wave, cfg, tb, st, mask, local, stats);
}

// crafter_legal_actions (legal.hpp): one wave per env, kLegalEnvs envs per workgroup, no LDS and no barrier: the waves of the
// batch tail and of masked rows leave at once.  MAP as for crafter_symbolic_kernel.
template <int MAP>
__global__ void __launch_bounds__(kLegalThreads)
crafter_legal_actions_kernel(Config cfg, TablePtrs tb, StatePtrs st, const uint8_t* __restrict__ mask, uint8_t* __restrict__ legal) {
  typedef WaveGfx950<kLegalThreads> WL;
  WL w;
  const int wave = WL::uni((int)(threadIdx.x >> 6));
  legal_body<WL, MAP>(w, (int)blockIdx.x * kLegalEnvs + wave, cfg, tb, st, mask, legal);
}

// crafter_reseed (env_levels.hpp): one thread per env edits its record and empties its two pool entries.
__global__ void __launch_bounds__(kReseedThreads)
crafter_reseed_kernel(Config cfg, StatePtrs st, const uint8_t* __restrict__ mask, const uint64_t* __restrict__ seed_lane,
                      const int32_t* __restrict__ episode) {
  reseed_body<WaveGfx950<kReseedThreads>>((int)(blockIdx.x * kReseedThreads + threadIdx.x), cfg, st, mask, seed_lane, episode);
}

// crafter_set_levels (env_levels.hpp): thread i copies table entry i and empties env i's pool entries; thread 0 writes the head.
__global__ void __launch_bounds__(kLevelThreads)
crafter_set_levels_kernel(Config cfg, StatePtrs st, LevelTable* __restrict__ table, const uint64_t* __restrict__ seed_lane,
                          const int32_t* __restrict__ episode, const uint32_t* __restrict__ cum, int n, uint64_t key) {
  set_levels_body<WaveGfx950<kLevelThreads>>((int)(blockIdx.x * kLevelThreads + threadIdx.x), cfg, st, table, seed_lane, episode, cum, n, key);
}

// crafter_level_ids: one thread per env, read-only.
__global__ void __launch_bounds__(kLevelThreads)
crafter_level_ids_kernel(Config cfg, StatePtrs st, const LevelTable* __restrict__ table, const uint8_t* __restrict__ mask,
                         int32_t* __restrict__ ids) {
  level_ids_body((int)(blockIdx.x * kLevelThreads + threadIdx.x), cfg, st, table, mask, ids);
}

// Builds the renderer's static block once per table upload (one workgroup).
__global__ void __launch_bounds__(kStepThreads)
crafter_init_tables_kernel(Config cfg, TablePtrs tb, uint8_t* dst) {
  WaveGfx950<kStepThreads> w;
  Env<WaveGfx950<kStepThreads>> e(w, cfg, tb);
  RenderTarget rt = obs_target<WaveGfx950<kStepThreads>>(cfg, tb, nullptr, 0);
  Renderer<WaveGfx950<kStepThreads>> r(e, rt, dst, nullptr, nullptr);
  r.build_static(dst);
}

// ... and the lit sprite rows behind it (render.hpp render_lit_sprite_bytes: 78 MB), one workgroup per (asleep, step)
__global__ void __launch_bounds__(kStepThreads)
crafter_init_lit_sprites_kernel(Config cfg, TablePtrs tb, uint8_t* dst) {
  WaveGfx950<kStepThreads> w;
  Env<WaveGfx950<kStepThreads>> e(w, cfg, tb);
  RenderTarget rt = obs_target<WaveGfx950<kStepThreads>>(cfg, tb, nullptr, 0);
  Renderer<WaveGfx950<kStepThreads>> r(e, rt, dst, nullptr, nullptr);
  r.build_lit_sprites(dst, (int)blockIdx.x, (int)gridDim.x);
}

// Unit-test access to the device's own transcendental-free noise and to the two libm calls of worldgen.py:25-27 as the
// generation kernels evaluate them (the pinned exp_cr of worldgen.hpp / sqrt): crafter_debug_eval.  mode 0: out = noise3(x, y, z)
// with the permutation perm[256]; 1: out = 1 / (1 + exp_cr(-x)); 2: out = 4 - sqrt(x); 3: out = exp_cr(x).
__global__ void __launch_bounds__(kStepThreads)
crafter_debug_eval_kernel(const uint8_t* __restrict__ perm, const double* __restrict__ x, const double* __restrict__ y,
                          const double* __restrict__ z, double* __restrict__ out, long long n, int mode) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* s_perm = smem;
  uint8_t* s_pg3 = smem + 256;
  SimplexLds* s_tab = (SimplexLds*)(smem + 512);
  if (mode == 0) {
    for (int i = (int)threadIdx.x; i < 256; i += kStepThreads) {
      s_perm[i] = perm[i];
      s_pg3[i] = (uint8_t)(perm[i] % 24);
    }
    simplex_fill_tables(s_tab, [&](int n, auto body) { for (int i = (int)threadIdx.x; i < n; i += kStepThreads) body(i); });
  }
  __syncthreads();
  Simplex<WaveGfx950<kStepThreads>> sx{s_perm, s_pg3, s_tab};
  for (long long i = (long long)blockIdx.x * kStepThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kStepThreads) {
    double v;
    if (mode == 0) v = sx.noise3(x[i], y[i], z[i]);
    else if (mode == 1) v = 1 / (1 + exp_cr(-x[i]));
    else if (mode == 3) v = exp_cr(x[i]);
    else v = 4 - __builtin_sqrt(x[i]);
    out[i] = v;
  }
}

thread_local std::string g_create_error;

// Experiment knobs.  The shipped library reads NONE of them: only a probe build (tools/ab_make.sh <name> tree -DCRAFTER_PROBES ->
// gpurun_ab/<name>.so, loaded through CRAFTER_HIP_LIB by the tools under tools/) looks at the environment.  What stays in every
// build are the four DISPATCH OVERRIDES documented in include/crafter_hip.h (CRAFTER_SPLIT, CRAFTER_ORDER, CRAFTER_STEP_WIDE, CRAFTER_STEP_EARLY):
// they choose between kernels the product ships, and the GPU tests use them to drive each of those at every batch size.
static const char* probe_env(const char* name) {
#ifdef CRAFTER_PROBES
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}

}  // namespace

// The renderer's derived tables (static block, inventory cells, lit rows, night pixel records: 5.7 MB for the default
// geometry, render.hpp; 85 MB while they held lit sprite rows too) depend on the frame geometry, the rules' sizes and the uploaded tables only: handles
// with the same inputs on the same device share one allocation -- a process with a few hundred `crafter_amd.Env` objects
// (each its own handle) would otherwise hold that many copies, and build them.
struct SharedBlock {
  void* ptr = nullptr;
  int refs = 0;
};
static std::mutex g_blocks_mutex;
static std::map<std::string, SharedBlock> g_blocks;   // key: device | content hash | size

static uint64_t fnv1a(uint64_t h, const void* p, size_t n) {
  const uint8_t* b = (const uint8_t*)p;
  for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}
// a second, independent 64-bit digest of the same bytes (the cache key carries both: ADVICE r2 -- a hit is trusted without
// comparing the megabytes it stands for)
static uint64_t mix64(uint64_t h, const void* p, size_t n) {
  const uint8_t* b = (const uint8_t*)p;
  for (size_t i = 0; i < n; i++) {
    h += b[i] + 0x9e3779b97f4a7c15ull;
    h = (h ^ (h >> 30)) * 0xbf58476d1ce4e5b9ull;
    h = (h ^ (h >> 27)) * 0x94d049bb133111ebull;
    h ^= h >> 31;
  }
  return h;
}

struct crafter_handle {
  Config cfg;
  TablePtrs tb;
  StatePtrs st;
  bool have_tables = false;
  bool have_state = false;
  std::vector<void*> owned;   // device allocations of the handle (tables)
  std::string shared_block_key;   // its entry in g_blocks (the renderer's derived tables), empty: none
  LaunchPlan plan;   // which step / rollout instance, in how much LDS (launch_plan.hpp): crafter_create, again in crafter_upload_tables
  int gen_resolve_lds_bytes = 0;
  int split = -1;                         // CRAFTER_SPLIT=0 / 1: the default instance never / always steps as rules kernel (+ frame kernel);
                                          // -1: when no frame is drawn (launch_plan.hpp choose_step)
  int requeue_grid = kRequeueGridPooled;  // CRAFTER_REQUEUE_GRID (A/B): workgroups of the inline-regeneration kernel while the pool runs
  int gen_lag = kGenLag;                  // CRAFTER_GEN_LAG (A/B): back-pressure distance in batches, 1 .. kGenRing - 2
  int classify_grid = kGenClassifyGrid;   // CRAFTER_GEN_CLASSIFY_GRID: workgroups of the classification kernel (A/B)
  int classify_grid_step = kGenClassifyGrid;   // ... of a batch launched behind a closed-loop step (kGenClassifyGridStep for the default geometry)
  long long steps = 0;
  std::string err;
  // world pool (asynchronous generation on a side stream)
  bool pool = false;
  // Schedule: batch j is launched on side stream j % kGenStreams every gen_period steps over request-queue
  // segment j % kGenRing and records event j % kGenRing behind itself.  Trust (safe_seq: the step kernel only adopts
  // worlds of batches <= safe_seq and regenerates inline otherwise -- unobservable: same generator, same
  // (seed, episode)) advances two ways: every crafter_step polls the oldest untrusted batch's event (non-blocking,
  // so a batch is usually trusted one period after its launch), and when batch j is launched the launch stream is
  // ordered behind batch j - kGenLag (hipStreamWaitEvent: the host does not block).  That wait is the back-pressure
  // that keeps generation ahead of demand: generation workgroups need a whole CU's registers and only get one when a
  // step kernel drains.  The burst a reset of all envs would cause does not exist: crafter_reset_kernel generates the
  // next world itself (sequence number 1).
  hipStream_t side[2] = {nullptr, nullptr};
  // dispatch order of the step launch (StepCtl::order): slow envs first.  Only where it can pay -- more envs than the chip
  // holds at once -- and only for the fused step kernel
  int32_t* order = nullptr;       // [2][N]: launch k reads half k & 1 (built during launch k - 1), builds half (k + 1) & 1
  int32_t* next_step = nullptr;   // [N]
  uint64_t ordered_launches = 0;
  const int32_t* order_override = nullptr;   // diagnostics: crafter_debug_set_dispatch_order
  int lds_pad = 0;                        // CRAFTER_LDS_PAD
  int rollout_order = 1;                  // CRAFTER_ROLLOUT_ORDER=0 (A/B): rollout launches in arrival order
  int rollout_lds_pad = 0;                // CRAFTER_ROLLOUT_LDS_PAD (A/B): extra LDS per workgroup of crafter_rollout_kernel<1, 1, 1> (26,872 B: six per CU)
  int32_t* stalled_at = nullptr;          // crafter_step_n: per env, the step of the call it stopped at for want of a world (-1: none)
  uint32_t* night_px = nullptr;           // split step: scratch of the frame kernel, a night frame's pixels in noise-stream order per env
  uint32_t* noise_raw = nullptr;          // fused step: the MT19937 states a night frame's noise comes from, generated ahead of the rules
                                          // (env_kernels.hpp noise_chain), kNoiseStates * 624 words per env; CRAFTER_NOISE_AHEAD=0: off (A/B)
  int noise_ahead = 1;
  hipStream_t aux = nullptr;              // split step: the regeneration kernel runs here, beside the frame kernel
  int wide = -1;                          // CRAFTER_STEP_WIDE=0|1: never / always the 512-thread step kernel of the default instance (default: batches of <= kWideMaxEnvs)
  hipEvent_t ev_rules = nullptr, ev_requeue = nullptr;
  hipEvent_t ev_main = nullptr;
  int probe_lds[3] = {-1, -1, -1}, probe_big = 0;   // CRAFTER_PROBE_OCCUPY_LDS="seed,classify,resolve" bytes; CRAFTER_PROBE_OCCUPY_BIG=1: 112 VGPRs per classify / resolve wave
  int probe_worlds = 0, probe_us[3] = {80, 120, 300};   // CRAFTER_PROBE_OCCUPY="worlds,seed_us,classify_item_us,resolve_us"
  int probe_free_gen = 0;            // CRAFTER_PROBE_FREE_GEN (probe builds): batches stamp their requests ready without generating
  int early_frame = -1;                   // CRAFTER_STEP_EARLY=0|1: never / always crafter_step_early_kernel for the default instance (default: batches of at least kEarlyMinEnvs envs)
  int gen_classify_prio = 0;              // CRAFTER_GEN_CLASSIFY_PRIO (probe builds): s_setprio of the classification kernel's waves
  int gen_serial_prio = -1;               // CRAFTER_GEN_SERIAL_PRIO (A/B): s_setprio of the seeding / draw kernels of every batch; -1: 2 behind a rollout stretch, 1 behind a step
  bool fold_main_event = true;            // CRAFTER_FOLD_MAIN_EVENT=0 (A/B): crafter_step_n marks the launch stream with a packet of its own
  hipEvent_t ev_gen[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  uint32_t batches = 1;        // launched so far; sequence number 1 = worlds generated inside crafter_reset_kernel
  uint32_t safe_seq = 1;       // trusted so far: every batch <= safe_seq is known complete ON safe_stream (or to the host)
  uint32_t polled_seq = 1;     // ... known complete to the host (event query): valid whatever stream the next call uses
  hipStream_t safe_stream = nullptr;   // the stream the stream-side waits behind safe_seq were enqueued on
  bool have_safe_stream = false;
  hipStream_t last_stream = nullptr;   // the stream of the last call that enqueued kernels (adopt_stream: ADVICE r4)
  bool have_last_stream = false;
  hipEvent_t ev_switch = nullptr;
  bool pool_failed = false;    // a HIP call of the scheduler failed: no more batches, finished envs regenerate inline
  std::string pool_err;
  int gen_parity = 0;          // segment collecting requests now
  int steps_since_gen = 0;
  int gen_period = 8;
  // crafter_copy_envs / _save_envs / _load_envs: the index check's per-row marks ([N], stamped with copy_stamp) and verdict
  int32_t* copy_mark = nullptr;
  int32_t* copy_verdict = nullptr;
  int32_t copy_stamp = 0;
  LevelTable* levels = nullptr;        // crafter_set_levels: the level table (env_levels.hpp), allocated once at full capacity by the first call;
                                       // every kernel that seeds a world takes it as a launch argument (null: no table yet)
  int32_t* subset_actions = nullptr;   // crafter_step_envs: [N] the call's actions scattered to their envs' rows (step_body reads actions[env])
  int32_t* rollout_row_of = nullptr;   // crafter_step_n_envs: [N] the row of the call's compact outputs each named env writes (its place in idx)
  // optional per-kernel timing (HIP events on the launch stream)
  bool timing = false;
  std::vector<hipEvent_t> events;   // triples: before step, between, after reset
};

static int fail(crafter_handle* h, const std::string& msg) {
  if (h)
    h->err = msg;
  else
    g_create_error = msg;
  return 1;
}

static int hip_fail(crafter_handle* h, const char* what, hipError_t e) {
  return fail(h, std::string(what) + ": " + hipGetErrorString(e));
}

// The three kernels of generation batch `seq` over request segment `seg`, for the plan's GEO
template <int GEO>
static void launch_generation(crafter_handle* h, hipStream_t side, dim3 gs, dim3 gc, int seg, uint32_t seq, int prio) {
  hipLaunchKernelGGL(crafter_gen_seed_kernel<GEO>, gs, dim3(kGenSeedThreads), kGenSeedLds, side, h->cfg, h->tb, h->st, seg, prio, (const LevelTable*)h->levels);
  hipLaunchKernelGGL(crafter_gen_classify_kernel<GEO>, gc, dim3(kGenClassifyThreads), gen_classify_lds_bytes(h->cfg), side, h->cfg, h->tb, h->st, seg, h->gen_classify_prio);
  hipLaunchKernelGGL(crafter_gen_resolve_kernel<GEO>, gs, dim3(kGenResolveThreads), h->gen_resolve_lds_bytes, side, h->cfg, h->tb,
                     h->st, seg, seq, prio);
}
#ifdef CRAFTER_PROBES
template <int GEO>
static void launch_generation_stamp(crafter_handle* h, hipStream_t side, int seg, uint32_t seq) {
  hipLaunchKernelGGL(crafter_gen_stamp_kernel<GEO>, dim3(64), dim3(kStepThreads), 0, side, h->cfg, h->tb, h->st, seg, seq);
}
#endif

extern "C" {

void crafter_struct_sizes(int32_t out[6]) {
  out[0] = sizeof(Obj);
  out[1] = sizeof(EnvRec);
  out[2] = sizeof(Rules);
  out[3] = sizeof(Config);
  out[4] = sizeof(StatePtrs);
  out[5] = sizeof(TablePtrs);
}

int32_t crafter_abi_version(void) { return 7; }

int crafter_create(const crafter_config* cfg, crafter_handle** out) {
  if (!cfg || !out) return fail(nullptr, "crafter_create: null argument");
  const Config& c = *cfg;
  if (c.num_envs < 1) return fail(nullptr, "crafter_create: num_envs < 1");
  if (c.W < 1 || c.H < 1 || c.W * c.H > 4 * 65536) return fail(nullptr, "crafter_create: bad area");
  if (c.max_objects < 2 || c.max_objects > 65535) return fail(nullptr, "crafter_create: bad max_objects");
  if (c.unit_x < 1 || c.unit_y < 1 || c.local_gw < 1 || c.local_gh < 1)
    return fail(nullptr, "crafter_create: bad view geometry");
  if (c.size_w < 1 || c.size_h < 1 || (long long)c.size_w * c.size_h > (1 << 22))   // pixel offsets use 24-bit multiplies
    return fail(nullptr, "crafter_create: bad image size (at most 2^22 pixels)");
  if (render_static_bytes(c) + sprite_rows_bytes(c) > kRenderStaticBound)
    return fail(nullptr, "crafter_create: image size too large for the renderer's LDS tables (width + height of the view in pixels)");
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count < 1)
    return fail(nullptr, "crafter_create: no HIP device visible (this library has no CPU path)");
  crafter_handle* h = new crafter_handle();
  h->cfg = c;
  if (const char* pad = probe_env("CRAFTER_LDS_PAD")) h->lds_pad = atoi(pad) > 0 ? atoi(pad) : 0;   // occupancy experiments: unused extra LDS per workgroup
  if (const char* v = probe_env("CRAFTER_ROLLOUT_ORDER")) h->rollout_order = atoi(v) != 0;
  if (const char* v = probe_env("CRAFTER_FOLD_MAIN_EVENT")) h->fold_main_event = atoi(v) != 0;
  if (const char* v = probe_env("CRAFTER_GEN_SERIAL_PRIO")) h->gen_serial_prio = atoi(v);
  if (const char* v = probe_env("CRAFTER_GEN_CLASSIFY_PRIO")) h->gen_classify_prio = atoi(v);
  if (const char* v = probe_env("CRAFTER_PROBE_FREE_GEN")) h->probe_free_gen = atoi(v);
  if (const char* v = probe_env("CRAFTER_PROBE_OCCUPY_LDS")) sscanf(v, "%d,%d,%d", &h->probe_lds[0], &h->probe_lds[1], &h->probe_lds[2]);
  if (const char* v = probe_env("CRAFTER_PROBE_OCCUPY_BIG")) h->probe_big = atoi(v);
  if (const char* v = probe_env("CRAFTER_PROBE_OCCUPY")) sscanf(v, "%d,%d,%d,%d", &h->probe_worlds, &h->probe_us[0], &h->probe_us[1], &h->probe_us[2]);
  if (const char* pad = probe_env("CRAFTER_ROLLOUT_LDS_PAD")) h->rollout_lds_pad = atoi(pad) > 0 ? atoi(pad) : 0;   // ... of the resident rollout kernel
  h->plan = launch_plan(c, false, h->lds_pad, h->rollout_lds_pad);   // (the rules are not known yet)
  h->gen_resolve_lds_bytes = gen_resolve_layout(c).total;
  if (const char* v = probe_env("CRAFTER_GEN_LAG")) h->gen_lag = atoi(v) >= 1 && atoi(v) <= kGenRing - 2 ? atoi(v) : kGenLag;
  if (const char* v = getenv("CRAFTER_SPLIT")) h->split = atoi(v) < 0 ? -1 : atoi(v) != 0 ? 1 : 0;
  if (const char* v = probe_env("CRAFTER_NOISE_AHEAD")) h->noise_ahead = atoi(v) != 0;
  if (const char* v = getenv("CRAFTER_STEP_WIDE")) h->wide = atoi(v) != 0 ? 1 : 0;
  if (const char* v = getenv("CRAFTER_STEP_EARLY")) h->early_frame = atoi(v) != 0 ? 1 : 0;
  if (const char* v = probe_env("CRAFTER_REQUEUE_GRID")) h->requeue_grid = atoi(v) >= 1 && atoi(v) <= kRequeueGrid ? atoi(v) : kRequeueGridPooled;
  // large worlds (maps in HBM): two classification workgroups per CU -- their step workgroups leave the registers, and a batch
  // is sixteen times the cells (8192 x 256x256, r4i: 256 / 512 / 1024 workgroups = 9.18 / 10.14 / 9.16 M env-steps/s)
  if (!h->plan.maps_in_lds) h->classify_grid = 2 * kGenClassifyGrid;
  h->classify_grid_step = h->plan.gen_geo ? kGenClassifyGridStep : h->classify_grid;
  if (const char* v = probe_env("CRAFTER_GEN_CLASSIFY_GRID")) h->classify_grid = h->classify_grid_step = atoi(v) > 0 ? atoi(v) : h->classify_grid;
  if (h->plan.render_lds > kMaxLds) {
    std::string msg = "crafter_create: one environment needs " + std::to_string(h->plan.render_lds) +
                      " B of LDS (> 160 KiB): area / max_objects too large for the LDS-resident kernels";
    delete h;
    return fail(nullptr, msg);
  }
  if ((c.step_threads != 0 && c.step_threads != kStepThreads) || (c.reset_threads != 0 && c.reset_threads != kResetThreads)) {
    delete h;
    return fail(nullptr, "crafter_create: workgroup sizes are fixed in this build (step_threads 0 or " +
                             std::to_string(kStepThreads) + ", reset_threads 0 or " + std::to_string(kResetThreads) + ")");
  }
  if (h->plan.opt_in_lds) {   // large worlds only: the generic instances (the default geometry needs 33 KB)
    std::vector<const void*> big;
#define CRAFTER_X(id, LM, GEO, RUL) \
    if constexpr (GEO != 1) big.push_back((const void*)crafter_step_kernel<LM, GEO, RUL>);
    CRAFTER_STEP_INSTANCES(CRAFTER_X)
#undef CRAFTER_X
    for (const void* f : {(const void*)crafter_reset_kernel, (const void*)crafter_reset_worlds_kernel, (const void*)crafter_gen_resolve_kernel<0>,
                          (const void*)crafter_requeue_reset_kernel, (const void*)crafter_requeue_final_kernel,
                          (const void*)crafter_render_kernel})
      big.push_back(f);
    hipError_t er = rollout_allow_lds(h->plan.render_lds);   // the rollout kernels live in crafter_rollout.hip
    if (er != hipSuccess) {
      std::string msg = std::string("crafter_create: hipFuncSetAttribute(rollout kernels): ") + hipGetErrorString(er);
      delete h;
      return fail(nullptr, msg);
    }
    er = subset_allow_lds(h->plan.render_lds);   // ... and crafter_step_envs' in crafter_subset.hip
    if (er != hipSuccess) {
      std::string msg = std::string("crafter_create: hipFuncSetAttribute(subset kernels): ") + hipGetErrorString(er);
      delete h;
      return fail(nullptr, msg);
    }
    er = rollout_envs_allow_lds(h->plan.render_lds);   // ... and crafter_step_n_envs' in crafter_rollout_subset.hip
    if (er != hipSuccess) {
      std::string msg = std::string("crafter_create: hipFuncSetAttribute(subset rollout kernels): ") + hipGetErrorString(er);
      delete h;
      return fail(nullptr, msg);
    }
    for (const void* f : big) {
      hipError_t ea = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, h->plan.render_lds);
      if (ea != hipSuccess) {
        std::string msg = std::string("crafter_create: hipFuncSetAttribute(MaxDynamicSharedMemorySize, ") +
                          std::to_string(h->plan.render_lds) + "): " + hipGetErrorString(ea);
        delete h;
        return fail(nullptr, msg);
      }
    }
  }
  {   // dispatch order (see crafter_handle::order).  CRAFTER_ORDER=0 / 1: never / whenever possible (A/B)
    const char* v = getenv("CRAFTER_ORDER");
    if (keeps_dispatch_order(c.num_envs, v ? atoi(v) : -1)) {
      hipError_t ea = hipMalloc((void**)&h->order, 2 * (size_t)c.num_envs * sizeof(int32_t));
      if (ea == hipSuccess) ea = hipMalloc((void**)&h->next_step, (size_t)c.num_envs * sizeof(int32_t));
      if (ea == hipSuccess) ea = hipMemset(h->next_step, 0, (size_t)c.num_envs * sizeof(int32_t));
      if (ea != hipSuccess) {
        std::string msg = std::string("crafter_create: dispatch order buffers: ") + hipGetErrorString(ea);
        delete h;
        return fail(nullptr, msg);
      }
      h->owned.push_back(h->order);
      h->owned.push_back(h->next_step);
    }
  }
  if (c.auto_reset) {   // (a failure here only costs the overlap: the regeneration kernel then stays on the launch stream)
    if (hipStreamCreateWithFlags(&h->aux, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_rules, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_requeue, hipEventDisableTiming) != hipSuccess) {
      if (h->aux) (void)hipStreamDestroy(h->aux);
      h->aux = nullptr;
    }
  }
  if (c.auto_reset && c.gen_period >= 0) {
    h->pool = true;
    h->gen_period = c.gen_period > 0 ? c.gen_period : kDefaultGenPeriod;
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);   // lo = least priority: generation yields to stepping
    bool ok = hipEventCreateWithFlags(&h->ev_main, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < kGenStreams && ok; i++)
      ok = hipStreamCreateWithPriority(&h->side[i], hipStreamNonBlocking, lo) == hipSuccess;
    for (int i = 0; i < kGenRing && ok; i++)
      ok = hipEventCreateWithFlags(&h->ev_gen[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
      delete h;
      return fail(nullptr, "crafter_create: cannot create the world-pool stream / events");
    }
  }
  *out = h;
  return 0;
}

void crafter_destroy(crafter_handle* h) {
  if (!h) return;
  for (int i = 0; i < kGenStreams; i++)
    if (h->side[i]) {
      (void)hipStreamSynchronize(h->side[i]);
      (void)hipStreamDestroy(h->side[i]);
    }
  if (h->aux) {
    (void)hipStreamSynchronize(h->aux);
    (void)hipStreamDestroy(h->aux);
  }
  if (h->ev_rules) (void)hipEventDestroy(h->ev_rules);
  if (h->ev_requeue) (void)hipEventDestroy(h->ev_requeue);
  if (h->ev_main) (void)hipEventDestroy(h->ev_main);
  if (h->ev_switch) (void)hipEventDestroy(h->ev_switch);
  for (int i = 0; i < kGenRing; i++)
    if (h->ev_gen[i]) (void)hipEventDestroy(h->ev_gen[i]);
  for (void* p : h->owned) (void)hipFree(p);
  if (!h->shared_block_key.empty()) {
    std::lock_guard<std::mutex> lock(g_blocks_mutex);
    auto it = g_blocks.find(h->shared_block_key);
    if (it != g_blocks.end() && --it->second.refs == 0) {
      (void)hipFree(it->second.ptr);
      g_blocks.erase(it);
    }
  }
  for (hipEvent_t ev : h->events)
    if (ev) (void)hipEventDestroy(ev);
  delete h;
}

static int upload(crafter_handle* h, const void* src, size_t bytes, const void** dst) {
  void* d = nullptr;
  if (bytes == 0) bytes = 16;
  hipError_t e = hipMalloc(&d, bytes);
  if (e != hipSuccess) return hip_fail(h, "hipMalloc(tables)", e);
  h->owned.push_back(d);
  if (src) {
    e = hipMemcpy(d, src, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(h, "hipMemcpy(tables)", e);
  }
  *dst = d;
  return 0;
}

int crafter_upload_tables(crafter_handle* h, const crafter_host_tables* t) {
  if (!h || !t) return fail(h, "crafter_upload_tables: null argument");
  if (h->have_tables) return fail(h, "crafter_upload_tables: tables already uploaded");
  const Config& c = h->cfg;
  if (t->n_tex_tile != TEX_COUNT || t->n_tex_icon != MAX_ITEMS || t->n_tex_digit != 11 ||
      t->n_tex_alpha != TEX_COUNT + MAX_ITEMS + 11 || t->n_item_pos != MAX_ITEMS * 4 || t->n_unit255 != 256)
    return fail(h, "crafter_upload_tables: table sizes do not match crafter_hip_types.h");
  if (t->n_daylight != c.n_daylight) return fail(h, "crafter_upload_tables: daylight table size != cfg.n_daylight");
  if (t->n_daylight >= (1 << 24)) return fail(h, "crafter_upload_tables: more than 2^24 - 1 steps per episode");   // (the step kernels keep the step counter in 24 bits of an LDS word)
  if (t->n_vignette != c.local_gw * c.unit_x * c.local_gh * c.unit_y)
    return fail(h, "crafter_upload_tables: vignette size != LocalView canvas");
  const Rules* r = t->rules;
  if (r->n_items > MAX_ITEMS || r->n_achievements > MAX_ACH || r->n_actions > MAX_ACTIONS ||
      r->n_materials >= MAX_MATERIALS)
    return fail(h, "crafter_upload_tables: rule tables exceed compiled limits");
  if (r->n_materials + 1 > kTileRows)
    return fail(h, "crafter_upload_tables: the renderer's row table holds " + std::to_string(kTileRows - 1) + " materials (render.hpp kTileRows)");
  TablePtrs& tb = h->tb;
  if (upload(h, t->rules, sizeof(Rules), (const void**)&tb.rules)) return 1;
  const bool default_rules = is_default_rules(*r);
  if (upload(h, t->atlas, t->atlas_bytes, (const void**)&tb.atlas)) return 1;
  if (upload(h, t->tex_tile, sizeof(int32_t) * t->n_tex_tile, (const void**)&tb.tex_tile)) return 1;
  if (upload(h, t->tex_icon, sizeof(int32_t) * t->n_tex_icon, (const void**)&tb.tex_icon)) return 1;
  if (upload(h, t->tex_digit, sizeof(int32_t) * t->n_tex_digit, (const void**)&tb.tex_digit)) return 1;
  if (upload(h, t->tex_alpha, t->n_tex_alpha, (const void**)&tb.tex_alpha)) return 1;
  if (upload(h, t->item_pos, sizeof(int32_t) * t->n_item_pos, (const void**)&tb.item_pos)) return 1;
  if (upload(h, t->daylight, sizeof(double) * t->n_daylight, (const void**)&tb.daylight)) return 1;
  if (upload(h, t->vignette, sizeof(double) * t->n_vignette, (const void**)&tb.vignette)) return 1;
  if (upload(h, t->unit255, sizeof(float) * t->n_unit255, (const void**)&tb.unit255)) return 1;
  {   // the renderer's derived tables, built once on the device (TablePtrs.render_static), shared between equal handles
    int dev = 0;
    (void)hipGetDevice(&dev);
    uint64_t hash = 14695981039346656037ull;
    const int32_t geo[] = {c.unit_x, c.unit_y, c.local_gw, c.local_gh, c.item_gw, c.item_gh, c.size_w, c.size_h, c.icon_w, c.icon_h,
                           c.digit_w, c.digit_h, c.n_daylight, r->n_items, r->n_materials};
    const struct { const void* p; size_t n; } spans[] = {
        {geo, sizeof(geo)}, {t->atlas, t->atlas_bytes}, {t->tex_tile, sizeof(int32_t) * t->n_tex_tile},
        {t->tex_icon, sizeof(int32_t) * t->n_tex_icon}, {t->tex_digit, sizeof(int32_t) * t->n_tex_digit},
        {t->tex_alpha, (size_t)t->n_tex_alpha}, {t->item_pos, sizeof(int32_t) * t->n_item_pos},
        {t->daylight, sizeof(double) * t->n_daylight}, {t->vignette, sizeof(double) * t->n_vignette},
        {t->unit255, sizeof(float) * t->n_unit255}};
    uint64_t hash2 = 0x243f6a8885a308d3ull;
    for (const auto& sp : spans) {
      hash = fnv1a(hash, sp.p, sp.n);
      hash2 = mix64(hash2, sp.p, sp.n);
    }
    size_t bytes = (size_t)render_static_total_bytes(c);
    std::string key = std::to_string(dev) + "|" + std::to_string(hash) + "|" + std::to_string(hash2) + "|" + std::to_string(bytes);
    std::lock_guard<std::mutex> lock(g_blocks_mutex);
    auto it = g_blocks.find(key);
    if (it == g_blocks.end()) {
      void* blk = nullptr;
      hipError_t e = hipMalloc(&blk, bytes);
      if (e != hipSuccess) return hip_fail(h, "crafter_upload_tables: hipMalloc", e);
      hipLaunchKernelGGL(crafter_init_tables_kernel, dim3(1), dim3(kStepThreads), 0, 0, h->cfg, tb, (uint8_t*)blk);
      if (render_lit_sprite_steps(c) > 0)
        hipLaunchKernelGGL(crafter_init_lit_sprites_kernel, dim3(2 * render_lit_sprite_steps(c)), dim3(kStepThreads), 0, 0, h->cfg, tb, (uint8_t*)blk);
      e = hipDeviceSynchronize();
      if (e != hipSuccess) {
        (void)hipFree(blk);
        return hip_fail(h, "crafter_upload_tables: static render block", e);
      }
      it = g_blocks.emplace(key, SharedBlock{blk, 0}).first;
    }
    it->second.refs++;
    h->shared_block_key = key;
    tb.render_static = (const uint8_t*)it->second.ptr;
  }
  h->plan = launch_plan(c, default_rules, h->lds_pad, h->rollout_lds_pad);   // the rules are known: the instance may be a compiled-in one
  h->have_tables = true;
  return 0;
}

// Episodes without a time limit (Env(length=None), env.py:29,103): the table of _update_time's values (env.py:135-139) is
// finite and the host evaluates it; this hands over a longer one.  Launches already in their queues keep the table (and
// the size) they were launched with, so nothing is waited for; the old table is freed with the handle.
int crafter_extend_daylight(crafter_handle* h, const double* daylight, int32_t n) {
  if (!h || !daylight) return fail(h, "crafter_extend_daylight: null argument");
  if (!h->have_tables) return fail(h, "crafter_extend_daylight: no tables uploaded yet");
  if (n <= h->cfg.n_daylight) return fail(h, "crafter_extend_daylight: the new table must be longer than the current one");
  if (n >= (1 << 24)) return fail(h, "crafter_extend_daylight: more than 2^24 - 1 steps per episode");
  if (h->cfg.n_daylight < kLitSteps)   // (the renderer's static block is laid out for min(n_daylight, kLitSteps) lit steps)
    return fail(h, "crafter_extend_daylight: a handle created with fewer than " + std::to_string(kLitSteps) + " daylight steps cannot grow");
  const void* d = nullptr;
  if (upload(h, daylight, sizeof(double) * (size_t)n, &d)) return 1;
  h->tb.daylight = (const double*)d;
  h->cfg.n_daylight = n;   // (no part of the launch plan: launch_plan.hpp)
  return 0;
}

int crafter_bind_state(crafter_handle* h, const crafter_state_ptrs* state) {
  if (!h || !state) return fail(h, "crafter_bind_state: null argument");
  const StatePtrs& s = *state;
  if (!s.mat || !s.objmap || !s.objs || !s.mt || !s.rec || !s.chunk_order || !s.chunk_seen)
    return fail(h, "crafter_bind_state: null state buffer");
  if (h->cfg.want_semantic && !s.semantic) return fail(h, "crafter_bind_state: want_semantic without a buffer");
  if (h->cfg.auto_reset && !s.reset_q) return fail(h, "crafter_bind_state: auto_reset without a reset queue");
  if (h->pool && (!s.pool_mat || !s.pool_objs || !s.pool_mt || !s.pool_hdr || !s.pool_chunk_order || !s.gen_q || !s.gen_latest || !s.pool_perm || !s.pool_census))
    return fail(h, "crafter_bind_state: world pool enabled but pool buffers missing");
  uintptr_t bits = (uintptr_t)s.mat | (uintptr_t)s.objmap | (uintptr_t)s.objs | (uintptr_t)s.mt | (uintptr_t)s.rec;
  if (bits & 15) return fail(h, "crafter_bind_state: state buffers must be 16-byte aligned");
  h->st = s;
  h->have_state = true;
  return 0;
}

int32_t crafter_lds_bytes(const crafter_handle* h) { return h ? h->plan.step_lds : -1; }

int32_t crafter_slot_map_derived(const crafter_handle* h) { return h ? h->plan.maps_in_lds : -1; }

int32_t crafter_step_instance(const crafter_handle* h) { return h ? h->plan.instance : -1; }

static int ready(crafter_handle* h, const char* who) {
  if (!h) return fail(nullptr, std::string(who) + ": null handle");
  if (!h->have_tables) return fail(h, std::string(who) + ": crafter_upload_tables not called");
  if (!h->have_state) return fail(h, std::string(who) + ": crafter_bind_state not called");
  return 0;
}

// World-pool scheduler, once per crafter_step (after the step's kernels are enqueued).  Any HIP failure here
// disables the pool for good (pool_failed): worlds of batches <= safe_seq stay valid, nothing newer is ever
// trusted, finished envs regenerate inline (gen_parity = -1 in StepCtl) -- slower, never wrong.
static void pool_fail(crafter_handle* h, const char* what, hipError_t e) {
  h->pool_failed = true;
  h->pool_err = std::string("world pool disabled (") + what + ": " + hipGetErrorString(e) + "); finished envs regenerate inline";
}

// Trust in batches polled_seq + 1 .. safe_seq rests on hipStreamWaitEvent calls enqueued on ONE stream (safe_stream).  The
// header only asks the caller to serialise the calls on a handle, not to keep to one stream: a call that arrives on
// another stream gets the same waits before any of its kernels is enqueued (a reset() under
// torch.cuda.stream(s) followed by step() on another stream trusted batches that stream had never waited for).
static void pool_adopt_stream(crafter_handle* h, hipStream_t stream) {
  if (!h->pool || h->pool_failed) return;
  if (h->have_safe_stream && h->safe_stream == stream) return;
  if (h->have_safe_stream)
    for (uint32_t s = (h->safe_seq > h->polled_seq + kGenRing ? h->safe_seq - kGenRing : h->polled_seq) + 1; s <= h->safe_seq; s++) {
      // (an event slot older than the ring has been recorded again by a later batch of the same side stream: waiting for
      // that one is waiting for more)
      hipError_t ew = hipStreamWaitEvent(stream, h->ev_gen[s % kGenRing], 0);
      if (ew != hipSuccess) {
        pool_fail(h, "hipStreamWaitEvent(new launch stream)", ew);
        h->safe_seq = h->polled_seq;
        break;
      }
    }
  h->safe_stream = stream;
  h->have_safe_stream = true;
}

// Every entry point that enqueues kernels takes the caller's stream.  The header promises that a caller who changes streams
// between calls need not order them himself: the new stream waits for whatever the handle still has in flight on the
// previous one (an event recorded there) -- whether or not the world pool runs (crafter_reset on stream A followed
// by crafter_step on stream B raced the reset kernel) -- and then for the pool batches the old stream had been ordered behind.
static int adopt_stream(crafter_handle* h, hipStream_t stream) {
  if (h->have_last_stream && h->last_stream != stream) {
    if (!h->ev_switch) {
      hipError_t ec = hipEventCreateWithFlags(&h->ev_switch, hipEventDisableTiming);
      if (ec != hipSuccess) return hip_fail(h, "stream change: hipEventCreate", ec);
    }
    hipError_t e = hipEventRecord(h->ev_switch, h->last_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(stream, h->ev_switch, 0);
    if (e != hipSuccess) {
      // The previous stream may be gone (a C caller may destroy a stream once its work is done -- ADVICE r5: the failed record
      // used to leave last_stream pointing at it, and every later call failed the same way).  Everything the handle enqueued
      // there is then ordered the blunt way, once, and the handle moves on to the new stream.
      (void)hipGetLastError();
      hipError_t es = hipDeviceSynchronize();
      if (es != hipSuccess) return hip_fail(h, "stream change: ordering the new stream behind the previous one", es);
    }
  }
  h->last_stream = stream;
  h->have_last_stream = true;
  pool_adopt_stream(h, stream);
  return 0;
}

// main_recorded: ev_main already marks the point of the launch stream the batch has to wait for (crafter_step_n: it is the
// stop event of the stretch's last kernel -- that kernel's own completion signal instead of a marker packet of its own
// behind it: every packet between two dependent kernels costs the launch stream 4-5 us here, profiles/r5_rollout_gaps.txt)
static void pool_schedule(crafter_handle* h, hipStream_t main, int steps = 1, bool main_recorded = false, bool behind_rollout = false) {
  // 1. trust: batches complete in launch order per stream but the two streams interleave, so poll in sequence order
  while (h->polled_seq < h->batches) {
    hipError_t q = hipEventQuery(h->ev_gen[(h->polled_seq + 1) % kGenRing]);
    if (q == hipSuccess) {
      h->polled_seq++;
      if (h->safe_seq < h->polled_seq) h->safe_seq = h->polled_seq;
    } else if (q == hipErrorNotReady) {
      break;
    } else {
      return pool_fail(h, "hipEventQuery", q);
    }
  }
  h->steps_since_gen += steps;
  if (h->steps_since_gen < h->gen_period) return;
  // 2. back-pressure: order the launch stream behind batch seq - kGenLag (no host wait).  This also covers the reuse
  //    of queue segment / event slot seq % kGenRing, last used by batch seq - kGenRing + 1 <= seq - kGenLag.
  uint32_t seq = h->batches + 1;
  if (seq > (uint32_t)h->gen_lag + 1 && h->safe_seq < seq - h->gen_lag) {
    uint32_t t = seq - h->gen_lag;
    hipError_t ew = hipStreamWaitEvent(main, h->ev_gen[t % kGenRing], 0);
    if (ew != hipSuccess) return pool_fail(h, "hipStreamWaitEvent(launch stream)", ew);
    h->safe_seq = t;   // steps enqueued from now on run after batch t
  }
  // 3. launch batch `seq` over the segment that has been collecting
  hipStream_t side = h->side[seq % kGenStreams];
  hipError_t e = main_recorded ? hipSuccess : hipEventRecord(h->ev_main, main);
  if (e != hipSuccess) return pool_fail(h, "hipEventRecord(launch stream)", e);
  e = hipStreamWaitEvent(side, h->ev_main, 0);
  if (e != hipSuccess) return pool_fail(h, "hipStreamWaitEvent(generation stream)", e);
  // (Consecutive batches run side by side on the two streams.  They never write the same pool entry: a request whose
  // entry still has an older generation on its way is put off on the device, request_generation / PoolHdr.pending.)
  int seg = h->gen_parity;
  int n = h->cfg.num_envs;
  // Wave priority of the batch's two one-wave-per-world kernels (seeding, ordered draws: a few hundred waves whose serial
  // chain is the batch's latency; the classification in between stays at 0).  Behind a rollout stretch 2: the launch
  // stream of an open loop runs far ahead of the host's polling, every stretch waits for batch seq - 3 on the device, and
  // on every second stretch that wait was a real one (profiles/r5_rollout_gaps.txt): open loop 74.5-74.9 -> 75.6-75.9 M.
  // Behind a closed-loop step 1 (round 6; 0 until then: priority 2 costs the 64x64 loop 0.5 %, 64.7 -> 64.4 M): the ordered draws of
  // a 256x256 world are a 7 ms chain, and BASELINE configs[3] -- bound by its generator -- runs at 15.05-15.12 M env-steps/s with it
  // against 14.25-14.59 M (profiles/r6_cfg4_prio.txt; 2 and 3: the same); the 64x64 loop's 20-step window gains 1.5 %, its
  // steady state loses 0.2 % (profiles/r6_headline_prio.txt).
  const int prio = h->gen_serial_prio >= 0 ? h->gen_serial_prio : (behind_rollout ? 2 : 1);
  const int cgrid = behind_rollout ? h->classify_grid : h->classify_grid_step;
  dim3 gs(n < kGenSerialGrid ? n : kGenSerialGrid), gc((long long)n * gen_classify_parts(h->cfg) < cgrid ? n * gen_classify_parts(h->cfg) : cgrid);
#ifdef CRAFTER_PROBES
  if (h->probe_free_gen) {   // timing probe: see crafter_gen_stamp_kernel
    if (h->probe_free_gen == 2) {   // ... behind workgroups that occupy what the three kernels occupy, for as long (profiles/r5_kernel_stats.csv)
      const int worlds = h->probe_worlds > 0 ? h->probe_worlds : 390;
      int ws = worlds < (int)gs.x ? worlds : (int)gs.x, wc = worlds * gen_classify_parts(h->cfg) < (int)gc.x ? worlds * gen_classify_parts(h->cfg) : (int)gc.x;
      const int l0 = h->probe_lds[0] >= 0 ? h->probe_lds[0] : kGenSeedLds, l1 = h->probe_lds[1] >= 0 ? h->probe_lds[1] : gen_classify_lds_bytes(h->cfg),
                l2 = h->probe_lds[2] >= 0 ? h->probe_lds[2] : h->gen_resolve_lds_bytes;
      if (h->probe_big) {
        hipLaunchKernelGGL(crafter_gen_occupy_kernel<0>, dim3(ws), dim3(kGenSeedThreads), l0, side, h->probe_us[0], worlds, (uint32_t*)nullptr);
        hipLaunchKernelGGL(crafter_gen_occupy_kernel<1>, dim3(wc), dim3(kGenClassifyThreads), l1, side, h->probe_us[1], worlds * gen_classify_parts(h->cfg), (uint32_t*)nullptr);
        hipLaunchKernelGGL(crafter_gen_occupy_kernel<1>, dim3(ws), dim3(kGenResolveThreads), l2, side, h->probe_us[2], worlds, (uint32_t*)nullptr);
      } else {
        hipLaunchKernelGGL(crafter_gen_occupy_kernel<0>, dim3(ws), dim3(kGenSeedThreads), l0, side, h->probe_us[0], worlds, (uint32_t*)nullptr);
        hipLaunchKernelGGL(crafter_gen_occupy_kernel<0>, dim3(wc), dim3(kGenClassifyThreads), l1, side, h->probe_us[1], worlds * gen_classify_parts(h->cfg), (uint32_t*)nullptr);
        hipLaunchKernelGGL(crafter_gen_occupy_kernel<0>, dim3(ws), dim3(kGenResolveThreads), l2, side, h->probe_us[2], worlds, (uint32_t*)nullptr);
      }
    }
    if (h->plan.gen_geo)
      launch_generation_stamp<1>(h, side, seg, seq);
    else
      launch_generation_stamp<0>(h, side, seg, seq);
  } else
#endif
  if (h->plan.gen_geo)
    launch_generation<1>(h, side, gs, gc, seg, seq, prio);
  else
    launch_generation<0>(h, side, gs, gc, seg, seq, prio);
  e = hipGetLastError();
  if (e != hipSuccess) return pool_fail(h, "generation kernel launch", e);
  // from here on the batch exists: the sequence number is consumed even if a later call fails (its event would then
  // never be trusted, because pool_failed stops the polling)
  h->batches = seq;
  h->steps_since_gen = 0;
  h->gen_parity = (seg + 1) % kGenRing;
  e = hipMemsetAsync(h->st.gen_q + (size_t)seg * gen_q_stride(h->cfg), 0, 16, side);
  if (e != hipSuccess) return pool_fail(h, "hipMemsetAsync(request segment)", e);
  e = hipEventRecord(h->ev_gen[seq % kGenRing], side);
  if (e != hipSuccess) return pool_fail(h, "hipEventRecord(generation stream)", e);
}

// Orders `stream` behind every launched batch (hipStreamWaitEvent: the host does not block) and trusts them all.
static void pool_wait_all(crafter_handle* h, hipStream_t stream, const char* what) {
  for (uint32_t s = h->safe_seq + 1; s <= h->batches && !h->pool_failed; s++) {
    hipError_t ew = hipStreamWaitEvent(stream, h->ev_gen[s % kGenRing], 0);
    if (ew != hipSuccess) pool_fail(h, what, ew);
  }
  if (!h->pool_failed) h->safe_seq = h->batches;
}

int crafter_reset(crafter_handle* h, const uint8_t* mask, uint8_t* obs, void* stream) {
  if (ready(h, "crafter_reset")) return 1;
  // The reset kernel generates the next episode's world into the env's pool entry itself (gen_one): it must not share
  // that entry with a generation batch still in flight on a side stream (an env reset in mid-episode k may have world
  // k + 2 in such a batch, and k + 2 lives in the entry the kernel is about to write: ADVICE r2).  So the launch stream
  // is ordered behind every launched batch first -- no host wait -- and all of them are trusted from here on.
  if (adopt_stream(h, (hipStream_t)stream)) return 1;
  if (h->pool && !h->pool_failed) pool_wait_all(h, (hipStream_t)stream, "hipStreamWaitEvent(reset)");
  hipLaunchKernelGGL(crafter_reset_kernel, dim3(h->cfg.num_envs), dim3(kResetThreads), h->plan.reset_lds,
                     (hipStream_t)stream, h->cfg, h->tb, h->st, mask, (h->pool && !h->pool_failed) ? h->gen_parity : -1, obs,
                     (const LevelTable*)h->levels);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(h, "crafter_reset launch", e);
  return 0;
}

// Env.reset into authored worlds: crafter_reset with another world source (env_worlds.hpp).  The kernel ends on the reset
// kernel's own tail (reset_pool_tail), so the launch stream is ordered behind the pool exactly as there.
int crafter_reset_worlds(crafter_handle* h, const uint8_t* mask, const int32_t* world_id, const uint8_t* bank_mat, const crafter_obj* bank_objs,
                         const int32_t* bank_nobj, const int32_t* bank_inv, int32_t n_worlds, int32_t bank_max_objects, uint8_t* obs,
                         void* stream) {
  if (ready(h, "crafter_reset_worlds")) return 1;
  if (!bank_mat || !bank_objs || !bank_nobj) return fail(h, "crafter_reset_worlds: bank_mat, bank_objs and bank_nobj must not be NULL");
  if (n_worlds < 1) return fail(h, "crafter_reset_worlds: n_worlds must be at least 1");
  if (bank_max_objects < 0) return fail(h, "crafter_reset_worlds: bank_max_objects must not be negative");
  if (((uintptr_t)bank_objs & 15u) != 0) return fail(h, "crafter_reset_worlds: bank_objs must be 16-byte aligned");
  if (adopt_stream(h, (hipStream_t)stream)) return 1;
  if (h->pool && !h->pool_failed) pool_wait_all(h, (hipStream_t)stream, "hipStreamWaitEvent(reset_worlds)");
  WorldBank bank;
  bank.world_id = world_id;
  bank.mat = bank_mat;
  bank.objs = bank_objs;
  bank.nobj = bank_nobj;
  bank.inv = bank_inv;
  bank.n_worlds = n_worlds;
  bank.max_objects = bank_max_objects;
  hipLaunchKernelGGL(crafter_reset_worlds_kernel, dim3(h->cfg.num_envs), dim3(kResetThreads), h->plan.reset_lds, (hipStream_t)stream,
                     h->cfg, h->tb, h->st, mask, bank, (h->pool && !h->pool_failed) ? h->gen_parity : -1, obs,
                     (const LevelTable*)h->levels);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(h, "crafter_reset_worlds launch", e);
  return 0;
}

// Copies of envs read and write rows of the world pool (crafter_copy_envs: the source's two entries go along; crafter_load_envs:
// the destination's entries are emptied).  Before that every pool row must be at rest, exactly as before crafter_reset: the
// segment collecting requests now is launched as a batch (no request stays queued with PoolHdr.pending set, which would block
// its entry for later requests), the launch stream is ordered behind every launched batch (hipStreamWaitEvent: the host does
// not block) and all of them are trusted.  Batches launched afterwards wait for the copy (ev_main, pool_schedule).
static void pool_quiesce(crafter_handle* h, hipStream_t stream) {
  if (!h->pool || h->pool_failed) return;
  pool_schedule(h, stream, h->gen_period);
  pool_wait_all(h, stream, "hipStreamWaitEvent(copy)");
}

// The scratch of an index check on the device (crafter_copy_check_kernel, crafter_step_envs_check_kernel): one mark per row of
// the bound state and the verdict word, allocated on first use; *stamp: this call's number in the marks, which are cleared
// only when the numbers start again.
static int index_check_scratch(crafter_handle* h, const char* who, hipStream_t stream, int32_t* stamp) {
  if (!h->copy_mark) {
    hipError_t ea = hipMalloc((void**)&h->copy_mark, ((size_t)h->cfg.num_envs + 1) * sizeof(int32_t));
    if (ea != hipSuccess) return hip_fail(h, who, ea);
    h->owned.push_back(h->copy_mark);
    h->copy_verdict = h->copy_mark + h->cfg.num_envs;
    h->copy_stamp = 0;
  }
  if (h->copy_stamp <= 0 || h->copy_stamp == 0x7fffffff) {   // first call, or the stamps wrapped: start the marks afresh
    hipError_t em = hipMemsetAsync(h->copy_mark, 0, (size_t)h->cfg.num_envs * sizeof(int32_t), stream);
    if (em != hipSuccess) return hip_fail(h, who, em);
    h->copy_stamp = 0;
  }
  *stamp = ++h->copy_stamp;
  return 0;
}

// The index check, then the copy (env_copy.hpp).  pool_rows: the pool is at rest and both sides are the bound state.
static int launch_copy(crafter_handle* h, const char* who, int mode, const CopySide& a, const CopySide& b, const int32_t* sidx,
                       const int32_t* didx, int n, hipStream_t stream, bool pool_rows) {
  CopyPlan plan;
  if (!make_copy_plan(plan, h->cfg, a, b, mode, !h->plan.maps_in_lds, (size_t)h->cfg.size_w * h->cfg.size_h * 3, pool_rows))
    return fail(h, std::string(who) + ": too many buffers for one copy plan");
  int32_t stamp = 0;
  if (index_check_scratch(h, who, stream, &stamp)) return 1;
  hipLaunchKernelGGL(crafter_copy_check_kernel, dim3(1), dim3(kCheckThreads), 0, stream, sidx, didx, n, a.rows, b.rows, mode, stamp,
                     h->copy_mark, h->copy_verdict, (EnvRec*)h->st.rec, h->cfg.num_envs);
  hipLaunchKernelGGL(crafter_copy_envs_kernel, dim3((unsigned)((long long)n * plan.parts)), dim3(kCopyThreads), 0, stream, plan, sidx,
                     didx, n, (const int32_t*)h->copy_verdict);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(h, who, e);
  return 0;
}

static int check_store(crafter_handle* h, const char* who, const crafter_state_ptrs* store, int32_t rows, int32_t max_objects) {
  if (!store || rows < 0 || max_objects < 1) return fail(h, std::string(who) + ": bad store");
  const StatePtrs& s = *store;
  if (!s.mat || !s.objs || !s.mt || !s.rec || !s.chunk_order || !s.chunk_seen || !s.census)
    return fail(h, std::string(who) + ": null store buffer");
  if (!h->plan.maps_in_lds && !s.objmap) return fail(h, std::string(who) + ": this world keeps its slot map in HBM: the store needs objmap");
  if (s.pool_mat || s.pool_hdr || s.gen_q || s.gen_latest) return fail(h, std::string(who) + ": a store holds no pool buffers or queues");
  return 0;
}

int crafter_copy_envs(crafter_handle* h, const int32_t* src, const int32_t* dst, int32_t n, uint8_t* obs, float* reward, uint8_t* done,
                      void* stream) {
  if (ready(h, "crafter_copy_envs")) return 1;
  if (n < 0 || (n > 0 && (!src || !dst))) return fail(h, "crafter_copy_envs: bad index arrays");
  if (n == 0) return 0;
  if (adopt_stream(h, (hipStream_t)stream)) return 1;
  pool_quiesce(h, (hipStream_t)stream);
  const int N = h->cfg.num_envs;
  CopySide side{&h->st, N, h->cfg.max_objects, obs, reward, done};
  return launch_copy(h, "crafter_copy_envs", COPY_WITHIN, side, side, src, dst, n, (hipStream_t)stream, h->pool && !h->pool_failed);
}

int crafter_save_envs(crafter_handle* h, const int32_t* idx, int32_t n, const uint8_t* obs, const float* reward, const uint8_t* done,
                      const crafter_state_ptrs* store, int32_t store_rows, int32_t store_max_objects, uint8_t* store_obs,
                      float* store_reward, uint8_t* store_done, void* stream) {
  if (ready(h, "crafter_save_envs")) return 1;
  if (check_store(h, "crafter_save_envs", store, store_rows, store_max_objects)) return 1;
  if (n < 0 || n > store_rows) return fail(h, "crafter_save_envs: n outside 0 .. store_rows");
  if (store_max_objects < h->cfg.max_objects) return fail(h, "crafter_save_envs: the store's slot table is narrower than the batch's");
  if (n == 0) return 0;
  if (adopt_stream(h, (hipStream_t)stream)) return 1;   // (reads live rows only: the pool's side streams never write them)
  CopySide a{&h->st, h->cfg.num_envs, h->cfg.max_objects, obs, reward, done};
  CopySide b{store, store_rows, store_max_objects, store_obs, store_reward, store_done};
  return launch_copy(h, "crafter_save_envs", COPY_SAVE, a, b, idx, nullptr, n, (hipStream_t)stream, false);
}

int crafter_load_envs(crafter_handle* h, const crafter_state_ptrs* store, int32_t store_rows, int32_t store_max_objects,
                      const uint8_t* store_obs, const float* store_reward, const uint8_t* store_done, const int32_t* rows,
                      const int32_t* idx, int32_t n, uint8_t* obs, float* reward, uint8_t* done, void* stream) {
  if (ready(h, "crafter_load_envs")) return 1;
  if (check_store(h, "crafter_load_envs", store, store_rows, store_max_objects)) return 1;
  if (n < 0 || (n > 0 && !idx)) return fail(h, "crafter_load_envs: bad index arrays");
  if (store_max_objects > h->cfg.max_objects) return fail(h, "crafter_load_envs: the store's slot table is wider than the batch's (grow the batch first)");
  if (h->cfg.want_semantic && !store->semantic) return fail(h, "crafter_load_envs: the batch keeps info['semantic'], the store does not");
  if (n == 0) return 0;
  if (adopt_stream(h, (hipStream_t)stream)) return 1;
  pool_quiesce(h, (hipStream_t)stream);
  CopySide a{store, store_rows, store_max_objects, store_obs, store_reward, store_done};
  CopySide b{&h->st, h->cfg.num_envs, h->cfg.max_objects, obs, reward, done};
  return launch_copy(h, "crafter_load_envs", COPY_LOAD, a, b, rows, idx, n, (hipStream_t)stream, false);
}

// Level selection (env_levels.hpp): the named envs' next reset starts episode `episode` of lane `seed_lane`.  The kernel empties
// their pool entries, so the pool is brought to rest first, exactly as before crafter_load_envs: without that a batch in flight
// could deliver a world of the old lane into an emptied entry behind the kernel, and a queued request would keep `pending` set.
// A pool that is off or has failed is not waited for; a failed pool's entries (still bound) are emptied all the same.
int crafter_reseed(crafter_handle* h, const uint8_t* mask, const uint64_t* seed_lane, const int32_t* episode, void* stream) {
  if (ready(h, "crafter_reseed")) return 1;
  if (!seed_lane) return fail(h, "crafter_reseed: null seed_lane");
  if (adopt_stream(h, (hipStream_t)stream)) return 1;
  pool_quiesce(h, (hipStream_t)stream);
  hipLaunchKernelGGL(crafter_reseed_kernel, dim3((unsigned)((h->cfg.num_envs + kReseedThreads - 1) / kReseedThreads)), dim3(kReseedThreads), 0,
                     (hipStream_t)stream, h->cfg, h->st, mask, seed_lane, episode);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(h, "crafter_reseed launch", e);
  return 0;
}

// Level sets (env_levels.hpp).  The table lives in one handle-owned buffer of full capacity, allocated by the first call, so no
// reallocation is ever ordered against work in flight; kernels enqueued before that call got a null pointer: no table.  Every
// pooled world was generated under the table being replaced, so the pool is brought to rest as before crafter_reseed and the
// kernel empties EVERY env's entries.  With the pool off or failed (the step kernels then never adopt) only the table is written.
int crafter_set_levels(crafter_handle* h, const uint64_t* seed_lane, const int32_t* episode, const uint32_t* cum, int32_t n_levels,
                       uint64_t key, void* stream) {
  if (ready(h, "crafter_set_levels")) return 1;
  if (n_levels < 0 || n_levels > kMaxLevels) return fail(h, "crafter_set_levels: n_levels outside 0 .. " + std::to_string(kMaxLevels));
  if (n_levels > 0 && (!seed_lane || !episode)) return fail(h, "crafter_set_levels: null seed_lane / episode");
  bool fresh = false;
  if (!h->levels) {
    if (n_levels == 0) return 0;   // no table was ever set: nothing to clear
    hipError_t ea = hipMalloc((void**)&h->levels, sizeof(LevelTable));
    if (ea != hipSuccess) return hip_fail(h, "crafter_set_levels: hipMalloc", ea);
    h->owned.push_back(h->levels);
    fresh = true;
  }
  if (adopt_stream(h, (hipStream_t)stream)) return 1;
  if (fresh) {   // "no table" until the kernel below has run: the batch pool_quiesce launches (ordered behind this point of the
                 // stream, ev_main) already takes the pointer
    hipError_t em = hipMemsetAsync(h->levels, 0, offsetof(LevelTable, lane), (hipStream_t)stream);
    if (em != hipSuccess) return hip_fail(h, "crafter_set_levels: hipMemsetAsync", em);
  }
  pool_quiesce(h, (hipStream_t)stream);
  StatePtrs st = h->st;
  if (!h->pool || h->pool_failed) {
    st.pool_hdr = nullptr;
    st.gen_latest = nullptr;
  }
  const int threads = n_levels > h->cfg.num_envs ? n_levels : h->cfg.num_envs;
  hipLaunchKernelGGL(crafter_set_levels_kernel, dim3((unsigned)((threads + kLevelThreads - 1) / kLevelThreads)), dim3(kLevelThreads), 0,
                     (hipStream_t)stream, h->cfg, st, h->levels, seed_lane, episode, n_levels > 0 ? cum : nullptr, (int)n_levels, key);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(h, "crafter_set_levels launch", e);
  return 0;
}

int crafter_level_ids(crafter_handle* h, const uint8_t* mask, int32_t* ids, void* stream) {
  if (ready(h, "crafter_level_ids")) return 1;
  if (!ids) return fail(h, "crafter_level_ids: null ids");
  if (adopt_stream(h, (hipStream_t)stream)) return 1;   // (reads the records and the table only: no wait for the pool beyond that)
  hipLaunchKernelGGL(crafter_level_ids_kernel, dim3((unsigned)((h->cfg.num_envs + kLevelThreads - 1) / kLevelThreads)), dim3(kLevelThreads), 0,
                     (hipStream_t)stream, h->cfg, h->st, (const LevelTable*)h->levels, mask, ids);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(h, "crafter_level_ids launch", e);
  return 0;
}

static int requeue_grid(const crafter_handle* h, const StepCtl& ctl) {
  // With the world pool running the queue is all but always empty (0 of 68,684 resets in the benchmark): a handful of
  // workgroups finds that out faster than 256 (each needs a slot next to the resident generation workgroups).  Without
  // the pool every reset comes through here.
  int full = h->cfg.num_envs < kRequeueGrid ? h->cfg.num_envs : kRequeueGrid;
  return (ctl.gen_parity >= 0 && full > h->requeue_grid) ? h->requeue_grid : full;
}
// fin: crafter_step_final -- the step kernels ran with gen_parity = -1 and queued every finished env; the kernel that walks the
// queue draws the terminal frame first and takes worlds from the pool itself (pool_parity: the segment collecting requests,
// -1: pool off).  All of them come through here: the full grid, whatever the pool does.
static void launch_requeue(crafter_handle* h, const StepCtl& ctl, uint8_t* obs, hipStream_t stream, hipEvent_t start, hipEvent_t stop,
                           const FinalOut* fin = nullptr, int pool_parity = -1) {
  if (fin) {
    const int grid = h->cfg.num_envs < kRequeueGrid ? h->cfg.num_envs : kRequeueGrid;
    const int lds = h->plan.render_lds > h->plan.reset_lds ? h->plan.render_lds : h->plan.reset_lds;
    CRAFTER_LAUNCH(crafter_requeue_final_kernel, dim3(grid), dim3(kRequeueThreads), lds, stream, start, stop, h->cfg, h->tb, h->st, ctl.parity,
                   pool_parity, ctl.safe_seq, obs, ctl.next_step, *fin, (const LevelTable*)h->levels);
    return;
  }
  CRAFTER_LAUNCH(crafter_requeue_reset_kernel, dim3(requeue_grid(h, ctl)), dim3(kRequeueThreads), h->plan.reset_lds, stream, start, stop,
                        h->cfg, h->tb, h->st, ctl.parity, ctl.gen_parity, obs, (const LevelTable*)h->levels);
}

static int need_noise_raw(crafter_handle* h, const char* who) {
  if (h->noise_raw || !h->noise_ahead) return 0;
  hipError_t ea = hipMalloc((void**)&h->noise_raw, (size_t)h->cfg.num_envs * kNoiseStates * MT_N * sizeof(uint32_t));
  if (ea != hipSuccess) return hip_fail(h, who, ea);
  h->owned.push_back(h->noise_raw);
  return 0;
}

// the scratch a night frame's pixels wait in when the kernel's layout keeps no buffer for them in LDS (split / pipelined
// step: the frame halves; big_layout: the step kernel of large worlds), allocated on first use
static int need_night_px(crafter_handle* h, const char* who) {
  if (h->night_px) return 0;
  hipError_t ea = hipMalloc((void**)&h->night_px, (size_t)h->cfg.num_envs * frame_night_px_words(h->cfg) * 4);
  if (ea != hipSuccess) return hip_fail(h, who, ea);
  h->owned.push_back(h->night_px);
  return 0;
}

// timing mode: start / stop events attached to the kernels themselves (hipExtLaunchKernelGGL), i.e. the
// execution time a profiler reports, without the dispatch latency a hipEventRecord bracket would include
static int timing_events(crafter_handle* h, hipEvent_t ev[4], const char* who) {
  if (h->timing)
    for (int i = 0; i < 4; i++) {
      hipError_t ee = hipEventCreate(&ev[i]);
      if (ee != hipSuccess) return hip_fail(h, who, ee);
    }
  return 0;
}
static void keep_timing_events(crafter_handle* h, hipEvent_t ev[4]) {
  if (h->timing)
    for (int i = 0; i < 4; i++) h->events.push_back(ev[i]);
}

// The dispatch order of an ordered launch (crafter_handle::order; one order for crafter_step and crafter_step_n): launch k
// reads the half launch k - 1 built and builds the other.  The launch needs one block more: block 0 builds.
static void set_dispatch_order(crafter_handle* h, StepCtl& ctl) {
  uint64_t k = h->ordered_launches++;
  ctl.order = k > 0 ? h->order + (size_t)(k & 1) * h->cfg.num_envs : nullptr;
  if (h->order_override) ctl.order = h->order_override;
  ctl.order_build = h->order + (size_t)((k + 1) & 1) * h->cfg.num_envs;
  ctl.next_step = h->next_step;
}

// crafter_step_kernel<LM, GEO, RUL> of the plan's instance
static void launch_step_fused(crafter_handle* h, dim3 grid, hipStream_t stream, hipEvent_t start, hipEvent_t stop, const int32_t* actions,
                              uint8_t* obs, float* reward, uint8_t* done, const StepCtl& ctl) {
  switch (h->plan.instance) {
#define CRAFTER_X(id, LM, GEO, RUL)                                                                                              \
    case id:                                                                                                                     \
      CRAFTER_LAUNCH((crafter_step_kernel<LM, GEO, RUL>), grid, dim3(kStepThreads), h->plan.step_lds, stream, start, stop, h->cfg, \
                     h->tb, h->st, actions, obs, reward, done, ctl);                                                             \
      break;
    CRAFTER_STEP_INSTANCES(CRAFTER_X)
#undef CRAFTER_X
  }
}

// crafter_step (fin null) and crafter_step_final: one launch sequence.  With fin the step kernels see the pool as off -- every
// finished env is queued, none adopts a world or draws a frame -- and crafter_requeue_final_kernel walks the queue.
static int step_launch(crafter_handle* h, const int32_t* actions, uint8_t* obs, float* reward, uint8_t* done, void* stream,
                       const FinalOut* fin) {
  StepCtl ctl;
  const int pool_parity = (h->pool && !h->pool_failed) ? h->gen_parity : -1;
  ctl.gen_parity = fin ? -1 : pool_parity;
  ctl.safe_seq = h->safe_seq;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  const bool frames = h->cfg.render_obs != 0 && obs != nullptr;
  const bool requeue = h->cfg.auto_reset != 0;
  const StepKernel kernel = choose_step(h->plan, h->cfg.num_envs, frames, h->order != nullptr, h->split, h->wide, h->early_frame);
  const bool ordered = h->order && !is_split(kernel);   // (the wide kernel is only chosen where no order is kept)
  ctl.parity = (int)(h->steps++ & 1);   // (the reset_q halves alternate over the launches that use them)
  ctl.early_frame = step_early_frame(h->cfg.num_envs, h->early_frame);
  if (timing_events(h, ev, "crafter_step: hipEventCreate (timing mode)")) return 1;
  // the scratch the choice needs
  if (frames && !is_split(kernel)) {   // a fused step kernel draws: its night frames take their noise from states generated ahead
    if (need_noise_raw(h, "crafter_step: noise scratch")) return 1;
    ctl.noise_raw = h->noise_raw;
  }
  if (ordered) set_dispatch_order(h, ctl);
  if (kernel == kStepRulesFrame && need_night_px(h, "crafter_step: frame kernel scratch")) return 1;
  if (h->plan.night_px) {
    if (frames && need_night_px(h, "crafter_step: night frame scratch")) return 1;
    ctl.night_px = h->night_px;
  }
  const dim3 grid_n(h->cfg.num_envs + (ordered ? 1 : 0)), block_s(kStepThreads);   // (ordered: block 0 builds the next launch's order)
  // The regeneration kernel (envs that finished and found no world in the pool: all but never any) only has to sit between
  // the rules of this step and the rules of the next.  In the split step it runs BESIDE the frame kernel, on the handle's own
  // stream -- the envs it regenerates and draws are exactly those the frame kernel skips -- so its launch and the look at
  // the (empty) queue cost the launch stream nothing.
  bool beside = false;
  switch (kernel) {
    case kStepRules:   // split step: rules at wave granularity ...
      CRAFTER_LAUNCH(crafter_rules_kernel, grid_n, dim3(kRulesThreads), lane_layout(h->cfg).total, (hipStream_t)stream, ev[0], ev[1],
                     h->cfg, h->tb, h->st, actions, obs, reward, done, ctl);
      break;
    case kStepRulesFrame:   // ... then the frames
      CRAFTER_LAUNCH(crafter_rules_kernel, grid_n, dim3(kRulesThreads), lane_layout(h->cfg).total, (hipStream_t)stream, ev[0], nullptr,
                     h->cfg, h->tb, h->st, actions, obs, reward, done, ctl);
      if (requeue && h->aux) {
        hipError_t ea = hipEventRecord(h->ev_rules, (hipStream_t)stream);
        if (ea == hipSuccess) ea = hipStreamWaitEvent(h->aux, h->ev_rules, 0);
        if (ea != hipSuccess) return hip_fail(h, "crafter_step: fork to the regeneration stream", ea);
        beside = true;
        launch_requeue(h, ctl, obs, h->aux, ev[2], ev[3], fin, pool_parity);
        ea = hipEventRecord(h->ev_requeue, h->aux);
        if (ea != hipSuccess) return hip_fail(h, "crafter_step: hipEventRecord(regeneration stream)", ea);
      }
      CRAFTER_LAUNCH(crafter_frame_kernel, grid_n, block_s, frame_layout(h->cfg).total, (hipStream_t)stream, nullptr, ev[1],
                     h->cfg, h->tb, h->st, obs, h->night_px);
      if (beside) {
        hipError_t ea = hipStreamWaitEvent((hipStream_t)stream, h->ev_requeue, 0);
        if (ea != hipSuccess) return hip_fail(h, "crafter_step: join of the regeneration stream", ea);
      }
      break;
    case kStepWide:   // few envs: eight waves per env
      CRAFTER_LAUNCH(crafter_step_wide_kernel, grid_n, dim3(kWideThreads), h->plan.step_lds, (hipStream_t)stream, ev[0], ev[1],
                     h->cfg, h->tb, h->st, actions, obs, reward, done, ctl);
      break;
    case kStepEarly:   // batches larger than the chip holds at once
      CRAFTER_LAUNCH(crafter_step_early_kernel, grid_n, block_s, h->plan.step_lds, (hipStream_t)stream, ev[0], ev[1],
                     h->cfg, h->tb, h->st, actions, obs, reward, done, ctl);
      break;
    case kStepFused:
      launch_step_fused(h, grid_n, (hipStream_t)stream, ev[0], ev[1], actions, obs, reward, done, ctl);
      break;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(h, "crafter_step launch", e);
  if (requeue && !beside) launch_requeue(h, ctl, obs, (hipStream_t)stream, ev[2], ev[3], fin, pool_parity);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(h, "crafter_step (auto-reset) launch", e);
  keep_timing_events(h, ev);
  if (h->pool && !h->pool_failed) pool_schedule(h, (hipStream_t)stream);
  return 0;
}

int crafter_step(crafter_handle* h, const int32_t* actions, uint8_t* obs, float* reward, uint8_t* done,
                 void* stream) {
  if (ready(h, "crafter_step")) return 1;
  if (!actions || !reward || !done) return fail(h, "crafter_step: null argument");
  if (adopt_stream(h, (hipStream_t)stream)) return 1;
  return step_launch(h, actions, obs, reward, done, stream, nullptr);
}

int crafter_step_final(crafter_handle* h, const int32_t* actions, uint8_t* obs, float* reward, uint8_t* done,
                       uint8_t* final_obs, uint8_t* terminated, uint8_t* final_local, float* final_stats, void* stream) {
  if (ready(h, "crafter_step_final")) return 1;
  if (!actions || !reward || !done || !terminated) return fail(h, "crafter_step_final: null argument");
  if (!h->cfg.auto_reset || !h->st.reset_q)
    return fail(h, "crafter_step_final: the handle has no auto_reset (obs of crafter_step already is the final frame there)");
  const int lds = h->plan.render_lds > h->plan.reset_lds ? h->plan.render_lds : h->plan.reset_lds;
  if (symbolic_strip_bytes(h->cfg) > lds) return fail(h, "crafter_step_final: the local view is too large for the kernel's LDS");
  if (adopt_stream(h, (hipStream_t)stream)) return 1;
  FinalOut fin;
  fin.obs = h->cfg.render_obs != 0 ? final_obs : nullptr;
  fin.terminated = terminated;
  fin.local = final_local;
  fin.stats = final_stats;
  return step_launch(h, actions, obs, reward, done, stream, &fin);
}

// Env.step for the n envs idx names, and for no other: the index check (which scatters the actions to their envs' rows), then
// n workgroups of the plan's instance (crafter_subset.hip), then the regeneration kernel as behind crafter_step.  One call is
// one step to the world pool's schedule: an env steps at most once per call.
int crafter_step_envs(crafter_handle* h, const int32_t* idx, int32_t n, const int32_t* actions, uint8_t* obs, float* reward, uint8_t* done,
                      void* stream) {
  if (ready(h, "crafter_step_envs")) return 1;
  if (n < 0 || n > h->cfg.num_envs) return fail(h, "crafter_step_envs: n outside 0 .. num_envs");
  if (n == 0) return 0;
  if (!idx) return fail(h, "crafter_step_envs: null index list");
  if (!actions || !reward || !done) return fail(h, "crafter_step_envs: null argument");
  if (adopt_stream(h, (hipStream_t)stream)) return 1;
  if (!h->subset_actions) {
    hipError_t ea = hipMalloc((void**)&h->subset_actions, (size_t)h->cfg.num_envs * sizeof(int32_t));
    if (ea != hipSuccess) return hip_fail(h, "crafter_step_envs: actions scratch", ea);
    h->owned.push_back(h->subset_actions);
  }
  StepCtl ctl;
  ctl.gen_parity = (h->pool && !h->pool_failed) ? h->gen_parity : -1;
  ctl.safe_seq = h->safe_seq;
  ctl.early_frame = 0;             // (no early-frame kernel for subsets: launch_plan.hpp choose_step_envs)
  ctl.next_step = h->next_step;    // an ordered handle: the named envs' entries stay current; the launch follows no order and builds none
  const bool frames = h->cfg.render_obs != 0 && obs != nullptr;
  const StepEnvsKernel kernel = choose_step_envs(h->plan, n, frames, h->wide);
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  if (frames) {   // night frames take their noise from states generated ahead, as in crafter_step
    if (need_noise_raw(h, "crafter_step_envs: noise scratch")) return 1;
    ctl.noise_raw = h->noise_raw;
  }
  if (h->plan.night_px) {
    if (frames && need_night_px(h, "crafter_step_envs: night frame scratch")) return 1;
    ctl.night_px = h->night_px;
  }
  SubsetCheck chk;
  chk.idx = idx; chk.actions = actions; chk.n = n;
  if (index_check_scratch(h, "crafter_step_envs", (hipStream_t)stream, &chk.stamp)) return 1;
  chk.mark = h->copy_mark; chk.verdict = h->copy_verdict; chk.rec = (EnvRec*)h->st.rec; chk.rows = h->cfg.num_envs;
  chk.scattered = h->subset_actions;
  if (timing_events(h, ev, "crafter_step_envs: hipEventCreate (timing mode)")) return 1;
  ctl.parity = (int)(h->steps++ & 1);   // (the reset_q halves alternate over every launch that uses them)
  // timing mode: the step time of the call runs from the check's start to the subset kernel's end
  launch_step_envs_check(chk, (hipStream_t)stream, ev[0], nullptr);
  launch_step_subset(kernel, h->plan.instance, n, (size_t)h->plan.step_lds, (hipStream_t)stream, nullptr, ev[1], h->cfg, h->tb, h->st, idx,
                     h->copy_verdict, h->subset_actions, obs, reward, done, ctl);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(h, "crafter_step_envs launch", e);
  if (h->cfg.auto_reset != 0) launch_requeue(h, ctl, obs, (hipStream_t)stream, ev[2], ev[3]);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(h, "crafter_step_envs (auto-reset) launch", e);
  keep_timing_events(h, ev);
  if (h->pool && !h->pool_failed) pool_schedule(h, (hipStream_t)stream);
  return 0;
}

int crafter_set_timing(crafter_handle* h, int enable) {
  if (!h) return 1;
  h->timing = enable != 0;
  if (!h->timing && !h->events.empty()) {   // a caller that switches timing off without reading it: nothing is kept
    for (hipEvent_t ev : h->events) {
      if (!ev) continue;
      (void)hipEventSynchronize(ev);
      (void)hipEventDestroy(ev);
    }
    h->events.clear();
  }
  return 0;
}

int crafter_get_timing(crafter_handle* h, double* step_ms, double* reset_ms, int32_t* launches) {
  if (!h || !step_ms || !reset_ms || !launches) return fail(h, "crafter_get_timing: null argument");
  double a = 0, b = 0;
  int n = (int)h->events.size() / 4;
  for (int i = 0; i < n; i++) {
    hipEvent_t* ev = &h->events[4 * i];
    hipError_t e = hipEventSynchronize(ev[1]);
    if (e != hipSuccess) return hip_fail(h, "hipEventSynchronize", e);
    float x = 0, y = 0;
    (void)hipEventElapsedTime(&x, ev[0], ev[1]);
    a += x;
    if (h->cfg.auto_reset && ev[2] && ev[3] && hipEventSynchronize(ev[3]) == hipSuccess && hipEventElapsedTime(&y, ev[2], ev[3]) == hipSuccess) b += y;
    for (int k = 0; k < 4; k++)
      if (ev[k]) (void)hipEventDestroy(ev[k]);
  }
  (void)hipGetLastError();   // (an event pair that was never recorded -- a launch that failed half-way -- must not leave its error for the caller's next HIP call)
  h->events.clear();
  *step_ms = a;
  *reset_ms = b;
  *launches = n;
  return 0;
}

// T consecutive steps of every env in one launch per stretch between two generation batches (rollout_body): the open-loop
// form of crafter_step for policies that do not look at the observations (random, scripted, action repeat).  Outputs of
// step t at obs + t * num_envs * obs_bytes, reward + t * num_envs, done + t * num_envs; bit-identical to T calls of
// crafter_step with the same actions.
int crafter_step_n(crafter_handle* h, int32_t steps, const int32_t* actions, uint8_t* obs, float* reward, uint8_t* done,
                   void* stream) {
  if (ready(h, "crafter_step_n")) return 1;
  if (!actions || !reward || !done || steps < 1) return fail(h, "crafter_step_n: bad argument");
  if (adopt_stream(h, (hipStream_t)stream)) return 1;
  bool pooled = h->pool && !h->pool_failed;
  if (!h->stalled_at) {
    hipError_t ea = hipMalloc((void**)&h->stalled_at, (size_t)h->cfg.num_envs * sizeof(int32_t));
    if (ea != hipSuccess) return hip_fail(h, "crafter_step_n: hipMalloc", ea);
    h->owned.push_back(h->stalled_at);
  }
  const size_t n = (size_t)h->cfg.num_envs;
  const size_t obs_stride = n * (size_t)h->cfg.size_w * h->cfg.size_h * 3;
  bool requeue = h->cfg.auto_reset != 0;
  for (int done_steps = 0; done_steps < steps;) {
    int left = steps - done_steps;
    // a stretch never crosses a generation batch (requests keep their segment).  Without the pool every env that finishes
    // an episode stops in the rollout kernel and runs the REST of the stretch in the regeneration kernel, on a small grid,
    // with the generic step instance: stretches stay short there too (one launch over all T steps put nearly
    // all the work on that grid once T exceeded an episode).
    int room = pooled ? h->gen_period - h->steps_since_gen : (left < kUnpooledStretch ? left : kUnpooledStretch);
    int T = left < room ? left : (room > 0 ? room : 1);
    const int32_t* a = actions + (size_t)done_steps * n;
    uint8_t* o = obs ? obs + (size_t)done_steps * obs_stride : nullptr;
    float* r = reward + (size_t)done_steps * n;
    uint8_t* d = done + (size_t)done_steps * n;
    StepCtl ctl;
    ctl.parity = (int)(h->steps++ & 1);
    ctl.gen_parity = pooled ? h->gen_parity : -1;
    ctl.safe_seq = h->safe_seq;
    RolloutArgs ra;
    ra.T = T; ra.obs_stride = obs_stride; ra.stalled_at = h->stalled_at;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    if (timing_events(h, ev, "crafter_step_n: hipEventCreate (timing mode)")) return 1;
    if (o && h->cfg.render_obs) {
      if (need_noise_raw(h, "crafter_step_n: noise scratch")) return 1;
      ctl.noise_raw = h->noise_raw;
    }
    if (h->order && h->rollout_order) set_dispatch_order(h, ctl);   // slow envs first, as in crafter_step
    if (h->plan.night_px) {   // big_layout
      if (o && h->cfg.render_obs && need_night_px(h, "crafter_step_n: night frame scratch")) return 1;
      ctl.night_px = h->night_px;
    }
    launch_rollout(h->plan.instance, h->cfg.num_envs, (size_t)h->plan.rollout_lds, (hipStream_t)stream, ev[0], ev[1], h->cfg, h->tb, h->st,
                   a, o, r, d, ctl, ra);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(h, "crafter_step_n launch", e);
    // (a generation batch follows this stretch: its side stream waits for the stretch's last kernel through that kernel's
    // own stop event)
    const bool batch_follows = pooled && requeue && !h->timing && h->fold_main_event && h->steps_since_gen + T >= h->gen_period;
    if (requeue)
      launch_requeue_rollout(requeue_grid(h, ctl), (size_t)h->plan.render_lds, (hipStream_t)stream, ev[2], batch_follows ? h->ev_main : ev[3], h->cfg, h->tb,
                             h->st, a, o, r, d, ctl, ra, h->levels);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(h, "crafter_step_n (auto-reset) launch", e);
    keep_timing_events(h, ev);
    if (pooled) pool_schedule(h, (hipStream_t)stream, T, batch_follows, true);
    pooled = h->pool && !h->pool_failed;
    done_steps += T;
  }
  return 0;
}

// crafter_step_n for the n envs idx names, and for no other, with compact outputs (crafter_rollout_subset.hpp): the index check
// once, in front of the first stretch -- its verdict stays valid for the call's later stretches, calls on a handle being
// serialised --, then crafter_step_n's stretch loop over the subset's kernels.
int crafter_step_n_envs(crafter_handle* h, const int32_t* idx, int32_t n, int32_t steps, const int32_t* actions, uint8_t* obs, float* reward,
                        uint8_t* done, void* stream) {
  if (ready(h, "crafter_step_n_envs")) return 1;
  if (n < 0 || n > h->cfg.num_envs) return fail(h, "crafter_step_n_envs: n outside 0 .. num_envs");
  if (n == 0) return 0;
  if (!idx) return fail(h, "crafter_step_n_envs: null index list");
  if (!actions || !reward || !done || steps < 1) return fail(h, "crafter_step_n_envs: bad argument");
  if (adopt_stream(h, (hipStream_t)stream)) return 1;
  bool pooled = h->pool && !h->pool_failed;
  if (!h->stalled_at) {
    hipError_t ea = hipMalloc((void**)&h->stalled_at, (size_t)h->cfg.num_envs * sizeof(int32_t));
    if (ea != hipSuccess) return hip_fail(h, "crafter_step_n_envs: hipMalloc", ea);
    h->owned.push_back(h->stalled_at);
  }
  if (!h->rollout_row_of) {
    hipError_t ea = hipMalloc((void**)&h->rollout_row_of, (size_t)h->cfg.num_envs * sizeof(int32_t));
    if (ea != hipSuccess) return hip_fail(h, "crafter_step_n_envs: row scratch", ea);
    h->owned.push_back(h->rollout_row_of);
  }
  const bool frames = obs != nullptr && h->cfg.render_obs != 0;
  if (frames && need_noise_raw(h, "crafter_step_n_envs: noise scratch")) return 1;
  if (h->plan.night_px && frames && need_night_px(h, "crafter_step_n_envs: night frame scratch")) return 1;   // big_layout
  RolloutEnvsCheck chk;
  chk.idx = idx; chk.n = n;
  if (index_check_scratch(h, "crafter_step_n_envs", (hipStream_t)stream, &chk.stamp)) return 1;
  chk.mark = h->copy_mark; chk.verdict = h->copy_verdict; chk.rec = (EnvRec*)h->st.rec; chk.rows = h->cfg.num_envs;
  chk.row_of = h->rollout_row_of;
  const size_t rows = (size_t)n;
  const size_t obs_stride = rows * (size_t)h->cfg.size_w * h->cfg.size_h * 3;
  const bool requeue = h->cfg.auto_reset != 0;
  for (int done_steps = 0; done_steps < steps;) {
    int left = steps - done_steps;
    // stretches as crafter_step_n's: up to the pool's next generation batch, kUnpooledStretch steps without the pool
    int room = pooled ? h->gen_period - h->steps_since_gen : (left < kUnpooledStretch ? left : kUnpooledStretch);
    int T = left < room ? left : (room > 0 ? room : 1);
    const int32_t* a = actions + (size_t)done_steps * rows;
    uint8_t* o = obs ? obs + (size_t)done_steps * obs_stride : nullptr;
    float* r = reward + (size_t)done_steps * rows;
    uint8_t* d = done + (size_t)done_steps * rows;
    StepCtl ctl;
    ctl.parity = (int)(h->steps++ & 1);
    ctl.gen_parity = pooled ? h->gen_parity : -1;
    ctl.safe_seq = h->safe_seq;
    ctl.next_step = h->next_step;   // an ordered handle: the named envs' entries stay current; the launch follows no order and builds none
    if (frames) ctl.noise_raw = h->noise_raw;
    if (h->plan.night_px) ctl.night_px = h->night_px;
    RolloutEnvsArgs ra;
    ra.idx = idx; ra.verdict = h->copy_verdict; ra.row_of = h->rollout_row_of; ra.n = n; ra.T = T; ra.stalled_at = h->stalled_at;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    if (timing_events(h, ev, "crafter_step_n_envs: hipEventCreate (timing mode)")) return 1;
    // timing mode: the first stretch's step time runs from the check's start to the rollout kernel's end
    if (done_steps == 0) launch_rollout_envs_check(chk, (hipStream_t)stream, ev[0], nullptr);
    launch_rollout_envs(h->plan.instance, (size_t)h->plan.rollout_lds, (hipStream_t)stream, done_steps == 0 ? nullptr : ev[0], ev[1], h->cfg, h->tb,
                        h->st, a, o, r, d, ctl, ra);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(h, "crafter_step_n_envs launch", e);
    // (a generation batch follows this stretch: its side stream waits for the stretch's last kernel through that kernel's
    // own stop event, as in crafter_step_n)
    const bool batch_follows = pooled && requeue && !h->timing && h->fold_main_event && h->steps_since_gen + T >= h->gen_period;
    if (requeue)
      launch_requeue_rollout_envs(requeue_grid(h, ctl), (size_t)h->plan.render_lds, (hipStream_t)stream, ev[2], batch_follows ? h->ev_main : ev[3],
                                  h->cfg, h->tb, h->st, a, o, r, d, ctl, ra, h->levels);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(h, "crafter_step_n_envs (auto-reset) launch", e);
    keep_timing_events(h, ev);
    if (pooled) pool_schedule(h, (hipStream_t)stream, T, batch_follows, true);
    pooled = h->pool && !h->pool_failed;
    done_steps += T;
  }
  return 0;
}

// Diagnostics / experiments: the next crafter_step calls dispatch the envs in this order (device int32[num_envs], a
// permutation -- not checked; the caller keeps it alive) instead of the one the library builds; NULL: back to its own.
int crafter_debug_set_dispatch_order(crafter_handle* h, const int32_t* order) {
  if (ready(h, "crafter_debug_set_dispatch_order")) return 1;
  if (!h->order) return 2;
  if (order) {   // two workgroups stepping one env would corrupt it: checked here, once (a diagnostic call: the copy synchronises)
    std::vector<int32_t> host((size_t)h->cfg.num_envs);
    hipError_t e = hipMemcpy(host.data(), order, host.size() * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(h, "crafter_debug_set_dispatch_order", e);
    std::vector<uint8_t> seen(host.size(), 0);
    for (int32_t v : host) {
      if (v < 0 || v >= h->cfg.num_envs || seen[(size_t)v]) return fail(h, "crafter_debug_set_dispatch_order: not a permutation of the env indices");
      seen[(size_t)v] = 1;
    }
  }
  h->order_override = order;
  return 0;
}

// Diagnostics: the dispatch order the next crafter_step will use (host int32[num_envs]; synchronises the device).
// Returns 2 when this handle keeps none (see crafter_handle::order).
int crafter_debug_dispatch_order(crafter_handle* h, int32_t* out) {
  if (ready(h, "crafter_debug_dispatch_order")) return 1;
  if (!out) return fail(h, "crafter_debug_dispatch_order: null argument");
  if (!h->order || h->ordered_launches == 0) return 2;
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess)
    e = hipMemcpy(out, h->order + (size_t)(h->ordered_launches & 1) * h->cfg.num_envs, (size_t)h->cfg.num_envs * sizeof(int32_t),
                  hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hip_fail(h, "crafter_debug_dispatch_order", e);
  return 0;
}

int crafter_render(crafter_handle* h, const uint8_t* mask, uint8_t* out, void* stream) {
  if (ready(h, "crafter_render")) return 1;
  if (!out) return fail(h, "crafter_render: null output");
  if (adopt_stream(h, (hipStream_t)stream)) return 1;
  hipLaunchKernelGGL(crafter_render_kernel, dim3(h->cfg.num_envs), dim3(kStepThreads), h->plan.render_lds,
                     (hipStream_t)stream, h->cfg, h->tb, h->st, mask, out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(h, "crafter_render launch", e);
  return 0;
}

// The symbolic observation of the state as it stands on `stream` (symbolic.hpp).  Reads live rows only -- the pool's side
// streams never write them -- so, like crafter_save_envs, it waits for no batch.
int crafter_symbolic(crafter_handle* h, const uint8_t* mask, uint8_t* local, float* stats, void* stream) {
  if (ready(h, "crafter_symbolic")) return 1;
  if (!local && !stats) return 0;
  const int lds = kSymbolicEnvs * symbolic_strip_bytes(h->cfg);
  if (lds > 64 * 1024) return fail(h, "crafter_symbolic: the local view is too large for the kernel's LDS strips");
  if (adopt_stream(h, (hipStream_t)stream)) return 1;
  const dim3 grid((unsigned)((h->cfg.num_envs + kSymbolicEnvs - 1) / kSymbolicEnvs)), block(kSymbolicThreads);
  if (h->plan.maps_in_lds)
    hipLaunchKernelGGL(crafter_symbolic_kernel<0>, grid, block, lds, (hipStream_t)stream, h->cfg, h->tb, h->st, mask, local, stats,
                       symbolic_strip_bytes(h->cfg));
  else
    hipLaunchKernelGGL(crafter_symbolic_kernel<1>, grid, block, lds, (hipStream_t)stream, h->cfg, h->tb, h->st, mask, local, stats,
                       symbolic_strip_bytes(h->cfg));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(h, "crafter_symbolic launch", e);
  return 0;
}

// The legal-action mask of the state as it stands on `stream` (legal.hpp).  Like crafter_symbolic it reads live rows only and
// waits for no batch of the pool.
int crafter_legal_actions(crafter_handle* h, const uint8_t* mask, uint8_t* legal, void* stream) {
  if (ready(h, "crafter_legal_actions")) return 1;
  if (!legal) return fail(h, "crafter_legal_actions: null output");
  if (adopt_stream(h, (hipStream_t)stream)) return 1;
  const dim3 grid((unsigned)((h->cfg.num_envs + kLegalEnvs - 1) / kLegalEnvs)), block(kLegalThreads);
  if (h->plan.maps_in_lds)
    hipLaunchKernelGGL(crafter_legal_actions_kernel<0>, grid, block, 0, (hipStream_t)stream, h->cfg, h->tb, h->st, mask, legal);
  else
    hipLaunchKernelGGL(crafter_legal_actions_kernel<1>, grid, block, 0, (hipStream_t)stream, h->cfg, h->tb, h->st, mask, legal);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(h, "crafter_legal_actions launch", e);
  return 0;
}

#ifdef CRAFTER_PROBES
// probe builds: the generation kernels' phase clocks (env_kernels.hpp g_gen_probe), read and cleared; synchronises the device
int crafter_debug_gen_probe(uint64_t out[32]) {
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_gen_probe), 32 * sizeof(uint64_t)) != hipSuccess) return 1;
  uint64_t zero[32] = {0};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_gen_probe), zero, sizeof(zero)) == hipSuccess ? 0 : 1;
}
#endif

int crafter_pool_status(const crafter_handle* h, uint32_t* launched, uint32_t* trusted) {
  if (!h) return -1;
  if (launched) *launched = h->batches;
  if (trusted) *trusted = h->safe_seq;
  return !h->pool ? 0 : h->pool_failed ? 2 : 1;
}

const char* crafter_pool_error(const crafter_handle* h) { return h ? h->pool_err.c_str() : ""; }

int crafter_debug_eval(int mode, const uint8_t* perm, const double* x, const double* y, const double* z, double* out,
                       int64_t n, void* stream) {
  if (mode < 0 || mode > 3 || !x || !out || n < 0 || (mode == 0 && (!perm || !y || !z)))
    return fail(nullptr, "crafter_debug_eval: bad argument");
  if (n == 0) return 0;
  long long blocks = (n + kStepThreads - 1) / kStepThreads;
  hipLaunchKernelGGL(crafter_debug_eval_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(kStepThreads), 512 + kSimplexLdsBytes, (hipStream_t)stream,
                     perm, x, y, z, out, (long long)n, mode);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(nullptr, "crafter_debug_eval launch", e);
  return 0;
}

const char* crafter_last_error(const crafter_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Multi-GPU: the per-step exchange the north star names ("RCCL gather of obs / reward / done over xGMI"), enqueued from C.
// Through torch.distributed one step of an N > 1 run costs the host 49-72 us of Python (begin + step(out=) + all_gather
// launch + result) against 26-31 us of GPU at one GPU's share of configs[2] (512 envs): host-bound before a byte has
// crossed xGMI (round 4).  Here ONE call enqueues the step kernels -- writing straight into the packed send record -- and
// the all-gather of that record, on a stream of the exchange's own behind an event, so that it overlaps the next step.
// RCCL is bound at run time (dlopen: the library torch already loaded, or ROCm's): libcrafter_hip.so itself links no
// communication library, and a single-GPU user never touches this code.
#include <dlfcn.h>

namespace {
struct NcclId { char internal[128]; };
typedef void* NcclComm;
struct Rccl {
  int (*GetUniqueId)(NcclId*) = nullptr;
  int (*CommInitRank)(NcclComm*, int, NcclId, int) = nullptr;
  int (*CommDestroy)(NcclComm) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, NcclComm, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  std::string err;
  bool ok = false;
};
Rccl& rccl() {
  static Rccl r;
  static std::once_flag once;
  std::call_once(once, [] {
    // The copy the process has loaded ALREADY comes first (torch.distributed's "nccl" backend brings its own librccl: a second
    // copy next to it would be a second set of the library's global state -- ADVICE r5); only then a search by name / path.
    void* lib = nullptr;
    for (const char* name : {"librccl.so.1", "librccl.so"}) {
      lib = dlopen(name, RTLD_NOW | RTLD_NOLOAD);
      if (lib) break;
    }
    if (!lib)
      for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
        lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (lib) break;
      }
    if (!lib) {
      r.err = std::string("RCCL not found (dlopen librccl.so): ") + (dlerror() ? dlerror() : "");
      return;
    }
    r.GetUniqueId = (int (*)(NcclId*))dlsym(lib, "ncclGetUniqueId");
    r.CommInitRank = (int (*)(NcclComm*, int, NcclId, int))dlsym(lib, "ncclCommInitRank");
    r.CommDestroy = (int (*)(NcclComm))dlsym(lib, "ncclCommDestroy");
    r.AllGather = (int (*)(const void*, void*, size_t, int, NcclComm, hipStream_t))dlsym(lib, "ncclAllGather");
    r.GetErrorString = (const char* (*)(int))dlsym(lib, "ncclGetErrorString");
    r.ok = r.GetUniqueId && r.CommInitRank && r.CommDestroy && r.AllGather && r.GetErrorString;
    if (!r.ok) r.err = "librccl.so lacks ncclGetUniqueId / ncclCommInitRank / ncclAllGather";
  });
  return r;
}
constexpr int kNcclUint8 = 1;   // ncclUint8 (rccl.h ncclDataType_t)
constexpr int kExchangeMaxSlots = 8;
thread_local std::string g_exchange_error;
}  // namespace

struct crafter_exchange {
  NcclComm comm = nullptr;
  int rank = 0, world = 1, slots = 2;
  hipStream_t stream = nullptr;                       // the collectives run here, beside the launch stream's next step
  hipEvent_t ready[kExchangeMaxSlots] = {};           // the record of slot k is complete on the launch stream
  hipEvent_t done[kExchangeMaxSlots] = {};            // its all-gather is complete
  bool in_flight[kExchangeMaxSlots] = {};
  std::string err;
};

static int xfail(crafter_exchange* x, const std::string& msg) {
  if (x) x->err = msg; else g_exchange_error = msg;
  return 1;
}

extern "C" {

int crafter_exchange_unique_id(uint8_t id[128]) {
  Rccl& r = rccl();
  if (!r.ok) return xfail(nullptr, r.err);
  NcclId nid;
  int rc = r.GetUniqueId(&nid);
  if (rc != 0) return xfail(nullptr, std::string("ncclGetUniqueId: ") + r.GetErrorString(rc));
  memcpy(id, nid.internal, 128);
  return 0;
}

int crafter_exchange_create(const uint8_t id[128], int32_t rank, int32_t world, int32_t slots, crafter_exchange** out) {
  if (!id || !out || world < 1 || rank < 0 || rank >= world || slots < 1 || slots > kExchangeMaxSlots)
    return xfail(nullptr, "crafter_exchange_create: bad argument");
  Rccl& r = rccl();
  if (!r.ok) return xfail(nullptr, r.err);
  crafter_exchange* x = new crafter_exchange();
  x->rank = rank; x->world = world; x->slots = slots;
  NcclId nid;
  memcpy(nid.internal, id, 128);
  int rc = r.CommInitRank(&x->comm, world, nid, rank);
  if (rc != 0) {
    delete x;
    return xfail(nullptr, std::string("ncclCommInitRank: ") + r.GetErrorString(rc));
  }
  bool ok = hipStreamCreateWithFlags(&x->stream, hipStreamNonBlocking) == hipSuccess;
  for (int k = 0; k < slots && ok; k++)
    ok = hipEventCreateWithFlags(&x->ready[k], hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&x->done[k], hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    crafter_exchange_destroy(x);
    return xfail(nullptr, "crafter_exchange_create: cannot create the exchange's stream / events");
  }
  *out = x;
  return 0;
}

void crafter_exchange_destroy(crafter_exchange* x) {
  if (!x) return;
  if (x->stream) (void)hipStreamSynchronize(x->stream);
  if (x->comm) (void)rccl().CommDestroy(x->comm);
  for (int k = 0; k < kExchangeMaxSlots; k++) {
    if (x->ready[k]) (void)hipEventDestroy(x->ready[k]);
    if (x->done[k]) (void)hipEventDestroy(x->done[k]);
  }
  if (x->stream) (void)hipStreamDestroy(x->stream);
  delete x;
}

int crafter_exchange_wait(crafter_exchange* x, int32_t slot, void* stream) {
  if (!x || slot < 0 || slot >= x->slots) return xfail(x, "crafter_exchange_wait: bad argument");
  if (!x->in_flight[slot]) return 0;
  hipError_t e = hipStreamWaitEvent((hipStream_t)stream, x->done[slot], 0);
  if (e != hipSuccess) return xfail(x, std::string("crafter_exchange_wait: ") + hipGetErrorString(e));
  return 0;
}

int crafter_step_exchange(crafter_handle* h, crafter_exchange* x, int32_t slot, const int32_t* actions, uint8_t* send, uint8_t* recv,
                          int64_t record_bytes, int64_t off_reward, int64_t off_done, int32_t with_obs, void* stream) {
  if (!x || slot < 0 || slot >= x->slots || !send || !recv || record_bytes <= 0 || off_reward < 0 || off_done <= off_reward ||
      off_done >= record_bytes || (off_reward & 3))
    return xfail(x, "crafter_step_exchange: bad argument");
  if (!h) return xfail(x, "crafter_step_exchange: null env handle");
  // the slot's previous gather read `send` and wrote `recv`: the kernels that overwrite the record come behind it
  if (crafter_exchange_wait(x, slot, stream)) return 1;
  if (crafter_step(h, actions, with_obs ? send : nullptr, (float*)(send + off_reward), send + off_done, stream)) {
    x->err = std::string("crafter_step: ") + crafter_last_error(h);
    return 1;
  }
  hipError_t e = hipEventRecord(x->ready[slot], (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(x->stream, x->ready[slot], 0);
  if (e != hipSuccess) return xfail(x, std::string("crafter_step_exchange: fork to the exchange stream: ") + hipGetErrorString(e));
  Rccl& r = rccl();
  int rc = r.AllGather(send, recv, (size_t)record_bytes, kNcclUint8, x->comm, x->stream);
  if (rc != 0) return xfail(x, std::string("ncclAllGather: ") + r.GetErrorString(rc));
  e = hipEventRecord(x->done[slot], x->stream);
  if (e != hipSuccess) return xfail(x, std::string("crafter_step_exchange: hipEventRecord: ") + hipGetErrorString(e));
  x->in_flight[slot] = true;
  return 0;
}

const char* crafter_exchange_error(const crafter_exchange* x) { return x ? x->err.c_str() : g_exchange_error.c_str(); }

}  // extern "C"
