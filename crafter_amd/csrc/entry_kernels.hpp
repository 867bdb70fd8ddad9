// The entry kernels of libcrafter_hip.so's main unit and their launch constants: every __global__ function crafter_hip.hip
// defines, in the order the unit has always defined them.  Included by crafter_hip.hip only, once, behind the headers of the
// bodies (env_kernels.hpp ...) and `using namespace crafter`: the text lives here so that the unit itself reads as host code.
#pragma once

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

template <int LM, int GEO, int RUL>   // LM 1: maps staged in LDS, 0: large world, maps stay in HBM (env_stage.hpp bind_lds);
                                     // RUL 1: the uploaded rules equal the compiled-in kDefaultRules (types.hpp)
__global__ void __launch_bounds__(kStepThreads, step_min_waves(LM))   // (launch_plan.hpp)
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

// Split step of the default instance (step_body.hpp "Split step"): the rule half, one wave per env ...
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
// (gen_bodies.hpp gen_seed_body / gen_classify_body / gen_resolve_body).  GEO as for the step kernel.
// The queue head they open with: the segment of `parity` (pool_entry.hpp: count, 3 pad, (env, episode) pairs), its count clamped
// to the segment's capacity.
struct GenQueue {
  const int32_t* q;
  int count;
  __device__ __forceinline__ int env(int k) const { return q[4 + 2 * k]; }
  __device__ __forceinline__ int episode(int k) const { return q[4 + 2 * k + 1]; }
};
__device__ __forceinline__ GenQueue gen_queue(const Config& cfg, const StatePtrs& st, int parity) {
  const int32_t* q = st.gen_q + (size_t)parity * gen_q_stride(cfg);
  return {q, q[0] > gen_q_capacity(cfg) ? gen_q_capacity(cfg) : q[0]};
}

template <int GEO>
__global__ void __launch_bounds__(kGenSeedThreads)
crafter_gen_seed_kernel(Config cfg_in, TablePtrs tb, StatePtrs st, int parity, int prio, const LevelTable* __restrict__ levels) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  WaveGfx950<kGenSeedThreads>::set_priority(prio);   // (pool_schedule: one wave per world, a chain -- see there)
  const Config cfg = GEO ? with_default_geometry(cfg_in) : cfg_in;
  const GenQueue gq = gen_queue(cfg, st, parity);
  WaveGfx950<kGenSeedThreads> w;
  for (int k = (int)blockIdx.x; k < gq.count; k += (int)gridDim.x) {
    gen_seed_body(w, smem, gq.env(k), gq.episode(k), cfg, tb, st, levels);
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
  const GenQueue gq = gen_queue(cfg, st, parity);
  WaveGfx950<kGenClassifyThreads> w;
  const int parts = gen_classify_parts(cfg);
  for (int item = (int)blockIdx.x; item < gq.count * parts; item += (int)gridDim.x) {
    int k = item / parts;
    gen_classify_body(w, smem, gq.env(k), gq.episode(k), item - k * parts, parts, cfg, tb, st);
    __syncthreads();
  }
}

template <int GEO>
__global__ void __launch_bounds__(kGenResolveThreads)
crafter_gen_resolve_kernel(Config cfg_in, TablePtrs tb, StatePtrs st, int parity, uint32_t seq, int prio) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  WaveGfx950<kGenResolveThreads>::set_priority(prio);
  const Config cfg = GEO ? with_default_geometry(cfg_in) : cfg_in;
  const GenQueue gq = gen_queue(cfg, st, parity);
  WaveGfx950<kGenResolveThreads> w;
  for (int k = (int)blockIdx.x; k < gq.count; k += (int)gridDim.x) {
    gen_resolve_body(w, smem, gq.env(k), gq.episode(k), seq, cfg, tb, st);
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
  const GenQueue gq = gen_queue(cfg, st, parity);
  const int cells = cfg.W * cfg.H, nch = cfg.nchunk_x * cfg.nchunk_y;
  for (int k = (int)blockIdx.x; k < gq.count; k += (int)gridDim.x) {
    int env = gq.env(k), episode = gq.episode(k);
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

// crafter_fingerprint (fingerprint.hpp): one wave per env, kFingerprintEnvs envs per workgroup, no LDS and no barrier: the waves
// of the batch tail and of masked rows leave at once.  One instance: the objects are read from the slot table wherever the maps live.
__global__ void __launch_bounds__(kFingerprintThreads)
crafter_fingerprint_kernel(Config cfg, TablePtrs tb, StatePtrs st, const uint8_t* __restrict__ mask, uint32_t parts,
                           uint64_t* __restrict__ key, uint64_t* __restrict__ part_hash) {
  typedef WaveGfx950<kFingerprintThreads> WF;
  WF w;
  const int wave = WF::uni((int)(threadIdx.x >> 6));
  fingerprint_body<WF>(w, (int)blockIdx.x * kFingerprintEnvs + wave, cfg, tb, st, mask, parts, key, part_hash);
}

// crafter_navigate (navigate.hpp), worlds of at most 64 x 64 cells: one wave per env, kNavEnvs envs per workgroup, each wave with
// its own staging strip and no barrier: the waves of the batch tail and of masked rows leave at once.  MAP as for
// crafter_symbolic_kernel.  The query travels by value.  (Eight waves per SIMD, asked for: the query's words and the sweep's masks
// would otherwise take a few scalar registers more than that allows.)
template <int MAP>
__global__ void __launch_bounds__(kNavThreads, 8)
crafter_navigate_kernel(Config cfg, TablePtrs tb, StatePtrs st, const uint8_t* __restrict__ mask, NavQuery q,
                        int32_t* __restrict__ dist, int32_t* __restrict__ first, uint8_t* __restrict__ facing) {
  __shared__ uint32_t strips[kNavEnvs][kNavStripWords];
  typedef WaveGfx950<kNavThreads> WN;
  WN w;
  const int wave = WN::uni((int)(threadIdx.x >> 6));
  navigate_body<WN, MAP>(w, strips[wave], (int)blockIdx.x * kNavEnvs + wave, cfg, tb, st, mask, q, dist, first, facing);
}

// ... and any other area: one workgroup per env, the boards in nav_lds_bytes(cfg) of LDS.
template <int MAP>
__global__ void __launch_bounds__(kNavWideThreads)
crafter_navigate_lds_kernel(Config cfg, TablePtrs tb, StatePtrs st, const uint8_t* __restrict__ mask, NavQuery q,
                            int32_t* __restrict__ dist, int32_t* __restrict__ first, uint8_t* __restrict__ facing) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  WaveGfx950<kNavWideThreads> w;
  navigate_lds_body<WaveGfx950<kNavWideThreads>, MAP>(w, (uint32_t*)smem, (int)blockIdx.x, cfg, tb, st, mask, q, dist, first, facing);
}

// crafter_audit (audit.hpp): one workgroup per env, its tables in audit_lds_words(cfg) words of LDS.  NT 64 (one wave: worlds of
// at most 64 x 64 cells and 256 slots) or 256.  MAP as for crafter_symbolic_kernel.
template <int NT, int MAP>
__global__ void __launch_bounds__(NT)
crafter_audit_kernel(Config cfg, TablePtrs tb, StatePtrs st, const uint8_t* __restrict__ mask, int32_t* __restrict__ flags,
                     int32_t* __restrict__ detail) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  WaveGfx950<NT> w;
  audit_body<WaveGfx950<NT>, MAP>(w, (uint32_t*)smem, (int)blockIdx.x, cfg, tb, st, mask, flags, detail);
}

// crafter_nearby (nearby.hpp): one workgroup per env, its counters and sort keys in near_lds_words(cfg, q.k) words of LDS.  NT 64
// (one wave: worlds of at most 64 x 64 cells) or 256.  MAP as for crafter_symbolic_kernel.  The query travels by value.
template <int NT, int MAP>
__global__ void __launch_bounds__(NT)
crafter_nearby_kernel(Config cfg, TablePtrs tb, StatePtrs st, const uint8_t* __restrict__ mask, NearQuery q, int32_t* __restrict__ counts,
                      int16_t* __restrict__ ents, int32_t* __restrict__ n) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  WaveGfx950<NT> w;
  nearby_body<WaveGfx950<NT>, MAP>(w, (uint32_t*)smem, (int)blockIdx.x, cfg, tb, st, mask, q, counts, ents, n);
}

// crafter_edit_envs (env_edit.hpp): one workgroup per named env, behind the index check of crafter_step_n_envs (a refused list:
// every workgroup leaves at once, no row changes).  Workgroup b replays row b of the tape on env idx[b].
__global__ void __launch_bounds__(kEditThreads)
crafter_edit_envs_kernel(Config cfg, TablePtrs tb, StatePtrs st, const int32_t* __restrict__ idx, const int32_t* __restrict__ verdict,
                         const int32_t* __restrict__ ops, int ops_per_env, int32_t* __restrict__ next_step) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int env = step_envs_env(idx, verdict, (int)blockIdx.x);
  if (env < 0) return;
  WaveGfx950<kEditThreads> w;
  edit_body(w, smem, env, cfg, tb, st, ops + (size_t)blockIdx.x * (size_t)ops_per_env * kEditWords, ops_per_env, next_step);
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

}  // namespace
