// The host state behind the C ABI of include/crafter_hip.h: the probe-knob reader, the cache of shared render blocks,
// crafter_handle, the error reporting, and one helper per idiom the entry points of crafter_hip.hip repeat.  Included by
// crafter_hip.hip only, once, behind entry_kernels.hpp (the handle's defaults are that header's launch constants).
#pragma once

namespace {

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
                                          // (env_stage.hpp noise_chain), kNoiseStates * 624 words per env; CRAFTER_NOISE_AHEAD=0: off (A/B)
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
  int n_materials = 0;                 // crafter_navigate, crafter_nearby: the uploaded rules' material count (their class sets are checked on the host)
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

static int ready(crafter_handle* h, const char* who) {
  if (!h) return fail(nullptr, std::string(who) + ": null handle");
  if (!h->have_tables) return fail(h, std::string(who) + ": crafter_upload_tables not called");
  if (!h->have_state) return fail(h, std::string(who) + ": crafter_bind_state not called");
  return 0;
}

// The close of every launch sequence: 0, or 1 with the launch error under `who`.
static int launched(crafter_handle* h, const char* who) {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : hip_fail(h, who, e);
}

// Scratch of the handle that is allocated by the first call that needs it and freed with the handle.
static int need_scratch(crafter_handle* h, void** ptr, size_t bytes, const char* who) {
  if (*ptr) return 0;
  hipError_t e = hipMalloc(ptr, bytes);
  if (e != hipSuccess) return hip_fail(h, who, e);
  h->owned.push_back(*ptr);
  return 0;
}

// the states a fused step's night frames take their noise from (crafter_handle::noise_raw; none with CRAFTER_NOISE_AHEAD=0)
static int need_noise_raw(crafter_handle* h, const char* who) {
  if (!h->noise_ahead) return 0;
  return need_scratch(h, (void**)&h->noise_raw, (size_t)h->cfg.num_envs * kNoiseStates * MT_N * sizeof(uint32_t), who);
}

// the scratch a night frame's pixels wait in when the kernel's layout keeps no buffer for them in LDS (split / pipelined
// step: the frame halves; big_layout: the step kernel of large worlds)
static int need_night_px(crafter_handle* h, const char* who) {
  return need_scratch(h, (void**)&h->night_px, (size_t)h->cfg.num_envs * frame_night_px_words(h->cfg) * 4, who);
}

// The world pool runs: kernels may adopt its worlds and queue requests.  (Off by configuration, or for good after a HIP call
// of the scheduler failed: world_pool.hpp pool_fail.)
static bool pool_live(const crafter_handle* h) { return h->pool && !h->pool_failed; }

// What every step launch is told in the same way, and the launch's number: the reset_q halves alternate over the launches
// that use them.  frames: the launch draws with a fused kernel, whose night frames take their noise from states generated
// ahead.  The caller has allocated the scratch it needs (need_noise_raw, need_night_px) before: nothing here can fail.
static StepCtl step_ctl(crafter_handle* h, bool frames) {
  StepCtl ctl;
  ctl.parity = (int)(h->steps++ & 1);
  ctl.gen_parity = pool_live(h) ? h->gen_parity : -1;
  ctl.safe_seq = h->safe_seq;
  if (frames) ctl.noise_raw = h->noise_raw;
  if (h->plan.night_px) ctl.night_px = h->night_px;
  return ctl;
}

// The kernels of this unit that crafter_create allows more LDS than the default limit, for large worlds (plan.opt_in_lds): the
// generic instances -- the default geometry needs 33 KB.  It stands here, in front of world_pool.hpp, because the compiler emits
// the unit's kernel instances in the order the host code first names them: this keeps the step kernels in front of the
// generation kernels in the code object, where they have always been.
static std::vector<const void*> big_lds_kernels() {
  std::vector<const void*> big;
#define CRAFTER_X(id, LM, GEO, RUL) \
  if constexpr (GEO != 1) big.push_back((const void*)crafter_step_kernel<LM, GEO, RUL>);
  CRAFTER_STEP_INSTANCES(CRAFTER_X)
#undef CRAFTER_X
  for (const void* f : {(const void*)crafter_reset_kernel, (const void*)crafter_reset_worlds_kernel, (const void*)crafter_gen_resolve_kernel<0>,
                        (const void*)crafter_requeue_reset_kernel, (const void*)crafter_requeue_final_kernel,
                        (const void*)crafter_render_kernel, (const void*)crafter_edit_envs_kernel})
    big.push_back(f);
  return big;
}

// LDS of crafter_requeue_final_kernel: it draws the terminal frame and resets in one workgroup.
static int final_lds(const crafter_handle* h) { return h->plan.render_lds > h->plan.reset_lds ? h->plan.render_lds : h->plan.reset_lds; }
