// libcrafter_hip.so: gfx950 kernels + the C ABI of include/crafter_hip.h.  This unit defines the entry kernels
// (entry_kernels.hpp) and holds every extern "C" entry point but the RCCL exchange's (crafter_exchange.hip), with the launch
// helpers only they use; the handle and the helpers of the repeated idioms are handle.hpp's, the world pool's scheduler
// world_pool.hpp's.
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
#include "../../include/crafter_hip_audit.h"
#include "../../include/crafter_hip_edit.h"
#include "../../include/crafter_hip_fingerprint.h"
#include "../../include/crafter_hip_navigate.h"
#include "../../include/crafter_hip_nearby.h"
#include "audit.hpp"
#include "crafter_rollout.hpp"
#include "crafter_rollout_subset.hpp"
#include "crafter_subset.hpp"
#include "dispatch_order.hpp"
#include "env_copy.hpp"
#include "env_edit.hpp"
#include "env_kernels.hpp"
#include "env_levels.hpp"
#include "env_worlds.hpp"
#include "fingerprint.hpp"
#include "launch_plan.hpp"
#include "legal.hpp"
#include "navigate.hpp"
#include "nearby.hpp"
#include "symbolic.hpp"
#include "wave_gfx950.hpp"

using namespace crafter;

#include "entry_kernels.hpp"
#include "handle.hpp"
#include "world_pool.hpp"

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

// The one exit of crafter_create once the handle exists: crafter_destroy frees whatever it owns by then (buffers, streams, events).
static int create_fail(crafter_handle* h, const std::string& msg) {
  crafter_destroy(h);
  return fail(nullptr, msg);
}

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
  if (h->plan.render_lds > kMaxLds)
    return create_fail(h, "crafter_create: one environment needs " + std::to_string(h->plan.render_lds) +
                              " B of LDS (> 160 KiB): area / max_objects too large for the LDS-resident kernels");
  if ((c.step_threads != 0 && c.step_threads != kStepThreads) || (c.reset_threads != 0 && c.reset_threads != kResetThreads))
    return create_fail(h, "crafter_create: workgroup sizes are fixed in this build (step_threads 0 or " +
                              std::to_string(kStepThreads) + ", reset_threads 0 or " + std::to_string(kResetThreads) + ")");
  if (h->plan.opt_in_lds) {   // large worlds only: the generic instances (the default geometry needs 33 KB)
    hipError_t er = rollout_allow_lds(h->plan.render_lds);   // the rollout kernels live in crafter_rollout.hip
    if (er != hipSuccess) return create_fail(h, std::string("crafter_create: hipFuncSetAttribute(rollout kernels): ") + hipGetErrorString(er));
    er = subset_allow_lds(h->plan.render_lds);   // ... and crafter_step_envs' in crafter_subset.hip
    if (er != hipSuccess) return create_fail(h, std::string("crafter_create: hipFuncSetAttribute(subset kernels): ") + hipGetErrorString(er));
    er = rollout_envs_allow_lds(h->plan.render_lds);   // ... and crafter_step_n_envs' in crafter_rollout_subset.hip
    if (er != hipSuccess) return create_fail(h, std::string("crafter_create: hipFuncSetAttribute(subset rollout kernels): ") + hipGetErrorString(er));
    for (const void* f : big_lds_kernels()) {
      hipError_t ea = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, h->plan.render_lds);
      if (ea != hipSuccess)
        return create_fail(h, std::string("crafter_create: hipFuncSetAttribute(MaxDynamicSharedMemorySize, ") +
                                  std::to_string(h->plan.render_lds) + "): " + hipGetErrorString(ea));
    }
  }
  {   // dispatch order (see crafter_handle::order).  CRAFTER_ORDER=0 / 1: never / whenever possible (A/B)
    const char* v = getenv("CRAFTER_ORDER");
    if (keeps_dispatch_order(c.num_envs, v ? atoi(v) : -1)) {
      hipError_t ea = hipMalloc((void**)&h->order, 2 * (size_t)c.num_envs * sizeof(int32_t));
      if (ea == hipSuccess) h->owned.push_back(h->order);
      if (ea == hipSuccess) ea = hipMalloc((void**)&h->next_step, (size_t)c.num_envs * sizeof(int32_t));
      if (ea == hipSuccess) h->owned.push_back(h->next_step);
      if (ea == hipSuccess) ea = hipMemset(h->next_step, 0, (size_t)c.num_envs * sizeof(int32_t));
      if (ea != hipSuccess) return create_fail(h, std::string("crafter_create: dispatch order buffers: ") + hipGetErrorString(ea));
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
    if (!ok) return create_fail(h, "crafter_create: cannot create the world-pool stream / events");
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
  h->n_materials = r->n_materials;
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

int crafter_reset(crafter_handle* h, const uint8_t* mask, uint8_t* obs, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (ready(h, "crafter_reset")) return 1;
  // The reset kernel generates the next episode's world into the env's pool entry itself (gen_one): it must not share
  // that entry with a generation batch still in flight on a side stream (an env reset in mid-episode k may have world
  // k + 2 in such a batch, and k + 2 lives in the entry the kernel is about to write: ADVICE r2).  So the launch stream
  // is ordered behind every launched batch first -- no host wait -- and all of them are trusted from here on.
  if (adopt_stream(h, s)) return 1;
  if (pool_live(h)) pool_wait_all(h, s, "hipStreamWaitEvent(reset)");
  hipLaunchKernelGGL(crafter_reset_kernel, dim3(h->cfg.num_envs), dim3(kResetThreads), h->plan.reset_lds,
                     s, h->cfg, h->tb, h->st, mask, pool_live(h) ? h->gen_parity : -1, obs,
                     (const LevelTable*)h->levels);
  return launched(h, "crafter_reset launch");
}

// Env.reset into authored worlds: crafter_reset with another world source (env_worlds.hpp).  The kernel ends on the reset
// kernel's own tail (reset_pool_tail), so the launch stream is ordered behind the pool exactly as there.
int crafter_reset_worlds(crafter_handle* h, const uint8_t* mask, const int32_t* world_id, const uint8_t* bank_mat, const crafter_obj* bank_objs,
                         const int32_t* bank_nobj, const int32_t* bank_inv, int32_t n_worlds, int32_t bank_max_objects, uint8_t* obs,
                         void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (ready(h, "crafter_reset_worlds")) return 1;
  if (!bank_mat || !bank_objs || !bank_nobj) return fail(h, "crafter_reset_worlds: bank_mat, bank_objs and bank_nobj must not be NULL");
  if (n_worlds < 1) return fail(h, "crafter_reset_worlds: n_worlds must be at least 1");
  if (bank_max_objects < 0) return fail(h, "crafter_reset_worlds: bank_max_objects must not be negative");
  if (((uintptr_t)bank_objs & 15u) != 0) return fail(h, "crafter_reset_worlds: bank_objs must be 16-byte aligned");
  if (adopt_stream(h, s)) return 1;
  if (pool_live(h)) pool_wait_all(h, s, "hipStreamWaitEvent(reset_worlds)");
  WorldBank bank;
  bank.world_id = world_id;
  bank.mat = bank_mat;
  bank.objs = bank_objs;
  bank.nobj = bank_nobj;
  bank.inv = bank_inv;
  bank.n_worlds = n_worlds;
  bank.max_objects = bank_max_objects;
  hipLaunchKernelGGL(crafter_reset_worlds_kernel, dim3(h->cfg.num_envs), dim3(kResetThreads), h->plan.reset_lds, s,
                     h->cfg, h->tb, h->st, mask, bank, pool_live(h) ? h->gen_parity : -1, obs,
                     (const LevelTable*)h->levels);
  return launched(h, "crafter_reset_worlds launch");
}

// The scratch of an index check on the device (crafter_copy_check_kernel, crafter_step_envs_check_kernel): one mark per row of
// the bound state and the verdict word, allocated on first use; *stamp: this call's number in the marks, which are cleared
// only when the numbers start again.
static int index_check_scratch(crafter_handle* h, const char* who, hipStream_t stream, int32_t* stamp) {
  if (need_scratch(h, (void**)&h->copy_mark, ((size_t)h->cfg.num_envs + 1) * sizeof(int32_t), who)) return 1;
  h->copy_verdict = h->copy_mark + h->cfg.num_envs;
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
  return launched(h, who);
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
  const hipStream_t s = (hipStream_t)stream;
  if (ready(h, "crafter_copy_envs")) return 1;
  if (n < 0 || (n > 0 && (!src || !dst))) return fail(h, "crafter_copy_envs: bad index arrays");
  if (n == 0) return 0;
  if (adopt_stream(h, s)) return 1;
  pool_quiesce(h, s);
  const int N = h->cfg.num_envs;
  CopySide side{&h->st, N, h->cfg.max_objects, obs, reward, done};
  return launch_copy(h, "crafter_copy_envs", COPY_WITHIN, side, side, src, dst, n, s, pool_live(h));
}

int crafter_save_envs(crafter_handle* h, const int32_t* idx, int32_t n, const uint8_t* obs, const float* reward, const uint8_t* done,
                      const crafter_state_ptrs* store, int32_t store_rows, int32_t store_max_objects, uint8_t* store_obs,
                      float* store_reward, uint8_t* store_done, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (ready(h, "crafter_save_envs")) return 1;
  if (check_store(h, "crafter_save_envs", store, store_rows, store_max_objects)) return 1;
  if (n < 0 || n > store_rows) return fail(h, "crafter_save_envs: n outside 0 .. store_rows");
  if (store_max_objects < h->cfg.max_objects) return fail(h, "crafter_save_envs: the store's slot table is narrower than the batch's");
  if (n == 0) return 0;
  if (adopt_stream(h, s)) return 1;   // (reads live rows only: the pool's side streams never write them)
  CopySide a{&h->st, h->cfg.num_envs, h->cfg.max_objects, obs, reward, done};
  CopySide b{store, store_rows, store_max_objects, store_obs, store_reward, store_done};
  return launch_copy(h, "crafter_save_envs", COPY_SAVE, a, b, idx, nullptr, n, s, false);
}

int crafter_load_envs(crafter_handle* h, const crafter_state_ptrs* store, int32_t store_rows, int32_t store_max_objects,
                      const uint8_t* store_obs, const float* store_reward, const uint8_t* store_done, const int32_t* rows,
                      const int32_t* idx, int32_t n, uint8_t* obs, float* reward, uint8_t* done, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (ready(h, "crafter_load_envs")) return 1;
  if (check_store(h, "crafter_load_envs", store, store_rows, store_max_objects)) return 1;
  if (n < 0 || (n > 0 && !idx)) return fail(h, "crafter_load_envs: bad index arrays");
  if (store_max_objects > h->cfg.max_objects) return fail(h, "crafter_load_envs: the store's slot table is wider than the batch's (grow the batch first)");
  if (h->cfg.want_semantic && !store->semantic) return fail(h, "crafter_load_envs: the batch keeps info['semantic'], the store does not");
  if (n == 0) return 0;
  if (adopt_stream(h, s)) return 1;
  pool_quiesce(h, s);
  CopySide a{store, store_rows, store_max_objects, store_obs, store_reward, store_done};
  CopySide b{&h->st, h->cfg.num_envs, h->cfg.max_objects, obs, reward, done};
  return launch_copy(h, "crafter_load_envs", COPY_LOAD, a, b, rows, idx, n, s, false);
}

// Level selection (env_levels.hpp): the named envs' next reset starts episode `episode` of lane `seed_lane`.  The kernel empties
// their pool entries, so the pool is brought to rest first, exactly as before crafter_load_envs: without that a batch in flight
// could deliver a world of the old lane into an emptied entry behind the kernel, and a queued request would keep `pending` set.
// A pool that is off or has failed is not waited for; a failed pool's entries (still bound) are emptied all the same.
int crafter_reseed(crafter_handle* h, const uint8_t* mask, const uint64_t* seed_lane, const int32_t* episode, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (ready(h, "crafter_reseed")) return 1;
  if (!seed_lane) return fail(h, "crafter_reseed: null seed_lane");
  if (adopt_stream(h, s)) return 1;
  pool_quiesce(h, s);
  hipLaunchKernelGGL(crafter_reseed_kernel, dim3((unsigned)((h->cfg.num_envs + kReseedThreads - 1) / kReseedThreads)), dim3(kReseedThreads), 0,
                     s, h->cfg, h->st, mask, seed_lane, episode);
  return launched(h, "crafter_reseed launch");
}

// Level sets (env_levels.hpp).  The table lives in one handle-owned buffer of full capacity, allocated by the first call, so no
// reallocation is ever ordered against work in flight; kernels enqueued before that call got a null pointer: no table.  Every
// pooled world was generated under the table being replaced, so the pool is brought to rest as before crafter_reseed and the
// kernel empties EVERY env's entries.  With the pool off or failed (the step kernels then never adopt) only the table is written.
int crafter_set_levels(crafter_handle* h, const uint64_t* seed_lane, const int32_t* episode, const uint32_t* cum, int32_t n_levels,
                       uint64_t key, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (ready(h, "crafter_set_levels")) return 1;
  if (n_levels < 0 || n_levels > kMaxLevels) return fail(h, "crafter_set_levels: n_levels outside 0 .. " + std::to_string(kMaxLevels));
  if (n_levels > 0 && (!seed_lane || !episode)) return fail(h, "crafter_set_levels: null seed_lane / episode");
  const bool fresh = !h->levels;
  if (fresh && n_levels == 0) return 0;   // no table was ever set: nothing to clear
  if (need_scratch(h, (void**)&h->levels, sizeof(LevelTable), "crafter_set_levels: hipMalloc")) return 1;
  if (adopt_stream(h, s)) return 1;
  if (fresh) {   // "no table" until the kernel below has run: the batch pool_quiesce launches (ordered behind this point of the
                 // stream, ev_main) already takes the pointer
    hipError_t em = hipMemsetAsync(h->levels, 0, offsetof(LevelTable, lane), s);
    if (em != hipSuccess) return hip_fail(h, "crafter_set_levels: hipMemsetAsync", em);
  }
  pool_quiesce(h, s);
  StatePtrs st = h->st;
  if (!pool_live(h)) {
    st.pool_hdr = nullptr;
    st.gen_latest = nullptr;
  }
  const int threads = n_levels > h->cfg.num_envs ? n_levels : h->cfg.num_envs;
  hipLaunchKernelGGL(crafter_set_levels_kernel, dim3((unsigned)((threads + kLevelThreads - 1) / kLevelThreads)), dim3(kLevelThreads), 0,
                     s, h->cfg, st, h->levels, seed_lane, episode, n_levels > 0 ? cum : nullptr, (int)n_levels, key);
  return launched(h, "crafter_set_levels launch");
}

int crafter_level_ids(crafter_handle* h, const uint8_t* mask, int32_t* ids, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (ready(h, "crafter_level_ids")) return 1;
  if (!ids) return fail(h, "crafter_level_ids: null ids");
  if (adopt_stream(h, s)) return 1;   // (reads the records and the table only: no wait for the pool beyond that)
  hipLaunchKernelGGL(crafter_level_ids_kernel, dim3((unsigned)((h->cfg.num_envs + kLevelThreads - 1) / kLevelThreads)), dim3(kLevelThreads), 0,
                     s, h->cfg, h->st, (const LevelTable*)h->levels, mask, ids);
  return launched(h, "crafter_level_ids launch");
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
    CRAFTER_LAUNCH(crafter_requeue_final_kernel, dim3(grid), dim3(kRequeueThreads), final_lds(h), stream, start, stop, h->cfg, h->tb, h->st, ctl.parity,
                   pool_parity, ctl.safe_seq, obs, ctl.next_step, *fin, (const LevelTable*)h->levels);
    return;
  }
  CRAFTER_LAUNCH(crafter_requeue_reset_kernel, dim3(requeue_grid(h, ctl)), dim3(kRequeueThreads), h->plan.reset_lds, stream, start, stop,
                        h->cfg, h->tb, h->st, ctl.parity, ctl.gen_parity, obs, (const LevelTable*)h->levels);
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
static int step_launch(crafter_handle* h, const int32_t* actions, uint8_t* obs, float* reward, uint8_t* done, hipStream_t s,
                       const FinalOut* fin) {
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  const bool frames = h->cfg.render_obs != 0 && obs != nullptr;
  const bool requeue = h->cfg.auto_reset != 0;
  const StepKernel kernel = choose_step(h->plan, h->cfg.num_envs, frames, h->order != nullptr, h->split, h->wide, h->early_frame);
  const bool ordered = h->order && !is_split(kernel);   // (the wide kernel is only chosen where no order is kept)
  const bool fused_frames = frames && !is_split(kernel);   // a fused step kernel draws
  // the scratch the choice needs
  if (fused_frames && need_noise_raw(h, "crafter_step: noise scratch")) return 1;
  if (kernel == kStepRulesFrame && need_night_px(h, "crafter_step: frame kernel scratch")) return 1;
  if (h->plan.night_px && frames && need_night_px(h, "crafter_step: night frame scratch")) return 1;
  StepCtl ctl = step_ctl(h, fused_frames);
  const int pool_parity = ctl.gen_parity;
  if (fin) ctl.gen_parity = -1;
  ctl.early_frame = step_early_frame(h->cfg.num_envs, h->early_frame);
  if (timing_events(h, ev, "crafter_step: hipEventCreate (timing mode)")) return 1;
  if (ordered) set_dispatch_order(h, ctl);
  const dim3 grid_n(h->cfg.num_envs + (ordered ? 1 : 0)), block_s(kStepThreads);   // (ordered: block 0 builds the next launch's order)
  // The regeneration kernel (envs that finished and found no world in the pool: all but never any) only has to sit between
  // the rules of this step and the rules of the next.  In the split step it runs BESIDE the frame kernel, on the handle's own
  // stream -- the envs it regenerates and draws are exactly those the frame kernel skips -- so its launch and the look at
  // the (empty) queue cost the launch stream nothing.
  bool beside = false;
  switch (kernel) {
    case kStepRules:   // split step: rules at wave granularity ...
      CRAFTER_LAUNCH(crafter_rules_kernel, grid_n, dim3(kRulesThreads), lane_layout(h->cfg).total, s, ev[0], ev[1],
                     h->cfg, h->tb, h->st, actions, obs, reward, done, ctl);
      break;
    case kStepRulesFrame:   // ... then the frames
      CRAFTER_LAUNCH(crafter_rules_kernel, grid_n, dim3(kRulesThreads), lane_layout(h->cfg).total, s, ev[0], nullptr,
                     h->cfg, h->tb, h->st, actions, obs, reward, done, ctl);
      if (requeue && h->aux) {
        hipError_t ea = hipEventRecord(h->ev_rules, s);
        if (ea == hipSuccess) ea = hipStreamWaitEvent(h->aux, h->ev_rules, 0);
        if (ea != hipSuccess) return hip_fail(h, "crafter_step: fork to the regeneration stream", ea);
        beside = true;
        launch_requeue(h, ctl, obs, h->aux, ev[2], ev[3], fin, pool_parity);
        ea = hipEventRecord(h->ev_requeue, h->aux);
        if (ea != hipSuccess) return hip_fail(h, "crafter_step: hipEventRecord(regeneration stream)", ea);
      }
      CRAFTER_LAUNCH(crafter_frame_kernel, grid_n, block_s, frame_layout(h->cfg).total, s, nullptr, ev[1],
                     h->cfg, h->tb, h->st, obs, h->night_px);
      if (beside) {
        hipError_t ea = hipStreamWaitEvent(s, h->ev_requeue, 0);
        if (ea != hipSuccess) return hip_fail(h, "crafter_step: join of the regeneration stream", ea);
      }
      break;
    case kStepWide:   // few envs: eight waves per env
      CRAFTER_LAUNCH(crafter_step_wide_kernel, grid_n, dim3(kWideThreads), h->plan.step_lds, s, ev[0], ev[1],
                     h->cfg, h->tb, h->st, actions, obs, reward, done, ctl);
      break;
    case kStepEarly:   // batches larger than the chip holds at once
      CRAFTER_LAUNCH(crafter_step_early_kernel, grid_n, block_s, h->plan.step_lds, s, ev[0], ev[1],
                     h->cfg, h->tb, h->st, actions, obs, reward, done, ctl);
      break;
    case kStepFused:
      launch_step_fused(h, grid_n, s, ev[0], ev[1], actions, obs, reward, done, ctl);
      break;
  }
  if (launched(h, "crafter_step launch")) return 1;
  if (requeue && !beside) launch_requeue(h, ctl, obs, s, ev[2], ev[3], fin, pool_parity);
  if (launched(h, "crafter_step (auto-reset) launch")) return 1;
  keep_timing_events(h, ev);
  if (pool_live(h)) pool_schedule(h, s);
  return 0;
}

int crafter_step(crafter_handle* h, const int32_t* actions, uint8_t* obs, float* reward, uint8_t* done,
                 void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (ready(h, "crafter_step")) return 1;
  if (!actions || !reward || !done) return fail(h, "crafter_step: null argument");
  if (adopt_stream(h, s)) return 1;
  return step_launch(h, actions, obs, reward, done, s, nullptr);
}

int crafter_step_final(crafter_handle* h, const int32_t* actions, uint8_t* obs, float* reward, uint8_t* done,
                       uint8_t* final_obs, uint8_t* terminated, uint8_t* final_local, float* final_stats, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (ready(h, "crafter_step_final")) return 1;
  if (!actions || !reward || !done || !terminated) return fail(h, "crafter_step_final: null argument");
  if (!h->cfg.auto_reset || !h->st.reset_q)
    return fail(h, "crafter_step_final: the handle has no auto_reset (obs of crafter_step already is the final frame there)");
  if (symbolic_strip_bytes(h->cfg) > final_lds(h)) return fail(h, "crafter_step_final: the local view is too large for the kernel's LDS");
  if (adopt_stream(h, s)) return 1;
  FinalOut fin;
  fin.obs = h->cfg.render_obs != 0 ? final_obs : nullptr;
  fin.terminated = terminated;
  fin.local = final_local;
  fin.stats = final_stats;
  return step_launch(h, actions, obs, reward, done, s, &fin);
}

// Env.step for the n envs idx names, and for no other: the index check (which scatters the actions to their envs' rows), then
// n workgroups of the plan's instance (crafter_subset.hip), then the regeneration kernel as behind crafter_step.  One call is
// one step to the world pool's schedule: an env steps at most once per call.
int crafter_step_envs(crafter_handle* h, const int32_t* idx, int32_t n, const int32_t* actions, uint8_t* obs, float* reward, uint8_t* done,
                      void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (ready(h, "crafter_step_envs")) return 1;
  if (n < 0 || n > h->cfg.num_envs) return fail(h, "crafter_step_envs: n outside 0 .. num_envs");
  if (n == 0) return 0;
  if (!idx) return fail(h, "crafter_step_envs: null index list");
  if (!actions || !reward || !done) return fail(h, "crafter_step_envs: null argument");
  if (adopt_stream(h, s)) return 1;
  if (need_scratch(h, (void**)&h->subset_actions, (size_t)h->cfg.num_envs * sizeof(int32_t), "crafter_step_envs: actions scratch")) return 1;
  const bool frames = h->cfg.render_obs != 0 && obs != nullptr;
  const StepEnvsKernel kernel = choose_step_envs(h->plan, n, frames, h->wide);
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  if (frames && need_noise_raw(h, "crafter_step_envs: noise scratch")) return 1;   // (night frames: as in crafter_step)
  if (h->plan.night_px && frames && need_night_px(h, "crafter_step_envs: night frame scratch")) return 1;
  SubsetCheck chk;
  chk.idx = idx; chk.actions = actions; chk.n = n;
  if (index_check_scratch(h, "crafter_step_envs", s, &chk.stamp)) return 1;
  chk.mark = h->copy_mark; chk.verdict = h->copy_verdict; chk.rec = (EnvRec*)h->st.rec; chk.rows = h->cfg.num_envs;
  chk.scattered = h->subset_actions;
  if (timing_events(h, ev, "crafter_step_envs: hipEventCreate (timing mode)")) return 1;
  StepCtl ctl = step_ctl(h, frames);   // (early_frame stays 0: no early-frame kernel for subsets, launch_plan.hpp choose_step_envs)
  ctl.next_step = h->next_step;        // an ordered handle: the named envs' entries stay current; the launch follows no order and builds none
  // timing mode: the step time of the call runs from the check's start to the subset kernel's end
  launch_step_envs_check(chk, s, ev[0], nullptr);
  launch_step_subset(kernel, h->plan.instance, n, (size_t)h->plan.step_lds, s, nullptr, ev[1], h->cfg, h->tb, h->st, idx,
                     h->copy_verdict, h->subset_actions, obs, reward, done, ctl);
  if (launched(h, "crafter_step_envs launch")) return 1;
  if (h->cfg.auto_reset != 0) launch_requeue(h, ctl, obs, s, ev[2], ev[3]);
  if (launched(h, "crafter_step_envs (auto-reset) launch")) return 1;
  keep_timing_events(h, ev);
  if (pool_live(h)) pool_schedule(h, s);
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
  const hipStream_t s = (hipStream_t)stream;
  if (ready(h, "crafter_step_n")) return 1;
  if (!actions || !reward || !done || steps < 1) return fail(h, "crafter_step_n: bad argument");
  if (adopt_stream(h, s)) return 1;
  bool pooled = pool_live(h);
  if (need_scratch(h, (void**)&h->stalled_at, (size_t)h->cfg.num_envs * sizeof(int32_t), "crafter_step_n: hipMalloc")) return 1;
  const bool frames = obs != nullptr && h->cfg.render_obs != 0;
  if (frames && need_noise_raw(h, "crafter_step_n: noise scratch")) return 1;
  if (h->plan.night_px && frames && need_night_px(h, "crafter_step_n: night frame scratch")) return 1;   // big_layout
  const size_t n = (size_t)h->cfg.num_envs;
  const size_t obs_stride = n * (size_t)h->cfg.size_w * h->cfg.size_h * 3;
  const bool requeue = h->cfg.auto_reset != 0;
  for (int done_steps = 0; done_steps < steps;) {
    const int T = stretch_steps(h, steps - done_steps, pooled);
    const int32_t* a = actions + (size_t)done_steps * n;
    uint8_t* o = obs ? obs + (size_t)done_steps * obs_stride : nullptr;
    float* r = reward + (size_t)done_steps * n;
    uint8_t* d = done + (size_t)done_steps * n;
    StepCtl ctl = step_ctl(h, frames);
    RolloutArgs ra;
    ra.T = T; ra.obs_stride = obs_stride; ra.stalled_at = h->stalled_at;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    if (timing_events(h, ev, "crafter_step_n: hipEventCreate (timing mode)")) return 1;
    if (h->order && h->rollout_order) set_dispatch_order(h, ctl);   // slow envs first, as in crafter_step
    launch_rollout(h->plan.instance, h->cfg.num_envs, (size_t)h->plan.rollout_lds, s, ev[0], ev[1], h->cfg, h->tb, h->st,
                   a, o, r, d, ctl, ra);
    if (launched(h, "crafter_step_n launch")) return 1;
    const bool batch = batch_follows(h, pooled, requeue, T);   // (then ev_main is the stop event of the stretch's last kernel)
    if (requeue)
      launch_requeue_rollout(requeue_grid(h, ctl), (size_t)h->plan.render_lds, s, ev[2], batch ? h->ev_main : ev[3], h->cfg, h->tb,
                             h->st, a, o, r, d, ctl, ra, h->levels);
    if (launched(h, "crafter_step_n (auto-reset) launch")) return 1;
    keep_timing_events(h, ev);
    if (pooled) pool_schedule(h, s, T, batch, true);
    pooled = pool_live(h);
    done_steps += T;
  }
  return 0;
}

// crafter_step_n for the n envs idx names, and for no other, with compact outputs (crafter_rollout_subset.hpp): the index check
// once, in front of the first stretch -- its verdict stays valid for the call's later stretches, calls on a handle being
// serialised --, then crafter_step_n's stretch loop over the subset's kernels.
int crafter_step_n_envs(crafter_handle* h, const int32_t* idx, int32_t n, int32_t steps, const int32_t* actions, uint8_t* obs, float* reward,
                        uint8_t* done, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (ready(h, "crafter_step_n_envs")) return 1;
  if (n < 0 || n > h->cfg.num_envs) return fail(h, "crafter_step_n_envs: n outside 0 .. num_envs");
  if (n == 0) return 0;
  if (!idx) return fail(h, "crafter_step_n_envs: null index list");
  if (!actions || !reward || !done || steps < 1) return fail(h, "crafter_step_n_envs: bad argument");
  if (adopt_stream(h, s)) return 1;
  bool pooled = pool_live(h);
  if (need_scratch(h, (void**)&h->stalled_at, (size_t)h->cfg.num_envs * sizeof(int32_t), "crafter_step_n_envs: hipMalloc")) return 1;
  if (need_scratch(h, (void**)&h->rollout_row_of, (size_t)h->cfg.num_envs * sizeof(int32_t), "crafter_step_n_envs: row scratch")) return 1;
  const bool frames = obs != nullptr && h->cfg.render_obs != 0;
  if (frames && need_noise_raw(h, "crafter_step_n_envs: noise scratch")) return 1;
  if (h->plan.night_px && frames && need_night_px(h, "crafter_step_n_envs: night frame scratch")) return 1;   // big_layout
  RolloutEnvsCheck chk;
  chk.idx = idx; chk.n = n;
  if (index_check_scratch(h, "crafter_step_n_envs", s, &chk.stamp)) return 1;
  chk.mark = h->copy_mark; chk.verdict = h->copy_verdict; chk.rec = (EnvRec*)h->st.rec; chk.rows = h->cfg.num_envs;
  chk.row_of = h->rollout_row_of;
  const size_t rows = (size_t)n;
  const size_t obs_stride = rows * (size_t)h->cfg.size_w * h->cfg.size_h * 3;
  const bool requeue = h->cfg.auto_reset != 0;
  for (int done_steps = 0; done_steps < steps;) {
    const int T = stretch_steps(h, steps - done_steps, pooled);   // stretches as crafter_step_n's
    const int32_t* a = actions + (size_t)done_steps * rows;
    uint8_t* o = obs ? obs + (size_t)done_steps * obs_stride : nullptr;
    float* r = reward + (size_t)done_steps * rows;
    uint8_t* d = done + (size_t)done_steps * rows;
    StepCtl ctl = step_ctl(h, frames);
    ctl.next_step = h->next_step;   // an ordered handle: the named envs' entries stay current; the launch follows no order and builds none
    RolloutEnvsArgs ra;
    ra.idx = idx; ra.verdict = h->copy_verdict; ra.row_of = h->rollout_row_of; ra.n = n; ra.T = T; ra.stalled_at = h->stalled_at;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    if (timing_events(h, ev, "crafter_step_n_envs: hipEventCreate (timing mode)")) return 1;
    // timing mode: the first stretch's step time runs from the check's start to the rollout kernel's end
    if (done_steps == 0) launch_rollout_envs_check(chk, s, ev[0], nullptr);
    launch_rollout_envs(h->plan.instance, (size_t)h->plan.rollout_lds, s, done_steps == 0 ? nullptr : ev[0], ev[1], h->cfg, h->tb,
                        h->st, a, o, r, d, ctl, ra);
    if (launched(h, "crafter_step_n_envs launch")) return 1;
    const bool batch = batch_follows(h, pooled, requeue, T);   // (as in crafter_step_n)
    if (requeue)
      launch_requeue_rollout_envs(requeue_grid(h, ctl), (size_t)h->plan.render_lds, s, ev[2], batch ? h->ev_main : ev[3],
                                  h->cfg, h->tb, h->st, a, o, r, d, ctl, ra, h->levels);
    if (launched(h, "crafter_step_n_envs (auto-reset) launch")) return 1;
    keep_timing_events(h, ev);
    if (pooled) pool_schedule(h, s, T, batch, true);
    pooled = pool_live(h);
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
  const hipStream_t s = (hipStream_t)stream;
  if (ready(h, "crafter_render")) return 1;
  if (!out) return fail(h, "crafter_render: null output");
  if (adopt_stream(h, s)) return 1;
  hipLaunchKernelGGL(crafter_render_kernel, dim3(h->cfg.num_envs), dim3(kStepThreads), h->plan.render_lds,
                     s, h->cfg, h->tb, h->st, mask, out);
  return launched(h, "crafter_render launch");
}

// The symbolic observation of the state as it stands on `stream` (symbolic.hpp).  Reads live rows only -- the pool's side
// streams never write them -- so, like crafter_save_envs, it waits for no batch.
int crafter_symbolic(crafter_handle* h, const uint8_t* mask, uint8_t* local, float* stats, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (ready(h, "crafter_symbolic")) return 1;
  if (!local && !stats) return 0;
  const int lds = kSymbolicEnvs * symbolic_strip_bytes(h->cfg);
  if (lds > 64 * 1024) return fail(h, "crafter_symbolic: the local view is too large for the kernel's LDS strips");
  if (adopt_stream(h, s)) return 1;
  const dim3 grid((unsigned)((h->cfg.num_envs + kSymbolicEnvs - 1) / kSymbolicEnvs)), block(kSymbolicThreads);
  if (h->plan.maps_in_lds)
    hipLaunchKernelGGL(crafter_symbolic_kernel<0>, grid, block, lds, s, h->cfg, h->tb, h->st, mask, local, stats,
                       symbolic_strip_bytes(h->cfg));
  else
    hipLaunchKernelGGL(crafter_symbolic_kernel<1>, grid, block, lds, s, h->cfg, h->tb, h->st, mask, local, stats,
                       symbolic_strip_bytes(h->cfg));
  return launched(h, "crafter_symbolic launch");
}

// The legal-action mask of the state as it stands on `stream` (legal.hpp).  Like crafter_symbolic it reads live rows only and
// waits for no batch of the pool.
int crafter_legal_actions(crafter_handle* h, const uint8_t* mask, uint8_t* legal, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (ready(h, "crafter_legal_actions")) return 1;
  if (!legal) return fail(h, "crafter_legal_actions: null output");
  if (adopt_stream(h, s)) return 1;
  const dim3 grid((unsigned)((h->cfg.num_envs + kLegalEnvs - 1) / kLegalEnvs)), block(kLegalThreads);
  if (h->plan.maps_in_lds)
    hipLaunchKernelGGL(crafter_legal_actions_kernel<0>, grid, block, 0, s, h->cfg, h->tb, h->st, mask, legal);
  else
    hipLaunchKernelGGL(crafter_legal_actions_kernel<1>, grid, block, 0, s, h->cfg, h->tb, h->st, mask, legal);
  return launched(h, "crafter_legal_actions launch");
}

// The state fingerprints of the envs as they stand on `stream` (fingerprint.hpp).  Like crafter_symbolic it reads live rows only
// and waits for no batch of the pool.
int crafter_fingerprint(crafter_handle* h, const uint8_t* mask, uint32_t parts, uint64_t* key, uint64_t* part_hash, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (ready(h, "crafter_fingerprint")) return 1;
  if (!key && !part_hash) return fail(h, "crafter_fingerprint: both outputs are null");
  if (parts & ~(uint32_t)CRAFTER_FP_ALL) return fail(h, "crafter_fingerprint: parts names a bit above CRAFTER_FP_IDENT");
  if (key && !parts) return fail(h, "crafter_fingerprint: a key of no part (parts == 0)");
  if (adopt_stream(h, s)) return 1;
  const dim3 grid((unsigned)((h->cfg.num_envs + kFingerprintEnvs - 1) / kFingerprintEnvs)), block(kFingerprintThreads);
  hipLaunchKernelGGL(crafter_fingerprint_kernel, grid, block, 0, s, h->cfg, h->tb, h->st, mask, parts, key, part_hash);
  return launched(h, "crafter_fingerprint launch");
}

// The navigation query of the envs as they stand on `stream` (navigate.hpp).  Like crafter_symbolic it reads live rows only and
// waits for no batch of the pool.  The instance follows the handle's config: boards in registers for worlds of at most 64 x 64
// cells, in LDS beyond; the object path as crafter_legal_actions.
int crafter_navigate(crafter_handle* h, const uint8_t* mask, const uint32_t* targets, int32_t k, uint32_t passable,
                     int32_t* dist, int32_t* first, uint8_t* facing, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (ready(h, "crafter_navigate")) return 1;
  if (const int why = nav_check(h->n_materials, targets, k, passable)) return fail(h, std::string("crafter_navigate: ") + nav_error_text(why));
  if (!dist || !first) return fail(h, "crafter_navigate: dist or first is null");
  NavQuery q;
  memset(&q, 0, sizeof(q));
  memcpy(q.targets, targets, sizeof(uint32_t) * (size_t)k);
  q.passable = passable;
  q.k = k;
  const bool map = !h->plan.maps_in_lds;
  if (nav_in_registers(h->cfg)) {
    if (adopt_stream(h, s)) return 1;
    const dim3 grid((unsigned)((h->cfg.num_envs + kNavEnvs - 1) / kNavEnvs)), block(kNavThreads);
    if (map)
      hipLaunchKernelGGL(crafter_navigate_kernel<1>, grid, block, 0, s, h->cfg, h->tb, h->st, mask, q, dist, first, facing);
    else
      hipLaunchKernelGGL(crafter_navigate_kernel<0>, grid, block, 0, s, h->cfg, h->tb, h->st, mask, q, dist, first, facing);
  } else {
    const size_t lds = nav_lds_bytes(h->cfg);
    if (lds > (size_t)kNavMaxLds) return fail(h, "crafter_navigate: the area's boards exceed 64 KiB of LDS");
    if (adopt_stream(h, s)) return 1;
    const dim3 grid((unsigned)h->cfg.num_envs), block(kNavWideThreads);
    if (map)
      hipLaunchKernelGGL(crafter_navigate_lds_kernel<1>, grid, block, lds, s, h->cfg, h->tb, h->st, mask, q, dist, first, facing);
    else
      hipLaunchKernelGGL(crafter_navigate_lds_kernel<0>, grid, block, lds, s, h->cfg, h->tb, h->st, mask, q, dist, first, facing);
  }
  return launched(h, "crafter_navigate launch");
}

// The audit of the rows as they stand on `stream` (audit.hpp): every derived table recounted from mat, objs and rec.  Like
// crafter_symbolic it reads live rows only and waits for no batch of the pool; it sets no status bit.  One wave per env for
// worlds of at most 64 x 64 cells and 256 slots, a workgroup of 256 threads beyond; objmap is audited where it is state.
int crafter_audit(crafter_handle* h, const uint8_t* mask, int32_t* flags, int32_t* detail, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (ready(h, "crafter_audit")) return 1;
  if (!flags || !detail) return fail(h, "crafter_audit: flags or detail is null");
  const size_t lds = audit_lds_words(h->cfg) * 4;
  if (lds > (size_t)kAuditMaxLds) return fail(h, "crafter_audit: the area's tables exceed 64 KiB of LDS");
  if (adopt_stream(h, s)) return 1;
  const dim3 grid((unsigned)h->cfg.num_envs);
  const bool map = !h->plan.maps_in_lds;
  if (audit_in_wave(h->cfg)) {
    if (map)
      hipLaunchKernelGGL((crafter_audit_kernel<kAuditThreads, 1>), grid, dim3(kAuditThreads), lds, s, h->cfg, h->tb, h->st, mask, flags, detail);
    else
      hipLaunchKernelGGL((crafter_audit_kernel<kAuditThreads, 0>), grid, dim3(kAuditThreads), lds, s, h->cfg, h->tb, h->st, mask, flags, detail);
  } else {
    if (map)
      hipLaunchKernelGGL((crafter_audit_kernel<kAuditWideThreads, 1>), grid, dim3(kAuditWideThreads), lds, s, h->cfg, h->tb, h->st, mask, flags, detail);
    else
      hipLaunchKernelGGL((crafter_audit_kernel<kAuditWideThreads, 0>), grid, dim3(kAuditWideThreads), lds, s, h->cfg, h->tb, h->st, mask, flags, detail);
  }
  return launched(h, "crafter_audit launch");
}

// The nearby query of the envs as they stand on `stream` (nearby.hpp): class counts over a window around the player and the k
// nearest objects.  Like crafter_symbolic it reads live rows only and waits for no batch of the pool.  One wave per env for worlds
// of at most 64 x 64 cells, a workgroup of 256 threads beyond; the object pass may walk objmap where it is state.
int crafter_nearby(crafter_handle* h, const uint8_t* mask, int32_t distance, int32_t flags, uint32_t classes, int32_t k,
                   int32_t* counts, int16_t* ents, int32_t* n, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (ready(h, "crafter_nearby")) return 1;
  if (const int why = near_check(h->cfg, h->n_materials, distance, flags, classes, k, counts, ents, n))
    return fail(h, std::string("crafter_nearby: ") + near_error_text(why));
  const NearQuery q = {distance, flags, classes, k, -1};
  const size_t lds = near_lds_words(h->cfg, k) * 4;
  if (adopt_stream(h, s)) return 1;
  const dim3 grid((unsigned)h->cfg.num_envs);
  const bool map = !h->plan.maps_in_lds;
  if (near_in_wave(h->cfg)) {
    if (map)
      hipLaunchKernelGGL((crafter_nearby_kernel<kNearThreads, 1>), grid, dim3(kNearThreads), lds, s, h->cfg, h->tb, h->st, mask, q, counts, ents, n);
    else
      hipLaunchKernelGGL((crafter_nearby_kernel<kNearThreads, 0>), grid, dim3(kNearThreads), lds, s, h->cfg, h->tb, h->st, mask, q, counts, ents, n);
  } else {
    if (map)
      hipLaunchKernelGGL((crafter_nearby_kernel<kNearWideThreads, 1>), grid, dim3(kNearWideThreads), lds, s, h->cfg, h->tb, h->st, mask, q, counts, ents, n);
    else
      hipLaunchKernelGGL((crafter_nearby_kernel<kNearWideThreads, 0>), grid, dim3(kNearWideThreads), lds, s, h->cfg, h->tb, h->st, mask, q, counts, ents, n);
  }
  return launched(h, "crafter_nearby launch");
}

// Edits of the n envs idx names, in place (env_edit.hpp): the index check of crafter_step_n_envs, then one workgroup per named
// env that replays its row of the tape.  Like crafter_save_envs it touches live rows only -- the pool's side streams never write
// them, and an edit leaves the pool's entries alone -- so it waits for no batch.  An ordered handle's next_step entries of the
// named envs follow a clock edit (the dispatch order's hint: stale it would cost time, never correctness).
int crafter_edit_envs(crafter_handle* h, const int32_t* idx, int32_t n, const int32_t* ops, int32_t ops_per_env, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (ready(h, "crafter_edit_envs")) return 1;
  if (n < 0 || n > h->cfg.num_envs) return fail(h, "crafter_edit_envs: n outside 0 .. num_envs");
  if (n == 0) return 0;
  if (!idx) return fail(h, "crafter_edit_envs: null index list");
  if (!ops) return fail(h, "crafter_edit_envs: null ops");
  if (ops_per_env < 1) return fail(h, "crafter_edit_envs: ops_per_env must be at least 1");
  if (((uintptr_t)ops & 15u) != 0) return fail(h, "crafter_edit_envs: ops must be 16-byte aligned");
  const int lds = edit_layout(h->cfg).total;   // (<= plan.render_lds: beyond 64 KB crafter_create has allowed the kernel that much, big_lds_kernels)
  if (adopt_stream(h, s)) return 1;
  if (need_scratch(h, (void**)&h->rollout_row_of, (size_t)h->cfg.num_envs * sizeof(int32_t), "crafter_edit_envs: row scratch")) return 1;
  RolloutEnvsCheck chk;
  chk.idx = idx; chk.n = n;
  if (index_check_scratch(h, "crafter_edit_envs", s, &chk.stamp)) return 1;
  chk.mark = h->copy_mark; chk.verdict = h->copy_verdict; chk.rec = (EnvRec*)h->st.rec; chk.rows = h->cfg.num_envs;
  chk.row_of = h->rollout_row_of;
  launch_rollout_envs_check(chk, s, nullptr, nullptr);
  hipLaunchKernelGGL(crafter_edit_envs_kernel, dim3((unsigned)n), dim3(kEditThreads), lds, s, h->cfg, h->tb, h->st, idx,
                     (const int32_t*)h->copy_verdict, ops, (int)ops_per_env, h->next_step);
  return launched(h, "crafter_edit_envs launch");
}

#ifdef CRAFTER_PROBES
// probe builds: the generation kernels' phase clocks (gen_bodies.hpp g_gen_probe), read and cleared; synchronises the device
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
  const hipStream_t s = (hipStream_t)stream;
  if (mode < 0 || mode > 3 || !x || !out || n < 0 || (mode == 0 && (!perm || !y || !z)))
    return fail(nullptr, "crafter_debug_eval: bad argument");
  if (n == 0) return 0;
  long long blocks = (n + kStepThreads - 1) / kStepThreads;
  hipLaunchKernelGGL(crafter_debug_eval_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(kStepThreads), 512 + kSimplexLdsBytes, s,
                     perm, x, y, z, out, (long long)n, mode);
  return launched(nullptr, "crafter_debug_eval launch");
}

const char* crafter_last_error(const crafter_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

}  // extern "C"
