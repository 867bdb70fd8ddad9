// Env.step: the launch parameters, the split step's frame record and frame half, step_body and the resident rollout_body.
#pragma once
#include "pool_entry.hpp"

namespace crafter {

// Per-step launch parameters of the world-pool protocol (pool_entry.hpp; host side: crafter_hip.hip).
struct StepCtl {
  int parity;          // which reset_q half this step appends to
  int gen_parity;      // which gen_q segment collects generation requests right now (-1: pool off)
  uint32_t safe_seq;   // newest generation batch whose completion the launch stream has waited on
  // Dispatch order (crafter_step_kernel only; all null: workgroup b steps env b).  A launch lasts as long as the envs
  // dispatched LAST need, and a night frame or a balance step takes twice a plain day step: with those dispatched first
  // the launch ends 8 us earlier.  Every step leaves the number of the env's next step in next_step[env];
  // one extra workgroup of every launch (block 0: dispatched first, done long before the others) sorts the envs for the
  // launch AFTER this one from what the launch BEFORE this one left there -- one step stale, nothing on the critical path.
  uint32_t* noise_raw = nullptr;    // [N][kNoiseStates * 624] the MT19937 states a night frame's noise comes from, generated ahead of
                                    // the rules (noise_chain); null: the frame regenerates them itself, epoch by epoch
  uint32_t* night_px = nullptr;     // [N][frame_night_px_words] scratch for a night frame's pixels (instances whose layout keeps none in LDS)
  int early_frame = 0;              // 1: the waves behind the first one draw the material half of a day frame while the object loop runs (render.hpp
                                    // early_frame): set by the host for crafter_step_early_kernel (batches of at least 2048 envs, where a shorter day
                                    // step is a shorter launch; where all envs are resident at once the launch ends with its night frames, which gain
                                    // nothing: profiles/r6_early_frame_ab.txt)
  const int32_t* order = nullptr;   // [N] workgroup b + 1 steps env order[b]
  int32_t* order_build = nullptr;   // [N] the order the next launch will use, written by block 0 of this one
  int32_t* next_step = nullptr;     // [N]
};

// ---------------------------------------------------------------------------------------------
// Split step (default geometry, default rules; crafter_hip.hip): the serial rule half of a step runs one WAVE per env
// (a 64-thread workgroup with 15 KB of LDS, ten to a CU), the frame half four waves per env with the renderer's tables but
// none of the env's maps.  What passes between them, besides the state itself (record, MT19937 state): the frame record,
// kFrameRecordBytes per env in the env's slice of StatePtrs.objmap (unused for LDS-resident worlds, whose slot map is
// derived state): for every cell of the view its material id (0xFF: outside the map) and its sprite's texture id (0xFF: none).
__device__ inline uint8_t* frame_record(const StatePtrs& st, const Config& c, int env) {
  return (uint8_t*)(st.objmap + (size_t)env * c.W * c.H);
}

// staging: kFrameRecordBytes of LDS the caller no longer needs once the view's materials have been read (LaneSlots: the window).
// returns whether the frame is a night frame
template <class W, class S>
__device__ __forceinline__ bool emit_frame_cells(Env<W, S>& e, const StatePtrs& st, int env, uint8_t* staging = nullptr, int hint_step = -1,
                                        double hint_D = 0.0) {
  const Config& c = e.cfg;
  W& w = e.w;
  uint8_t* rec = frame_record(st, c, env);
  Obj p = e.objs[1];
  int offx = c.local_gw / 2, offy = c.local_gh / 2;
  int ncell = c.local_gw * c.local_gh;
  bool sleeping = e.rec->sleeping != 0;
  if constexpr (Env<W, S>::kLane) {
    // (one wave) the record is put together in LDS -- lane registers first, the window is only overwritten when every
    // material has been read out of it -- and leaves in 8-byte stores, one per lane
    int px = p.x, py = p.y;
    w.lane_set(1, 0, ncell, [&](int k, int) -> uint32_t {
      int gx = k / c.local_gh, gy = k - gx * c.local_gh;
      int wx = px + gx - offx, wy = py + gy - offy;
      return (uint32_t)(e.inside(wx, wy) ? e.mat_at(wx, wy) : 0xFF);
    });
    w.lane_set(0, 0, ncell, [&](int, int) -> uint32_t { return 0xFFu; });
    w.occ_groups(
        e.nobj,
        [&](uint32_t pos) {
          int dx = (int)(pos & 0xFFFFu) - px + offx, dy = (int)(pos >> 16) - py + offy;
          return pos != 0xFFFFFFFFu && (unsigned)dx < (unsigned)c.local_gw && (unsigned)dy < (unsigned)c.local_gh;
        },
        [&](int g, uint64_t m) {
          while (m) {
            int slot = 64 * g + __builtin_ctzll(m);
            m &= m - 1;
            Obj o = e.objs[slot];
            w.lane_put(0, ((int)o.x - px + offx) * c.local_gh + ((int)o.y - py + offy), (uint32_t)sprite_texture(o, sleeping));
          }
        });
    int step = e.rec->step;
    double D = step == hint_step ? hint_D : e.tb.daylight[step];
    w.wsync();
    w.lanes(0, ncell, [&](int k, int lane) {
      staging[k] = (uint8_t)w.lane_get(1, lane);
      staging[kFrameSprites + k] = (uint8_t)w.lane_get(0, lane);
    });
    w.lanes(0, MAX_ITEMS, [&](int i, int) { staging[kFrameInventory + i] = (uint8_t)e.rec->inv[i]; });
    if (w.leader()) {
      staging[kFrameFlag] = 0;
      staging[kFrameSleeping] = (uint8_t)sleeping;
      *(double*)(staging + kFrameDaylight) = D;
      *(int32_t*)(staging + kFrameStep) = step;
      *(int32_t*)(staging + kFrameMtPos) = e.mt_pos;
      for (int i = kFrameMtPos + 4; i < kFrameRecordBytes; i += 4) *(int32_t*)(staging + i) = 0;
    }
    w.wsync();
    w.lanes(0, kFrameRecordBytes / 8, [&](int i, int) { ((uint64_t*)rec)[i] = ((const uint64_t*)staging)[i]; });
    return D < 0.5;
  } else {
    w.block_for(ncell, [&](int k) {
      int gx = k / c.local_gh, gy = k - gx * c.local_gh;
      int wx = (int)p.x + gx - offx, wy = (int)p.y + gy - offy;
      int m = 0xFF, sp = 0xFF;
      if (e.inside(wx, wy)) {
        int ci = e.cidx(wx, wy);
        m = e.mat[ci];
        int slot = e.objmap[ci];
        if (slot) sp = sprite_texture(e.objs[slot], sleeping);
      }
      rec[k] = (uint8_t)m;
      rec[kFrameSprites + k] = (uint8_t)sp;
    });
  }
  w.block_for(MAX_ITEMS, [&](int i) { rec[kFrameInventory + i] = (uint8_t)e.rec->inv[i]; });
  if (w.leader()) {
    rec[kFrameFlag] = 0;
    rec[kFrameSleeping] = (uint8_t)sleeping;
    int step = e.rec->step;
    *(double*)(rec + kFrameDaylight) = e.tb.daylight[step];
    *(int32_t*)(rec + kFrameStep) = step;
    *(int32_t*)(rec + kFrameMtPos) = e.mt_pos;
  }
  return e.tb.daylight[e.rec->step] < 0.5;
}

// The frame half of a split step: env.py:96 obs = self._obs() from the frame record, the env's record (step, sleeping,
// inventory) and -- at night -- its MT19937 stream, which it advances and stores back.
template <class W>
__device__ __forceinline__ void frame_body(W& w, uint8_t* smem, int env, const Config& cfg, const TablePtrs& tb, const StatePtrs& st,
                                  uint8_t* obs, uint32_t* night_px) {
  W::set_priority_mid();
  FrameLayout F = frame_layout(cfg);
  w.scratch = (uint32_t*)(smem + F.scratch);
  Env<W, uint8_t> e(w, cfg, tb, typename Env<W, uint8_t>::DefaultRulesTag{});
  e.mat = nullptr;
  e.objmap = nullptr;
  e.objs = nullptr;
  e.g_mat = nullptr;
  e.g_objmap = nullptr;
  e.rec = (EnvRec*)(smem + F.rec);
  e.mt = (uint32_t*)(smem + F.mt);
  RenderTarget rt = obs_target<W>(cfg, tb, obs, env);
  Renderer<W, uint8_t> r(e, rt, smem + F.render, (uint32_t*)(smem + F.mtb), (uint8_t*)(night_px + (size_t)env * frame_night_px_words(cfg)));
  r.pix_global = true;
  r.frame_cells = smem + F.cells;
  const uint8_t* cells = smem + F.cells;
  uint64_t* prof = st.prof ? st.prof + (size_t)env * 16 : nullptr;   // stamps 14 / 15 / (renderer: 7, 8, 12, 13) / 6: start, staged, ..., done
  r.prof = prof;
  if (prof && w.leader()) prof[14] = w.clock();
  {   // stage-in: the frame record and the static tables
    uint32_t qcells[1];
    typename Renderer<W, uint8_t>::Preload qr;
    const uint32_t* gcells = (const uint32_t*)frame_record(st, cfg, env);
    stage_issue(w, qcells, gcells, kFrameRecordBytes / 4);
    r.preload_issue(qr);
    stage_commit(w, qcells, (uint32_t*)(smem + F.cells), gcells, kFrameRecordBytes / 4);
    r.preload_commit(qr);
    w.sync();
  }
  if (cells[kFrameFlag]) return;   // (uniform: the whole workgroup leaves) the regeneration kernel draws this env's frame
  if (prof && w.leader()) prof[15] = w.clock();
  int step = *(const int32_t*)(cells + kFrameStep);
  double D = *(const double*)(cells + kFrameDaylight);
  bool sleeping = cells[kFrameSleeping] != 0;
  bool night = D < 0.5;
  // the few fields of the env's record a frame reads
  if (w.leader()) {
    e.rec->step = step;
    e.rec->sleeping = sleeping;
    e.rec->mt_pos = *(const int32_t*)(cells + kFrameMtPos);
  }
  w.block_for(MAX_ITEMS, [&](int i) { e.rec->inv[i] = cells[kFrameInventory + i]; });
  if (night) {   // only a night frame needs the stream
    const uint4* gmt = (const uint4*)(st.mt + (size_t)env * MT_N);
    uint4* lmt = (uint4*)e.mt;
    w.block_for(MT_N / 4, [&](int i) { lmt[i] = gmt[i]; });
  }
  w.sync();
  e.mt_pos = e.rec->mt_pos;
  e.nobj = 0;
  r.render(true, step, D);
  if (night) {   // it consumed noise: the stream goes back
    w.sync();
    uint4* gmt = (uint4*)(st.mt + (size_t)env * MT_N);
    const uint4* lmt = (const uint4*)e.mt;
    w.block_for(MT_N / 4, [&](int i) { gmt[i] = lmt[i]; });
    if (w.leader()) st.rec[env].mt_pos = e.mt_pos;
  }
  if (prof && w.leader()) prof[6] = w.clock();
}

// What step_body returns (bits): the env finished its episode and found no world in the pool (it then sits in the
// regeneration queue and this step has not drawn its observation: reset_body will) | the frame it drew recycled the LDS
// copies of the maps (a night frame's pixel buffer: render.hpp) -- only of interest to a caller that keeps the state in LDS.
enum : uint32_t { kStepStopped = 1u, kStepMapsGone = 2u };
// `res` of a RESIDENT step (RES = 1, rollout_body): the env's state stays in LDS from one step of a workgroup to its next.
//   kResLoaded  the state is in LDS already (the step before left it there): nothing but what a frame consumes is staged again
//   kResKeep    leave it there (no write-back to global memory, unless the env stops)
//   kResMapsGone  (with kResLoaded) the step before drew a night frame over the LDS copies of the maps: they come back from
//               global memory (the material map is written through as the rules run; the slot table was stored before the frame)
enum : uint32_t { kResLoaded = 1u, kResKeep = 2u, kResMapsGone = 4u };

template <class W, int LM = -1, int RUL = 0, class S = uint16_t, int SPLIT = 0, int RES = 0>
__device__ __forceinline__ uint32_t step_body(W& w, uint8_t* smem, int env, const Config& cfg, const TablePtrs& tb, const StatePtrs& st,
                                     const int32_t* actions, uint8_t* obs, float* reward, uint8_t* done, const StepCtl& ctl, uint32_t res = 0,
                                     int action_fetched = 0);

// SPLIT 1: the rule half of a split step (crafter_rules_kernel): no frame; the frame's inputs -- what each cell of the view
// shows -- are left in the env's frame record for frame_body (crafter_frame_kernel).
template <class W, int LM, int RUL, class S, int SPLIT, int RES>   // RUL 1: the rules are kDefaultRules (compile-time constants)
__device__ __forceinline__ uint32_t step_body(W& w, uint8_t* smem, int env, const Config& cfg, const TablePtrs& tb,
                                     const StatePtrs& st, const int32_t* actions, uint8_t* obs, float* reward,
                                     uint8_t* done, const StepCtl& ctl, uint32_t res, int action_fetched) {
  static_assert(!RES || !SPLIT, "resident steps are fused steps");
  W::set_priority_mid();   // above background generation; the serial rule phase of wave 0 goes higher still
  static_assert(!Env<W, S>::kLane || (SPLIT != 0 && RUL != 0), "LaneSlots is the rule kernel's layout: split step, compiled-in rules");
  static_assert(Env<W, S>::kFar == (LM == 0 && !SPLIT), "FarSlot is big_layout's slot type: the instance whose maps and slot table stay in global memory");
  LdsLayout L = Env<W, S>::kLane ? lane_layout(cfg) : (LM == 0 && !SPLIT) ? big_layout(cfg) : lds_layout(cfg, (int)sizeof(S), SPLIT != 0, !(RUL && !SPLIT));
  w.scratch = (uint32_t*)(smem + L.scratch);
  uint64_t* prof = st.prof ? st.prof + (size_t)env * 16 : nullptr;
  auto stamp = [&](int k) {
    if (prof && w.leader()) prof[k] = w.clock();
  };
  stamp(0);
  Env<W, S> e_staged(w, cfg, tb, smem + (RUL ? 0 : L.rules));
  Env<W, S> e_const(w, cfg, tb, typename Env<W, S>::DefaultRulesTag{});
  Env<W, S>& e = RUL ? e_const : e_staged;
  bind_lds<W, LM, S>(e, smem, L, st, env);
#ifdef CRAFTER_BALANCE_PROBE
  e.bal_prof = prof;
#endif
  RenderTarget rt = obs_target<W>(cfg, tb, obs, env);
  // (split: no renderer region in LDS; the object only serves the pixel-less night pass of render-off configurations)
  Renderer<W, S> r(e, rt, SPLIT ? nullptr : smem + L.render, SPLIT ? nullptr : (uint32_t*)(smem + L.mtb),
                   (!SPLIT && L.frame_bytes) ? smem + L.frame : nullptr);
  if (LM == 0 && !SPLIT && ctl.night_px) {   // big_layout: a night frame's pixels wait in the env's global scratch
    r.pix = ctl.night_px + (size_t)env * frame_night_px_words(cfg);
    r.pix_global = true;
  }
  r.prof = prof;
  const bool draw_here = !SPLIT && cfg.render_obs != 0 && obs != nullptr;   // this kernel draws the frame itself
  const bool ahead_possible = draw_here && ctl.noise_raw != nullptr && !Env<W, S>::kLane && W::kThreads >= 128;
  e.count_twists = ahead_possible;
  // the material half of a day frame is drawn by the waves behind the first one while the object loop runs (render.hpp early_frame)
  // (the CPU harness runs the run-time-layout instance, LM -1: there too, so that the path is covered without a GPU)
  const bool early_possible = W::kEarlyFrame && ctl.early_frame != 0 && ahead_possible && !RES && !SPLIT && (LM == 1 || (LM == -1 && !W::kConcurrentWaves && L.maps_in_lds != 0));
  // read before the stage-in: its latency hides under it.  A resident step has no stage-in to hide it under -- the rule wave
  // would wait a whole memory round trip for its action: the caller fetched it a step ago (rollout_body)
  int action_in = (RES && (res & kResLoaded)) ? action_fetched : actions[env];
  if (RES && (res & kResLoaded)) {
    // The state is where the step before left it, the noise look-ahead's copy of the stream state included (made at the end
    // of that step).  ONE barrier -- the frame before is through with the tables and the pixel buffer -- and the rule wave is
    // on its way: it waits for no load.  What a frame consumes and the frame before spoiled is staged again by the waves
    // that would otherwise wait for the rules: the renderer's static block (a day frame lights its rows in place) -- and,
    // behind a night frame, the maps (by everybody: the rules need them).
    w.sync();
    if (res & kResMapsGone) restage_maps(e, st, env, L.frame_over_objs != 0);   // (ends on a barrier)
    if (draw_here) r.preload_beside(false);   // (the material rows: stage_rows below)
    e.mt_pos = e.rec->mt_pos;
    e.nobj = e.rec->nobj;
    e.dirty_slots = 0;
    if constexpr (Env<W, S>::kFar) {   // the player has moved, objects have come and gone: the scan again (the table is current)
      e.far_clear();
      e.far_issue(w.wave_index());
      e.far_publish();
      w.sync();
      far_finish_scan(e);
    }
  } else {   // stage-in: every load of the state and of the renderer's static tables in flight at once
    bool draw = draw_here;
    if (early_possible) w.block_for(4, [&](int i) { r.hdr[i] = 0u; });   // (the early frame's hand-shake words: ahead of the stage-in's barrier)
    EnvStage<W, 1, Env<W, S>::kFar ? 2 : 1> qs;   // (the instance whose maps stay in HBM does not stage its slot table at all: Env::far_issue; its chunk tables are long)
    typename Renderer<W, S>::Preload qr;
    load_env_issue(e, st, env, 1, qs);
    if (draw) r.preload_issue(qr, false);
    load_env_commit(e, st, env, 1, qs, ahead_possible ? r.mtb : nullptr);   // the barrier inside only needs the state ...
    if (draw) r.preload_commit(qr, false);       // ... the tables are not read before the render's own barriers
  }
  stamp(1);
  // daylight of the step about to run, fetched now so the latency hides under the rule code
  const uint32_t staged_word = w.scratch[1];   // (the counter AS STAGED, and whether the player sleeps: see load_env_commit -- NOT e.rec->step, which wave 0 is about to overwrite)
  int step_now = (int)(staged_word & 0xFFFFFFu) + 1;
  if (step_now >= cfg.n_daylight) step_now = cfg.n_daylight - 1;
  double daylight_now = tb.daylight[step_now];
  // the material rows of the frame's row table -- by day lit, for this step, straight from the table -- by the waves that
  // would otherwise wait for the rules
  if (draw_here) w.consumers([&] { r.stage_rows(step_now, daylight_now, (staged_word >> 24) != 0u); });
  // a night step whose frame this workgroup draws: wave 1 generates the frame's noise states while wave 0 runs the rules
  uint32_t* noise_out = ahead_possible ? ctl.noise_raw + (size_t)env * (kNoiseStates * MT_N) : nullptr;
  // (only wave 1 asks, with a load of its own: wave 0 must not wait for a daylight value at the head of its rule phase)
  if (ahead_possible && w.wave_is(1)) {
    if (W::agent_load((const uint64_t*)(tb.daylight + step_now)) < 0x3FE0000000000000ull)   // 0 <= daylight < 0.5, compared as bits
      noise_chain(w, r.mtb, noise_out);
  }
  const bool staged_asleep = (staged_word >> 24) != 0u;
  if (early_possible && W::kConcurrentWaves) w.consumers([&] { r.early_frame(step_now, daylight_now, staged_asleep); });   // (waits for the rule wave's signal below)
  if (w.wave0()) {
    W::set_priority_high();   // the wave-uniform rule code is the critical path of the whole workgroup
    int action = action_in;
    uint32_t bad = 0;
    if (action < 0 || action >= e.R.n_actions) {
      bad |= ST_BAD_ACTION;
      action = 0;
    }
    int step = e.rec->step + 1;  // env.py:84
    if (step >= cfg.n_daylight) {
      bad |= ST_STEP_OVERFLOW;
      step = cfg.n_daylight - 1;
    }
    if (bad) e.st(&e.rec->status, e.rec->status | bad);
    e.st(&e.rec->step, step);
    w.wsync();
    e.update_all(action, prof, [&] {         // env.py:86-89
      if (!early_possible) return;
      if (W::kConcurrentWaves) {
        e.st(&r.hdr[0], 1u);                 // Player.update has run: the other waves start on the frame
      } else {
        r.early_frame(step_now, daylight_now, staged_asleep);
      }
    });
    stamp(2);
    if (step % 10 == 0) e.balance(daylight_now);   // env.py:90-95
    e.compact();
    e.finish_step(reward + env, done + env, cfg.reward);
    if constexpr (Env<W, S>::kFar) W::drain_stores();   // (the frame's waves read table records straight from the coherence point: Env::obj_rd_lane)
    stamp(3);
    W::set_priority_mid();
  }
  share_registers(e);
  if (st.terminal && e.rec->done) {   // the finished episode's totals survive the auto-reset here
    int32_t* t = st.terminal + (size_t)env * (MAX_ACH + 4);
    w.block_for(MAX_ACH, [&](int i) { t[i] = e.rec->ach[i]; });
    if (w.leader()) {
      t[MAX_ACH + 0] = e.rec->step;
      t[MAX_ACH + 1] = e.rec->ep_dhealth;
      t[MAX_ACH + 2] = e.rec->ep_unlock_steps;
      t[MAX_ACH + 3] = e.rec->episode;
    }
    w.sync();
  }
  bool will_reset = e.rec->needs_reset != 0;
  if (will_reset) {
    int next_episode = e.rec->episode + 1;
    if (ctl.gen_parity >= 0 && pool_ready<W>(cfg, st, env, next_episode, ctl.safe_seq)) {
      adopt_world(e, st, env, next_episode);             // Env.reset from the pool
      if (st.pool_stats && w.leader()) w.global_add(st.pool_stats + 0, 1);
      stamp(6);
      request_generation(w, cfg, st, ctl.gen_parity, env, next_episode + 2);
      will_reset = false;                                // falls through to the first-frame render
    } else if (st.reset_q && w.leader()) {               // queue this env for the regeneration kernel
      int32_t* q = st.reset_q + (size_t)ctl.parity * (cfg.num_envs + 4);
      int k = w.global_add(q, 1);
      q[4 + k] = env;
      if (st.pool_stats && ctl.gen_parity >= 0) w.global_add(st.pool_stats + 1, 1);
    }
  }
  bool objs_stored = false;
  uint32_t ret = will_reset ? kStepStopped : 0u;
  if (!will_reset) {
    // env.py:96 obs = self._obs(); an env handed to reset_body gets its obs there
    if (cfg.want_semantic && st.semantic) write_semantic(e, st.semantic, env);
    // A night frame's pixel buffer reaches into the slot table: its final content goes out first.  Only then -- stores
    // issued here would be in the memory pipeline ahead of the frame's own loads, which return in order behind them.
    bool maybe_night = !(daylight_now >= 0.5) || e.rec->step != step_now;   // (an adopted world starts at step 0)
    if (!SPLIT && L.frame_over_objs && maybe_night) {
      store_objs(e, st, env);
      objs_stored = true;
    }
    // (no barrier here: share_registers / adopt_world ended on one and nothing has written LDS since)
    stamp(11);
    if (SPLIT && cfg.render_obs != 0 && obs != nullptr)
      emit_frame_cells(e, st, env, smem + L.mat, step_now, daylight_now);   // the frame kernel draws
    else {
      if (ahead_possible && daylight_now < 0.5 && e.rec->step == step_now) {   // (not a world adopted in this very step: that one is at step 0, by day)
        r.noise_raw = noise_out;
        r.noise_base = e.rng_twists * MT_N + e.mt_pos;   // where the rules left the stream, counted from the staged state's first word
      }
      // (a night frame in quad mode leaves its pixels in L.frame -- the LDS copies of the maps -- whether its noise was
      // generated ahead or not; a frame in direct mode, or one that only advances the stream, touches none of it)
      if (RES && draw_here && L.frame_bytes && !r.pix_global && (e.rec->step == step_now ? daylight_now : e.tb.daylight[e.rec->step]) < 0.5) ret |= kStepMapsGone;
      if (draw_here) r.rows_staged(step_now, daylight_now, (w.scratch[1] >> 24) != 0u);   // (the word is as it was: nothing rewrites it before the step's tail)
      // an early frame stands if every drawing wave finished it, no material changed behind it and the env is still in the
      // step it was drawn for (an adopted world is at step 0)
      bool drawn = false;
      if (early_possible && r.early_frame_drawn() && !e.mat_dirty && e.rec->step == step_now) drawn = r.finish_day_frame(daylight_now);
      if (!drawn) r.render(draw_here, step_now, daylight_now);   // may recycle the LDS map copies: keep it last
    }
  } else if (SPLIT == 1) {
    if (w.leader()) frame_record(st, cfg, env)[kFrameFlag] = 1;   // no frame from this step: the regeneration kernel draws the reset frame
  }
  // (nor here: store_env's own barrier separates the frame's LDS traffic from the write-back)
  stamp(4);
  if (ctl.next_step && w.leader()) ctl.next_step[env] = e.rec->step + 1;   // (0 + 1 in a world just adopted)
  if (RES && (res & kResKeep) && !will_reset) {
    // resident: the wave-uniform registers go back into the LDS record (the next step of this workgroup reads them there,
    // behind its first barrier), and so does the step counter as the other waves will want it (load_env_commit)
    if ((ret & kStepMapsGone) && L.frame_over_objs && !objs_stored) store_objs(e, st, env);   // (never: a night frame stored them above)
    if (w.leader()) {
      e.rec->mt_pos = e.mt_pos;
      e.rec->nobj = e.nobj;
      w.scratch[1] = (uint32_t)e.rec->step | (e.rec->sleeping != 0 ? 1u << 24 : 0u);
    }
    // ... and the stream state as the NEXT step's noise look-ahead will want it (noise_chain twists a copy while the rule
    // wave draws from the original).  Element i by the thread that wrote element i of the state if this frame put it there
    // (Renderer::render, `ahead`); every other writer of the state is a barrier away.
    if (ahead_possible) {
      const vec16* src = (const vec16*)e.mt;
      vec16* dst = (vec16*)r.mtb;
      w.block_for(MT_N / 4, [&](int i) { dst[i] = src[i]; });
    }
  } else {
    store_env(e, st, env, !objs_stored, RES == 0);   // (a resident stretch stores the state array whatever this step did: an earlier one may have rewritten it)
  }
  stamp(5);
  return ret;
}

// Open-loop rollout (crafter_step_n): T consecutive steps of ONE env by one workgroup, actions[t][env] known in advance
// (random / scripted policies, action repeat, planning over fixed action sequences) -- envs are independent, so nothing but
// the API forces all of them through step t before any starts step t + 1, and without that barrier a launch ends with the
// slowest SUM of T steps instead of T times with the slowest step.  Step t's outputs go to obs + t * obs_stride,
// reward + t * N, done + t * N.  An env that finishes an episode and finds no world in the pool (all but never) cannot go
// on here: it is queued for the regeneration kernel as in a single step and records the step it stopped at;
// requeue_rollout_body (below) regenerates it and runs the rest of its steps.
template <class W, int LM, int RUL, class S>
__device__ __forceinline__ void rollout_body(W& w, uint8_t* smem, int env, const Config& cfg, const TablePtrs& tb,
                                    const StatePtrs& st, const int32_t* actions, uint8_t* obs, float* reward, uint8_t* done,
                                    const StepCtl& ctl, int T, size_t obs_stride, int32_t* stalled_at) {
  size_t n = (size_t)cfg.num_envs;
  // The env's working set is staged in ONCE, stays in LDS over the T steps and is written back once (round 5: a store +
  // stage-in per step was 5 k of a step's 32 k clocks and 3.5 x the compulsory reads); per step only the outputs leave --
  // frame, reward, done, map cells written through -- and the renderer's static block comes in again (a day frame lights
  // its rows in place).  A night frame's pixel buffer recycles the LDS copies of the maps: they are staged again behind it.
  uint32_t carry = 0;   // what the step before left: kResLoaded | kResMapsGone
  int action_next = 0;  // the action of the step after the one running, fetched while that one runs
  uint64_t* prof = st.prof ? st.prof + (size_t)env * 16 : nullptr;   // stamps 14 / 15: the workgroup's first / last clock (the steps' own stamps: the last step's survive)
  if (prof && w.leader()) prof[14] = w.clock();
#pragma clang loop unroll(disable)
  for (int t = 0; t < T; t++) {
    // As far as the optimiser can tell every step has a new thread index and a new env: inlined into a plain loop it
    // hoists what a step computes from them out of the loop and keeps it in registers across the steps (251 VGPRs against
    // the step kernel's 71: two workgroups per CU instead of five).
    w.refresh();
    int env_t = W::opaque(env);
    uint32_t res = carry | (t + 1 < T ? (uint32_t)kResKeep : 0u);
    int action_now = action_next;
    action_next = actions[(size_t)(t + 1 < T ? t + 1 : t) * n + env_t];
    uint32_t got = step_body<W, LM, RUL, S, 0, 1>(w, smem, env_t, cfg, tb, st, actions + (size_t)t * n, obs ? obs + (size_t)t * obs_stride : nullptr,
                                                   reward + (size_t)t * n, done + (size_t)t * n, ctl, res, action_now);
    if (got & kStepStopped) {   // (its state went to global memory: the regeneration kernel takes the env from there)
      if (w.leader()) stalled_at[env_t] = t;
      return;
    }
    carry = kResLoaded | ((got & kStepMapsGone) ? (uint32_t)kResMapsGone : 0u);
  }
  if (prof && w.leader()) prof[15] = w.clock();
}

}  // namespace crafter
