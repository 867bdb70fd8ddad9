// Env.reset and what runs in the reset kernels: the reset skeleton and its callers, Env.render, the final-observation path.
#pragma once
#include "step_body.hpp"
#include "symbolic.hpp"

namespace crafter {

// Env.reset (env.py:70-81) around whatever makes the new world: world(e, L) is called by every thread with the env's record
// staged, and returns behind a barrier with the world in place and the wave-uniform registers (nobj, mt_pos) in every wave;
// then info['semantic'], the first frame (step 0: by day) and the write-back.  Its callers: reset_body (the generator),
// adopt_reset_body (the pool), reset_world_body (an authored world, env_worlds.hpp).  prof: the env's stamp row (8 / 14 / 15:
// start, frame drawn, stored) or null.  Returns the episode the env is now in.  S: element type of the slot map in THIS kernel's
// LDS (2 bytes in general, 1 for the default geometry's frame kernel, whose workgroups have the compact layout's room).
template <class W, class S, class F>
__device__ __forceinline__ int reset_skeleton(W& w, uint8_t* smem, int env, const Config& cfg, const TablePtrs& tb, const StatePtrs& st,
                                     uint8_t* obs, uint64_t* prof, F&& world) {
  LdsLayout L = sizeof(S) == 2 ? big_reset_layout(cfg) : lds_layout(cfg, (int)sizeof(S));   // (= lds_layout for LDS-resident maps)
  w.scratch = (uint32_t*)(smem + L.scratch);
  Env<W, S> e(w, cfg, tb, smem + L.rules);
  bind_lds<W, -1, S>(e, smem, L, st, env);
  const bool objs_in_place = L.objs < 0;
  if (prof && w.leader()) prof[8] = w.clock();
  RenderTarget rt = obs_target<W>(cfg, tb, obs, env);
  Renderer<W, S> r(e, rt, smem + L.render, (uint32_t*)(smem + L.mtb), L.frame_bytes ? smem + L.frame : nullptr);
  if (cfg.render_obs != 0 && obs != nullptr) r.preload();   // completes under the barriers below
  load_env(e, st, env, 0);
  world(e, L);
  if (cfg.want_semantic && st.semantic) write_semantic(e, st.semantic, env);
  if (L.frame_over_objs) store_objs(e, st, env);   // a night frame's pixel buffer reaches into the slot table
  w.sync();
  r.render(cfg.render_obs != 0 && obs != nullptr);   // may recycle the LDS map copies: keep it last
  w.sync();
  if (prof && w.leader()) prof[14] = w.clock();
  store_env(e, st, env, !L.frame_over_objs && !objs_in_place);
  if (prof && w.leader()) prof[15] = w.clock();
  return e.rec->episode;
}

// levels: the handle's level table (env_levels.hpp; null: none) -- here and in every body below that seeds a world.
template <class W, class S = uint16_t>
__device__ __forceinline__ int reset_body(W& w, uint8_t* smem, int env, const Config& cfg, const TablePtrs& tb,
                                 const StatePtrs& st, uint8_t* obs, int gen_parity, const LevelTable* levels = nullptr) {
  uint64_t* prof = st.prof ? st.prof + (size_t)env * 16 : nullptr;
  return reset_skeleton<W, S>(w, smem, env, cfg, tb, st, obs, prof, [&](Env<W, S>& e, const LdsLayout& L) {
    WorldGen<W, S> wg(e, smem + L.wg);
    wg.levels = levels;
    wg.reset_env(prof);
    e.recount_space();
    share_registers(e);
    request_generation(w, cfg, st, gen_parity, env, e.rec->episode + 2);
  });
}

// The regeneration kernel's half of a rollout: env stopped at step stalled_at[env] for want of a world.  Generate it
// (its first frame is that step's observation), run the env's remaining steps with the generic step instance, and
// should it finish another episode without a pooled world, generate that one here too.
template <class W>
__device__ __forceinline__ void requeue_rollout_body(W& w, uint8_t* smem, int env, const Config& cfg, const TablePtrs& tb,
                                            const StatePtrs& st, const int32_t* actions, uint8_t* obs, float* reward, uint8_t* done,
                                            const StepCtl& ctl, int T, size_t obs_stride, const int32_t* stalled_at,
                                            const LevelTable* levels = nullptr) {
  StatePtrs sq = st;
  sq.reset_q = nullptr;   // an env that stops again is not queued: it is regenerated right here
  size_t n = (size_t)cfg.num_envs;
  int t = stalled_at[env];
  for (;;) {
    reset_body<W>(w, smem, env, cfg, tb, st, obs ? obs + (size_t)t * obs_stride : nullptr, ctl.gen_parity, levels);
    w.sync();
    bool stopped = false;
    for (t = t + 1; t < T; t++) {
      stopped = (step_body<W, -1, 0, uint16_t>(w, smem, env, cfg, tb, sq, actions + (size_t)t * n, obs ? obs + (size_t)t * obs_stride : nullptr,
                                               reward + (size_t)t * n, done + (size_t)t * n, ctl) & kStepStopped) != 0;
      w.sync();
      if (stopped) {
        if (st.pool_stats && ctl.gen_parity >= 0 && w.leader()) w.global_add(st.pool_stats + 1, 1);
        break;
      }
    }
    if (!stopped) return;
  }
}

// Env.render() on the current state (env.py:120-130): re-draws the frame and, like the reference,
// consumes the night noise from the env's RNG again (engine.py:208-209).
template <class W>
__device__ __forceinline__ void render_body(W& w, uint8_t* smem, int env, const Config& cfg, const TablePtrs& tb,
                                   const StatePtrs& st, uint8_t* out, bool store = true) {
  LdsLayout L = lds_layout(cfg);
  w.scratch = (uint32_t*)(smem + L.scratch);
  Env<W> e(w, cfg, tb, smem + L.rules);
  bind_lds(e, smem, L, st, env);
  RenderTarget rt = obs_target<W>(cfg, tb, out, env);
  Renderer<W> r(e, rt, smem + L.render, (uint32_t*)(smem + L.mtb), L.frame_bytes ? smem + L.frame : nullptr);
  if (out != nullptr) r.preload();
  load_env(e, st, env, 1);
  r.render(out != nullptr);   // daylight[rec.step]
  if (!store) return;
  w.sync();
  store_env(e, st, env, !L.frame_over_objs);   // rendering changes no object; the pixel buffer may have reached into the LDS copy
}

// ---------------------------------------------------------------------------------------------
// crafter_step_final: the regeneration kernel's body when the caller wants the finished episode's last observation.  The step
// launch ran with StepCtl::gen_parity = -1, so EVERY env that finished took step_body's will_reset path: its complete terminal
// state is in global memory, it sits in reset_q and no frame has been drawn for it.  Here, per queued env:
//   terminated   1 if the player died (env.py:106-115: discount = 1 - dead), 0 if the episode only ran into `length`
//   final_local / final_stats   crafter_symbolic's pair of the terminal state (one wave: symbolic_body reads global state)
//   final_obs    env.py:96 obs = self._obs() on the terminal state, night noise from the finished episode's stream included
//                (engine.py:208-209; the new episode reseeds, env.py:74: nothing of these draws is stored)
// and then Env.reset as the step kernel / reset_body would have done it: a pooled world if one is ready, else inline.
struct FinalOut {
  uint8_t* obs = nullptr;          // [N][size_h][size_w][3] or null
  uint8_t* terminated = nullptr;   // [N]
  uint8_t* local = nullptr;        // [N][2][local_gw][local_gh] or null
  float* stats = nullptr;          // [N][n_items + 4] or null
};

// Env.reset from the pool under the reset kernels' layout (big_reset_layout: for worlds whose maps stay in global memory the
// slot table is written in place): reset_body with adopt_world where it generates.
template <class W, class S = uint16_t>
__device__ __forceinline__ void adopt_reset_body(W& w, uint8_t* smem, int env, const Config& cfg, const TablePtrs& tb, const StatePtrs& st,
                                        uint8_t* obs, int gen_parity, int episode) {
  reset_skeleton<W, S>(w, smem, env, cfg, tb, st, obs, nullptr, [&](Env<W, S>& e, const LdsLayout&) {
    adopt_world(e, st, env, episode);
    if (st.pool_stats && w.leader()) w.global_add(st.pool_stats + 0, 1);
    request_generation(w, cfg, st, gen_parity, env, episode + 2);
  });
}

template <class W>
__device__ __forceinline__ void final_reset_body(W& w, uint8_t* smem, int env, const Config& cfg, const TablePtrs& tb, const StatePtrs& st,
                                        uint8_t* obs, int gen_parity, uint32_t safe_seq, int32_t* next_step, const FinalOut& fo,
                                        const LevelTable* levels = nullptr) {
  if (w.leader()) fo.terminated[env] = st.rec[env].dead != 0 ? 1 : 0;
  if ((fo.local || fo.stats) && w.wave0()) {
    if (lds_layout(cfg).maps_in_lds)
      symbolic_body<W, 0>(w, smem, env, cfg, tb, st, nullptr, fo.local, fo.stats);
    else
      symbolic_body<W, 1>(w, smem, env, cfg, tb, st, nullptr, fo.local, fo.stats);
  }
  w.sync();
  if (cfg.render_obs != 0 && fo.obs != nullptr) {
    render_body(w, smem, env, cfg, tb, st, fo.obs, false);   // the terminal frame: the state as the step left it, the terminal step's daylight, nothing stored
    w.sync();
  }
  const int next_episode = st.rec[env].episode + 1;
  if (gen_parity >= 0 && pool_ready<W>(cfg, st, env, next_episode, safe_seq)) {
    adopt_reset_body<W>(w, smem, env, cfg, tb, st, obs, gen_parity, next_episode);
    if (next_step && w.leader()) next_step[env] = 1;   // (the new episode's first step: what step_body leaves behind an adoption)
  } else {
    if (st.pool_stats && gen_parity >= 0 && w.leader()) w.global_add(st.pool_stats + 1, 1);
    reset_body<W>(w, smem, env, cfg, tb, st, obs, gen_parity, levels);
  }
}

}  // namespace crafter
