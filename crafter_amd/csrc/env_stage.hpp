// HBM <-> LDS staging of one env's working set under an LdsLayout, and the small pieces every body shares around it.
#pragma once
#include "lds_layout.hpp"

namespace crafter {

// LM: 1 / 0 = the caller knows at compile time that the maps are LDS-resident / stay in HBM, -1 = decided at run
// time.  It matters for the step kernel: with a run-time choice the map pointers are address-space-unknown and
// every map access of the rule code becomes a FLAT instruction instead of a DS one.
template <class W, int LM = -1, class S = uint16_t>
__device__ __forceinline__ void bind_lds(Env<W, S>& e, uint8_t* smem, const LdsLayout& L, const StatePtrs& st, int env) {
  const Config& c = e.cfg;
  size_t cells = (size_t)c.W * c.H;
  e.g_mat = st.mat + (size_t)env * cells;
  // The slot map (cell -> slot) of an LDS-resident world is derived state: rebuilt from the slot table
  // at stage-in, never written back (StatePtrs.objmap is only live for worlds whose maps stay in HBM).
  if constexpr (Env<W, S>::kLane) {
    e.g_objmap = nullptr;
    e.mat = smem + L.mat;   // the window (load_env_issue decides where it sits)
    e.objmap = nullptr;
  } else if (LM == 1) {
    e.g_objmap = nullptr;
    e.mat = smem + L.mat;
    e.objmap = (S*)(smem + L.objmap);
  } else if (LM == 0) {
    e.g_objmap = st.objmap + (size_t)env * cells;
    e.mat = e.g_mat;
    e.objmap = (S*)e.g_objmap;   // LM == 0 implies S == uint16_t
  } else {
    e.g_objmap = L.maps_in_lds ? nullptr : st.objmap + (size_t)env * cells;
    e.mat = L.maps_in_lds ? smem + L.mat : e.g_mat;
    e.objmap = L.maps_in_lds ? (S*)(smem + L.objmap) : (S*)e.g_objmap;
  }
  e.objs = L.objs >= 0 ? (Obj*)(smem + L.objs) : st.objs + (size_t)env * c.max_objects;   // (big_reset_layout, big_layout: in place)
  if constexpr (Env<W, S>::kFar) {
    e.nctr = (uint32_t*)(smem + L.far);
    e.ndm = smem + L.far + 16;
    e.ncache = (Obj*)(smem + L.far + 16 + 256);
    e.near_mask = (uint64_t*)(smem + L.far + 16 + 256 + 16 * kFarCache);
  }
  e.mt = (uint32_t*)(smem + L.mt);
  e.rec = (EnvRec*)(smem + L.rec);
  e.chunk_order = (uint16_t*)(smem + L.chunk_order);
  e.chunk_seen = smem + L.chunk_seen;
  if (L.census >= 0) {
    e.census = (int32_t*)(smem + L.census);
  } else {   // big_layout: the census is read and updated in place
    e.census = st.census + (size_t)env * c.nchunk_x * c.nchunk_y * 5;
    e.census_global = true;
  }
}

// The LDS copies of an LDS-resident world's maps, by every thread, no barrier:
// the material map from global memory, 16 bytes at a time where its size allows, else byte by byte
template <class W, class S>
__device__ __forceinline__ void copy_map_in(Env<W, S>& e) {
  int cells = e.cfg.W * e.cfg.H;
  if (cells % 16 == 0) {
    const uint4* gm = (const uint4*)e.g_mat;
    uint4* lm = (uint4*)e.mat;
    e.w.block_for(cells / 16, [&](int i) { lm[i] = gm[i]; });
  } else {
    e.w.block_for(cells, [&](int i) { e.mat[i] = e.g_mat[i]; });
  }
}
// the slot map (cell -> slot), emptied the same way ...
template <class W, class S>
__device__ __forceinline__ void clear_slot_map(Env<W, S>& e) {
  int cells = e.cfg.W * e.cfg.H;
  if ((cells * (int)sizeof(S)) % 16 == 0) {
    uint4 z;
    z.x = z.y = z.z = z.w = 0;
    uint4* lo = (uint4*)e.objmap;
    e.w.block_for(cells * (int)sizeof(S) / 16, [&](int i) { lo[i] = z; });
  } else {
    e.w.block_for(cells, [&](int i) { e.objmap[i] = 0; });
  }
}
// ... and derived from the first nobj records of the slot table (behind a barrier: the map is empty, the records are in LDS)
template <class W, class S>
__device__ __forceinline__ void derive_slot_map(Env<W, S>& e, int nobj) {
  e.w.block_for(nobj, [&](int i) {
    Obj o = e.objs[i];
    if (i >= 1 && o.type != T_NONE) e.objmap[e.cidx(o.x, o.y)] = (S)i;
  });
}

// HBM -> LDS in the two phases of stage_issue / stage_commit (env_core.hpp): every load of the env's
// state is in flight before the first one is waited for.
// everything: 1 = the whole state (step, render), 0 = only the scalar record (reset overwrites the rest)
// Registers per thread and array: sized for the default configuration's arrays at W's workgroup width, so that nothing
// falls through to stage_rest's byte loop (256 threads: one each; the split step's 64-thread rule kernel: up to four).
// OM: registers per thread for the slot table's blind prefix (OM x threads slots: 1 -- at most kBlindSlots of them -- for worlds
// of a few dozen objects; 4 for the instance whose maps stay in HBM: a 256x256 world holds ~750, and what the prefix misses
// costs a second memory round trip behind a barrier at the head of every step)
// CK: registers per thread for the two chunk tables (2 for worlds of up to 512 chunks -- 256x256: 484 --, whose tables' second half
// used to come by stage_rest's loop: two more memory round trips in a row at the head of every step, 5 k of its 10 k clocks: round 6)
template <class W, int OM = 1, int CK = 1>
struct EnvStage {
  static constexpr int M = W::kThreads >= 256 ? 1 : (256 + W::kThreads - 1) / W::kThreads;
  static constexpr int kObjRegs = OM > M ? OM : M;
  uint32_t rec[M];
  uint32_t rules[M];
  vec16 mat[M];
  vec16 mt[M];   // 624 words = 156 x 16 B: one vector load per thread of 256
  uint16_t chunk_order[CK];
  uint8_t chunk_seen[CK];
  int32_t census[M];
  vec16 objs[kObjRegs];
  uint64_t win[(kWinX * kWinY / 8 + W::kThreads - 1) / W::kThreads];   // LaneSlots: the material window, 8 bytes per load
};
#ifndef CRAFTER_BLIND_SLOTS
#define CRAFTER_BLIND_SLOTS 64
#endif
constexpr int kBlindSlots = CRAFTER_BLIND_SLOTS;   // the slot table's length is in the record that is still in flight: this
                                                   // many slots are fetched blindly with it

template <int OM>
__host__ __device__ constexpr int blind_slots(int max_objects, int nthreads) {
  return OM > 1 ? (max_objects < OM * nthreads ? max_objects : OM * nthreads) : (max_objects < kBlindSlots ? max_objects : kBlindSlots);
}
template <class W, class S, int OM, int CK>
__device__ __forceinline__ void load_env_issue(Env<W, S>& e, const StatePtrs& st, int env, int everything, EnvStage<W, OM, CK>& q) {
  const Config& c = e.cfg;
  W& w = e.w;
  int cells = c.W * c.H;
  int nch = c.nchunk_x * c.nchunk_y;
  uint32_t ppos = 0;
  if constexpr (Env<W, S>::kLane) {
    // The window is centred on the player, whose position sits in the slot table that is about to be fetched: ONE word
    // of it is asked for first (loads return in order: it is the shortest wait there is) and the window's loads join
    // the others once it is known.
    if (everything) ppos = ((const uint32_t*)(st.objs + (size_t)env * c.max_objects + 1))[1];
  }
  stage_issue(w, q.rec, (const uint32_t*)(st.rec + env), (int)(sizeof(EnvRec) / 4));
  if (e.rules_staged) stage_issue(w, q.rules, (const uint32_t*)e.tb.rules, CRAFTER_RULES_HEAD_BYTES / 4);
  if (!everything) return;
  if constexpr (!Env<W, S>::kLane)
    if (e.mat != e.g_mat && cells % 16 == 0) stage_issue(w, q.mat, (const vec16*)e.g_mat, cells / 16);
  stage_issue(w, q.mt, (const vec16*)(st.mt + (size_t)env * MT_N), MT_N / 4);
  stage_issue(w, q.chunk_order, st.chunk_order + (size_t)env * nch, nch);
  stage_issue(w, q.chunk_seen, st.chunk_seen + (size_t)env * nch, nch);
  if (!e.census_global) stage_issue(w, q.census, st.census + (size_t)env * nch * 5, nch * 5);
  if constexpr (Env<W, S>::kFar)
    e.far_issue(w.wave_index());   // (the slot table is not staged: the scan's first round, blind)
  else
    stage_issue(w, q.objs, (const vec16*)(st.objs + (size_t)env * c.max_objects), blind_slots<OM>(c.max_objects, W::kThreads));
  if constexpr (Env<W, S>::kLane) {
    place_window(e, (int)(ppos & 0xFFFFu), (int)(ppos >> 16));
    window_issue(e, e.g_mat, q.win);
  }
}

// LaneSlots: where the material window sits for a player at (px, py): inside the map, rows 8-byte aligned.
template <class W, class S>
__device__ __forceinline__ void place_window(Env<W, S>& e, int px, int py) {
  const Config& c = e.cfg;
  int x0 = px - kWinR, y0 = (py - kWinR) & ~7;
  x0 = x0 < 0 ? 0 : (x0 > c.W - kWinX ? c.W - kWinX : x0);
  y0 = y0 < 0 ? 0 : (y0 > c.H - kWinY ? c.H - kWinY : y0);   // H and kWinY are multiples of 8: stays aligned
  e.win_x0 = W::uni(x0);
  e.win_y0 = W::uni(y0);
}
// ... and its loads / LDS stores: row r of the window = kWinY bytes of row win_x0 + r of `src` (a whole map, x * H + y)
template <class W, class S, int K>
__device__ __forceinline__ void window_issue(Env<W, S>& e, const uint8_t* src, uint64_t (&r)[K]) {
  constexpr int per_row = kWinY / 8, n = kWinX * per_row;
#pragma unroll
  for (int k = 0; k < K; k++) {
    int j = e.w.tid() + k * e.w.nthreads();
    j = j < n ? j : n - 1;
    int row = j / per_row, col = j - row * per_row;
    r[k] = *(const uint64_t*)(src + (size_t)(e.win_x0 + row) * e.cfg.H + e.win_y0 + 8 * col);
  }
}
template <class W, class S, int K>
__device__ __forceinline__ void window_commit(Env<W, S>& e, const uint8_t* src, const uint64_t (&r)[K]) {
  constexpr int per_row = kWinY / 8, n = kWinX * per_row;
#pragma unroll
  for (int k = 0; k < K; k++) {
    int j = e.w.tid() + k * e.w.nthreads();
    if (j < n) ((uint64_t*)e.mat)[j] = r[k];
  }
  for (int j = K * e.w.nthreads() + e.w.tid(); j < n; j += e.w.nthreads()) {   // (narrower workgroups than the registers cover: the CPU harness)
    int row = j / per_row, col = j - row * per_row;
    ((uint64_t*)e.mat)[j] = *(const uint64_t*)(src + (size_t)(e.win_x0 + row) * e.cfg.H + e.win_y0 + 8 * col);
  }
}

// the scan's second half, behind the barrier that published the record and the player's position: the scan's batches are
// evaluated.  Ends on a barrier.
template <class W, class S>
__device__ __forceinline__ void far_finish_scan(Env<W, S>& e) {
  e.far_rounds(e.nobj);
  // (read BETWEEN the scan's two barriers: behind the second one the rule wave is on its way and may touch a new chunk before a
  // slower wave has looked -- that wave would then believe nothing changed and keep its share of the chunk tables to itself)
  e.far_chunks_staged = e.rec->nchunks_seen;
  e.w.sync();
  e.far_done();
}

// mt_copy: a second LDS home for the MT19937 state as staged (the noise look-ahead twists its own copy: noise_chain)
template <class W, class S, int OM, int CK>
__device__ __forceinline__ void load_env_commit(Env<W, S>& e, const StatePtrs& st, int env, int everything, const EnvStage<W, OM, CK>& q,
                                       uint32_t* mt_copy = nullptr) {
  const Config& c = e.cfg;
  W& w = e.w;
  int cells = c.W * c.H;
  int nch = c.nchunk_x * c.nchunk_y;
  bool lds_maps = e.mat != e.g_mat && !Env<W, S>::kLane;   // small world: maps are LDS-resident, the slot map is derived
  if constexpr (Env<W, S>::kLane)
    if (everything) window_commit(e, e.g_mat, q.win);
  if (everything && lds_maps) clear_slot_map(e);
  stage_commit(w, q.rec, (uint32_t*)e.rec, (const uint32_t*)(st.rec + env), (int)(sizeof(EnvRec) / 4));
  if (e.rules_staged) stage_commit(w, q.rules, (uint32_t*)&e.R, (const uint32_t*)e.tb.rules, CRAFTER_RULES_HEAD_BYTES / 4);
  const int blind = blind_slots<OM>(c.max_objects, W::kThreads);
  const uint4* gob = (const uint4*)(st.objs + (size_t)env * c.max_objects);
  uint4* lob = (uint4*)e.objs;
  if (everything) {
    if (lds_maps) {
      if (cells % 16 == 0)
        stage_commit(w, q.mat, (vec16*)e.mat, (const vec16*)e.g_mat, cells / 16);
      else
        w.block_for(cells, [&](int i) { e.mat[i] = e.g_mat[i]; });
    }
    stage_commit(w, q.mt, (vec16*)e.mt, (const vec16*)(st.mt + (size_t)env * MT_N), MT_N / 4);
    if (mt_copy) stage_commit(w, q.mt, (vec16*)mt_copy, (const vec16*)(st.mt + (size_t)env * MT_N), MT_N / 4);
    stage_commit(w, q.chunk_order, e.chunk_order, (const uint16_t*)(st.chunk_order + (size_t)env * nch), nch);
    stage_commit(w, q.chunk_seen, e.chunk_seen, (const uint8_t*)(st.chunk_seen + (size_t)env * nch), nch);
    if (!e.census_global) stage_commit(w, q.census, e.census, (const int32_t*)(st.census + (size_t)env * nch * 5), nch * 5);
    if constexpr (Env<W, S>::kFar) {
      e.far_clear();
      e.far_publish();
    } else {
      stage_commit(w, q.objs, (vec16*)lob, (const vec16*)gob, blind);
    }
  }
  {   // The step counter AS STAGED, in a word nobody writes while the step runs: wave 0 stores the incremented counter into
      // the record itself, with no barrier before the other waves' first look at it (a thread that arrives late
      // read the new value and guessed the frame's step one too far).  By the thread that holds the record's word.
    // Beside it, in the word's top byte: whether the player is asleep as the step begins (Renderer::stage_rows picks the
    // frame's lit rows by it while the rules run).  Two threads, disjoint bytes.
    constexpr int kStepWord = (int)(offsetof(EnvRec, step) / 4);
    constexpr int kSleepWord = (int)(offsetof(EnvRec, sleeping) / 4);
    const int nt = w.nthreads();
    auto staged = [&](int word) -> uint32_t {
      return (word / nt < EnvStage<W, OM, CK>::M) ? q.rec[word / nt < EnvStage<W, OM, CK>::M ? word / nt : 0] : ((const uint32_t*)(st.rec + env))[word];
    };
    if (w.tid() == kStepWord % nt) w.scratch[3] = 0u;   // (Env::mark_mt_rewritten: nothing has rewritten the stream's state yet)
    if (w.tid() == kStepWord % nt) {
      uint32_t v = staged(kStepWord);   // (< 2^24: crafter_create bounds the daylight table)
      ((uint16_t*)&w.scratch[1])[0] = (uint16_t)v;
      ((uint8_t*)&w.scratch[1])[2] = (uint8_t)(v >> 16);
    }
    if (w.tid() == kSleepWord % nt) ((uint8_t*)&w.scratch[1])[3] = staged(kSleepWord) != 0u ? 1 : 0;
  }
  w.sync();
  e.mt_pos = e.rec->mt_pos;
  e.nobj = e.rec->nobj;
  e.dirty_slots = 0;
  if constexpr (Env<W, S>::kFar) {
    if (everything) far_finish_scan(e);
    return;
  }
  if (everything && e.nobj > blind) {
    // the rest of the slot table (large worlds: ~700 records behind the blind prefix): four records' loads in flight per
    // thread and round -- as a plain copy loop each thread paid one memory round trip per record, three in a row at
    // 8192 x 256x256 (the 11 k clocks of that instance's stage-in: round 5)
    stage_rest((vec16*)lob + blind, (const vec16*)gob + blind, w.tid(), w.nthreads(), e.nobj - blind);
    w.sync();
  }
  if constexpr (Env<W, S>::kLane) {
    if (everything) e.occ_rebuild();   // (a single wave: the commits above are visible to it)
  } else if (everything && lds_maps) {
    derive_slot_map(e, e.nobj);
    w.sync();
  }
}

template <class W, class S>
__device__ __forceinline__ void load_env(Env<W, S>& e, const StatePtrs& st, int env, int everything) {
  EnvStage<W> q;
  load_env_issue(e, st, env, everything, q);
  load_env_commit(e, st, env, everything, q);
}

// LDS -> HBM for the compact tables (maps are written through while the rules run)
// the slot table alone (the step kernel stores it before it draws when the LDS frame overlaps it)
template <class W, class S>
__device__ __forceinline__ void store_objs(Env<W, S>& e, const StatePtrs& st, int env) {
  if constexpr (Env<W, S>::kFar) return;   // (the table in global memory is the one the rules wrote)
  vec16* gob = (vec16*)(st.objs + (size_t)env * e.cfg.max_objects);
  const vec16* lob = (const vec16*)e.objs;
  stage_out<1>(e.w, gob, lob, e.nobj);   // (one record per thread through registers: a 64x64 world has ~30 live objects)
}

// mt_if_rewritten: the stream's state array only goes back if something rewrote it since load_env_commit cleared the mark
// (Env::mark_mt_rewritten); otherwise only its position, in the record, moved
template <class W, class S>
__device__ __forceinline__ void store_env(Env<W, S>& e, const StatePtrs& st, int env, bool with_objs = true, bool mt_if_rewritten = false) {
  const Config& c = e.cfg;
  W& w = e.w;
  int nch = c.nchunk_x * c.nchunk_y;
  if (w.leader()) {
    e.rec->mt_pos = e.mt_pos;
    e.rec->nobj = e.nobj;
  }
  w.sync();
  static_assert(offsetof(EnvRec, mt_pos) == 0, "the record's first word is the stream position");
  uint32_t* grec = (uint32_t*)(st.rec + env);
  const uint32_t* lrec = (const uint32_t*)e.rec;
  constexpr int NT = W::kThreads >= 256 ? 256 : W::kThreads;
  constexpr int KREC = ((int)(sizeof(EnvRec) / 4) + NT - 1) / NT, KMT = (MT_N / 4 + NT - 1) / NT, KCEN = NT >= 256 ? 1 : 3;
  stage_out<KREC>(w, grec, lrec, (int)(sizeof(EnvRec) / 4));
  if (with_objs) store_objs(e, st, env);
  if (!mt_if_rewritten || w.scratch[3] != 0u) stage_out<KMT>(w, (vec16*)(st.mt + (size_t)env * MT_N), (const vec16*)e.mt, MT_N / 4);   // (behind the barrier above)
  bool chunks_changed = true;
  // (behind the barrier above; -1: an adopted world.  A resident stretch stores them whatever its last step did: an earlier one may have touched a chunk)
  if constexpr (Env<W, S>::kFar) chunks_changed = !mt_if_rewritten || e.rec->nchunks_seen != e.far_chunks_staged;
  if (chunks_changed) {
    stage_out<1>(w, st.chunk_order + (size_t)env * nch, (const uint16_t*)e.chunk_order, nch);
    stage_out<1>(w, st.chunk_seen + (size_t)env * nch, (const uint8_t*)e.chunk_seen, nch);
  }
  if (!e.census_global) stage_out<KCEN>(w, st.census + (size_t)env * nch * 5, (const int32_t*)e.census, nch * 5);
}

// wave 0 owns the wave-uniform registers while the rules run; hand them to the other waves
template <class W, class S>
__device__ __forceinline__ void share_registers(Env<W, S>& e) {
  if (e.w.leader()) {
    e.rec->mt_pos = e.mt_pos;
    e.rec->nobj = e.nobj;
    if (e.count_twists) e.w.scratch[2] = (uint32_t)e.rng_twists | ((uint32_t)(e.mat_dirty != 0) << 16);
  }
  e.w.sync();
  e.mt_pos = e.rec->mt_pos;
  e.nobj = e.rec->nobj;
  if (e.count_twists) {
    e.rng_twists = (int)(e.w.scratch[2] & 0xFFFFu);
    e.mat_dirty = (int)(e.w.scratch[2] >> 16);
  }
  e.rng_invalidate();
}

// Night noise, generated AHEAD.  A night frame draws 2 x 63 x 49 = 6174 words of the env's MT19937 stream behind whatever
// the step's rules drew (engine.py:208-209): ten regenerations of the 624-word state, each depending on the one before.
// Drawn inside the frame that is a serial chain in the middle of it -- an epoch's pixels cannot be shaded before its state
// exists, one wave regenerates while the others wait at a barrier per epoch: 28 k clocks per night frame against 2.6 k for
// a day frame's pixels, and the launch lasts as long as its slowest envs.  But the SEQUENCE of states does not
// depend on the rules at all -- they only decide where in it the noise starts -- and while wave 0 runs the rules, the
// workgroup's other waves have nothing to do: wave 1 regenerates a COPY of the staged state kNoiseStates - 1 times and
// leaves every state in the env's scratch in global memory (30 KB, L2 / MALL); the frame then reads its pixels' words
// from there, with no order among pixels, no epochs and no barriers, and the final state goes back into LDS from the
// same scratch.  (kNoiseStates, render.hpp; a step that regenerates twice in its rules falls back to the in-frame pass.)
template <class W>
__device__ __forceinline__ void noise_chain(W& w, uint32_t* state, uint32_t* out) {   // state: LDS copy of the staged state; one wave
  W::set_priority_high();   // the rules do not wait for it, the frame does
  {
    const vec16* src = (const vec16*)state;
    vec16* dst = (vec16*)out;
    w.wave_for(MT_N / 4, [&](int i) { dst[i] = src[i]; });
    w.wsync();
  }
  for (int s_ = 1; s_ < kNoiseStates; s_++) w.mt_twist_tee(state, out + (size_t)s_ * MT_N);   // every new word straight to the scratch as well
  W::set_priority_mid();
}

// Resident steps (rollout_body): the LDS copies of the maps behind a night frame, whose pixel buffer recycled them.  The
// material map comes back from global memory (written through as the rules run), the slot table too if the buffer reached
// into it (it was stored before the frame: frame_over_objs), the slot map is derived again.  Called by every thread behind
// the barrier that opens a resident step; ends on a barrier.
template <class W, class S>
__device__ __forceinline__ void restage_maps(Env<W, S>& e, const StatePtrs& st, int env, bool with_objs) {
  const Config& c = e.cfg;
  W& w = e.w;
  bool lds_maps = e.mat != e.g_mat && !Env<W, S>::kLane;
  int nobj = e.rec->nobj;   // (the record is not part of what a frame recycles; the step before left the count there)
  if (!lds_maps) return;
  const uint4* gob = (const uint4*)(st.objs + (size_t)env * c.max_objects);
  uint4* lob = (uint4*)e.objs;
  copy_map_in(e);
  if (with_objs) w.block_for(nobj, [&](int i) { lob[i] = gob[i]; });
  clear_slot_map(e);
  w.sync();
  derive_slot_map(e, nobj);
  w.sync();
}

template <class W>
__device__ inline RenderTarget obs_target(const Config& c, const TablePtrs& tb, uint8_t* obs, int env) {
  RenderTarget rt;
  rt.out = obs ? obs + (size_t)env * c.size_w * c.size_h * 3 : nullptr;
  rt.size_w = c.size_w;
  rt.size_h = c.size_h;
  rt.unit_x = c.unit_x;
  rt.unit_y = c.unit_y;
  rt.border_x = c.border_x;
  rt.border_y = c.border_y;
  rt.icon_w = c.icon_w;
  rt.icon_h = c.icon_h;
  rt.digit_w = c.digit_w;
  rt.digit_h = c.digit_h;
  rt.item_pos = tb.item_pos;
  rt.tex_tile = tb.tex_tile;
  rt.tex_icon = tb.tex_icon;
  rt.tex_digit = tb.tex_digit;
  rt.atlas = tb.atlas;
  rt.vignette = tb.vignette;
  return rt;
}

// info['semantic'] (engine.py:251-264): material ids with object cells replaced by class ids
template <class W, class S>
__device__ __forceinline__ void write_semantic(Env<W, S>& e, uint8_t* semantic, int env) {
  const Config& c = e.cfg;
  int cells = c.W * c.H;
  uint8_t* out = semantic + (size_t)env * cells;
  int base = e.R.n_materials;  // len(mat_ids) = n_materials + 1 (None), first class id = that + 0
  if constexpr (Env<W, S>::kLane) {   // no slot map: the materials first, then the objects' cells over them
    e.w.block_for(cells, [&](int i) {
      int x = i / c.H, y = i - x * c.H;
      out[i] = (uint8_t)e.mat_at(x, y);
    });
    W::drain_stores();   // the second pass rewrites bytes other lanes have just stored
    e.w.block_for(e.nobj, [&](int i) {
      Obj o = e.objs[i];
      if (i >= 1 && o.type != T_NONE) out[e.cidx(o.x, o.y)] = (uint8_t)(base + o.type);
    });
    return;
  }
  e.w.block_for(cells, [&](int i) {
    int v = e.mat[i];
    int slot = e.objmap[i];
    if (slot) v = base + e.objs[slot].type;
    out[i] = (uint8_t)v;
  });
}

}  // namespace crafter
