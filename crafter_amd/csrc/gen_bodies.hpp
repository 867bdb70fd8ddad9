// World generation into the pool: the fused gen_body and the three-kernel pipeline (seed, classify, resolve).
#pragma once
#include "pool_entry.hpp"

namespace crafter {

// What gen_body and gen_resolve_body share, each in its own order:
// the rules' head (load_env does this for the other kernels)
template <class W, class S>
__device__ __forceinline__ void copy_rules_head(Env<W, S>& e) {
  const uint32_t* src = (const uint32_t*)e.tb.rules;
  uint32_t* dst = (uint32_t*)&e.R;
  e.w.block_for(CRAFTER_RULES_HEAD_BYTES / 4, [&](int i) { dst[i] = src[i]; });
}
// the generated world's compact tables into its pool entry: slot table (unless it was written there in place), MT state, chunk
// order.  (The census goes out at a different point in either body and stays spelled out there: behind a helper of its own
// crafter_gen_resolve_kernel compiles to other code.)
template <class W, class S>
__device__ __forceinline__ void store_pool_tables(Env<W, S>& e, const StatePtrs& st, size_t slot, int nch) {
  W& w = e.w;
  uint4* gob = (uint4*)(st.pool_objs + slot * e.cfg.max_objects);
  const uint4* lob = (const uint4*)e.objs;
  if (lob != gob) w.block_for(e.nobj, [&](int i) { gob[i] = lob[i]; });
  uint32_t* gmt = st.pool_mt + slot * MT_N;
  w.block_for(MT_N, [&](int i) { gmt[i] = e.mt[i]; });
  uint16_t* gco = st.pool_chunk_order + slot * nch;
  w.block_for(nch, [&](int i) { gco[i] = e.chunk_order[i]; });
}
// the entry's header, by one thread behind the barrier that follows those stores; `ready` last: it publishes the entry
template <class W, class S>
__device__ __forceinline__ void publish_pool_entry(Env<W, S>& e, PoolHdr* h, uint32_t seq, int episode) {
  h->mt_pos = e.mt_pos;
  h->nobj = e.nobj;
  h->nchunks_seen = e.rec->nchunks_seen;
  h->pad = (int32_t)e.rec->status;
  W::agent_store(&h->ready, ((uint64_t)seq << 32) | (uint32_t)episode);
}

// Generates the world of (env, episode) into the pool.  Touches no live state of the env (which the
// launch stream may be stepping concurrently): reads only the immutable seed lane.
template <class W>
__device__ __forceinline__ void gen_body(W& w, uint8_t* smem, int env, int episode, uint32_t seq, const Config& cfg,
                                const TablePtrs& tb, const StatePtrs& st, const LevelTable* levels = nullptr) {
  LdsLayout L = big_reset_layout(cfg);
  w.scratch = (uint32_t*)(smem + L.scratch);
  if (!gen_wanted<W>(st, env, episode)) return;   // superseded by newer requests of the same env
  Env<W> e(w, cfg, tb, smem + L.rules);
  bind_lds(e, smem, L, st, env);
  if (L.objs < 0) e.objs = st.pool_objs + pool_slot(cfg, env, episode) * cfg.max_objects;   // the pool entry's table, in place
  int cells = cfg.W * cfg.H;
  int nch = cfg.nchunk_x * cfg.nchunk_y;
  bool lds_maps = e.mat != e.g_mat;
  size_t slot = pool_slot(cfg, env, episode);
  e.g_mat = st.pool_mat + slot * cells;   // the generator's write-through target is the pool
  e.g_objmap = nullptr;
  if (!lds_maps) {   // large world: generate straight into the pool entry; no slot map is needed
    e.mat = e.g_mat;
    e.objmap = nullptr;
  }
  w.sync();
  copy_rules_head(e);
  if (w.leader()) {
    e.rec->seed_lane = st.rec[env].seed_lane;
    e.rec->episode = episode - 1;
    e.rec->status = 0;
  }
  w.sync();
  WorldGen<W> wg(e, smem + L.wg);
  wg.levels = levels;
  wg.reset_env(nullptr);
  share_registers(e);
  store_pool_tables(e, st, slot, nch);
  w.sync();
  e.recount_space();
  int32_t* gcs = st.pool_census + slot * nch * 5;
  w.block_for(nch * 5, [&](int i) { gcs[i] = e.census[i]; });
  w.sync();
  if (w.leader()) publish_pool_entry(e, st.pool_hdr + slot, seq, episode);
}

// ---------------------------------------------------------------------------------------------
// World-pool generation as a pipeline of three kernels: the stages of WorldGen (worldgen.hpp "the generator's stages") that
// reset_env -- and with it gen_body, the fused form crafter_reset_kernel appends -- runs back to back, here with the pool entry
// in between: seed_world | classify_head / classify_lookup / classify_advance | world_reset, draw_world, strip_flags.
// Generating a world is 5 % seeding (serial: init_genrand, the OpenSimplex
// shuffle), 50 % terrain noise (parallel over cells, 128 VGPRs of f64) and 45 % ordered uniform() draws (serial, one
// wave).  In one 1024-thread workgroup the serial half holds a whole CU's registers while 15 waves sleep at a barrier;
// split by kind of parallelism, every piece is sized for what it does and fits NEXT TO the step kernel's workgroups:
//   gen_seed_body      1 wave  / world,  3.6 KB LDS
//   gen_classify_body  4 waves / world, 0.5 KB LDS, no barrier after the table load
//   gen_resolve_body   1 wave  / world, gen_resolve_lds_bytes (14 KB for 64x64)
// Hand-offs go through the pool entry itself: pool_mt (state after the seed draw), pool_perm, pool_mat (cell codes,
// then final materials), PoolHdr.mt_pos.  `ready` is stamped by the last stage only.

// Probe builds (-DCRAFTER_PROBES): shader clocks per phase of the generation kernels, summed over all worlds
// (crafter_debug_gen_probe reads and clears them).  [0..7] seeding, [8..15] classification, [16..31] ordered draws; the last slot
// of each group counts the worlds.
#if defined(CRAFTER_PROBES)
static __device__ unsigned long long g_gen_probe[32];
#define GEN_T0 uint64_t gen_t0_ = w.clock();
#define GEN_STAMP(k) do { if (w.leader()) { uint64_t t_ = w.clock(); atomicAdd(&g_gen_probe[k], (unsigned long long)(t_ - gen_t0_)); gen_t0_ = t_; } } while (0)
#define GEN_COUNT(k) do { if (w.leader()) atomicAdd(&g_gen_probe[k], 1ull); } while (0)
#else
#define GEN_T0
#define GEN_STAMP(k) do { } while (0)
#define GEN_COUNT(k) do { } while (0)
#endif

template <class W>
__device__ __forceinline__ void gen_seed_body(W& w, uint8_t* smem, int env, int episode, const Config& cfg, const TablePtrs& tb,
                                     const StatePtrs& st, const LevelTable* levels = nullptr) {
  if (!gen_wanted<W>(st, env, episode) || gen_done_already<W>(cfg, st, env, episode)) return;   // superseded by a newer request of the same env / a duplicate
  Env<W> e(w, cfg, tb);
  e.mt = (uint32_t*)smem;
  e.objmap = nullptr;
  e.g_objmap = nullptr;
  w.scratch = (uint32_t*)(smem + kGenSeedLds - 16);
  WorldGen<W> wg(e, smem + align16(4 * MT_N));
  uint32_t wseed = level_seed(levels, st.rec[env].seed_lane, episode);   // env.py:74
  GEN_T0
  wg.seed_world(wseed, false, [&](int k) { GEN_STAMP(k); });   // slots 0 .. 2; the tables are gen_classify_body's to fill: this LDS ends in front of them
  GEN_COUNT(7);
  e.mt_pos = (int)w.bcast_from_wave0((uint32_t)e.mt_pos);   // wave 0's stream position -> every wave (single-wave workgroups: a no-op)
  size_t slot = pool_slot(cfg, env, episode);
  uint32_t* gmt = st.pool_mt + slot * MT_N;
  w.block_for(MT_N, [&](int i) { gmt[i] = e.mt[i]; });
  uint32_t* gp = (uint32_t*)(st.pool_perm + slot * 512);
  const uint32_t* lp = (const uint32_t*)wg.perm;   // perm[256] and pg3[256] are adjacent
  w.block_for(128, [&](int i) { gp[i] = lp[i]; });
  if (w.leader()) st.pool_hdr[slot].mt_pos = e.mt_pos;
}

template <class W>
__device__ __forceinline__ void gen_classify_body(W& w, uint8_t* smem, int env, int episode, int part, int parts, const Config& cfg,
                                         const TablePtrs& tb, const StatePtrs& st) {
  if (!gen_wanted<W>(st, env, episode) || gen_done_already<W>(cfg, st, env, episode)) return;
  size_t slot = pool_slot(cfg, env, episode);
  GEN_T0
  Env<W> e(w, cfg, tb);
  WorldGen<W> wg(e, smem);
  const uint32_t* gp = (const uint32_t*)(st.pool_perm + slot * 512);
  uint32_t* lp = (uint32_t*)smem;
  w.block_for(128, [&](int i) { lp[i] = gp[i]; });
  wg.tab = (SimplexLds*)(smem + 512);   // this kernel keeps no MT state: the tables sit right behind the permutation
  wg.fill_gradients();
  w.sync();
  Simplex<W> sx{wg.perm, wg.pg3, wg.tab};
  const typename WorldGen<W>::ClassIds ids = wg.class_ids();
  int cells = cfg.W * cfg.H;
  int px = cfg.W / 2, py = cfg.H / 2;
  uint8_t* codes = st.pool_mat + slot * cells;
  int first = part * kGenClassifyCells;
  int per = cells - first < kGenClassifyCells ? cells - first : kGenClassifyCells;
  (void)parts;
  // LDS behind the tables (perm, gradient numbers, gradients): per-cell state bytes, the round's work list, its counter
  uint8_t* state = smem + kGenClassifyTables;
  uint16_t* items = (uint16_t*)(smem + kGenClassifyTables + kGenClassifyCells);
  uint32_t* count = (uint32_t*)(smem + kGenClassifyTables + 3 * kGenClassifyCells);
  w.block_for(per, [&](int k) {
    int i = first + k;
    int x = i / cfg.H, y = i - x * cfg.H;
    int stt;
    uint8_t code = WorldGen<W>::classify_head(sx, ids, x, y, px, py, stt);
    state[k] = (uint8_t)stt;
    if ((stt & 15) == WorldGen<W>::NK_DONE) codes[i] = code;
  });
  GEN_STAMP(8);
  for (;;) {
    if (w.leader()) *count = 0;
    w.sync();
    for (int base = 64 * w.wave_index(); base < per; base += 64 * W::num_waves()) {   // dense list of the cells that need a look-up
      uint64_t m = w.ballot(base, per, [&](int k) { return (state[k] & 15) != WorldGen<W>::NK_DONE; });
      if (!m) continue;
      uint32_t at = 0;
      if (w.lane() == 0) at = w.lds_fetch_add(count, (uint32_t)__builtin_popcountll(m));
      at = (uint32_t)W::uni((int)at);
      w.lanes(base, per, [&](int k, int lane) {
        if ((m >> lane) & 1ull) items[at + __builtin_popcountll(m & ((1ull << lane) - 1ull))] = (uint16_t)k;
      });
    }
    w.sync();
    int n = (int)*count;
    if (n == 0) break;
    GEN_COUNT(14);
    w.block_for(n, [&](int j) {
      int k = items[j];
      int i = first + k;
      int x = i / cfg.H, y = i - x * cfg.H;
      int stt = state[k];
      double v = WorldGen<W>::classify_lookup(sx, stt, x, y);
      uint8_t code = 0;
      int nxt = WorldGen<W>::classify_advance(ids, stt, v, code);
      state[k] = (uint8_t)nxt;
      if ((nxt & 15) == WorldGen<W>::NK_DONE) codes[i] = code;
    });
    w.sync();
  }
  GEN_STAMP(9);
  GEN_COUNT(15);
}

template <class W>
__device__ __forceinline__ void gen_resolve_body(W& w, uint8_t* smem, int env, int episode, uint32_t seq, const Config& cfg,
                                        const TablePtrs& tb, const StatePtrs& st) {
  if (!gen_wanted<W>(st, env, episode) || gen_done_already<W>(cfg, st, env, episode)) {
    if (w.leader()) gen_retire<W>(cfg, st, env, episode);
    return;
  }
  GenResolveLayout G = gen_resolve_layout(cfg);
  w.scratch = (uint32_t*)(smem + G.scratch);
  GEN_T0
  int cells = cfg.W * cfg.H;
  int nch = cfg.nchunk_x * cfg.nchunk_y;
  size_t slot = pool_slot(cfg, env, episode);
  Env<W> e(w, cfg, tb, smem + G.rules);
  e.g_mat = st.pool_mat + slot * cells;
  e.g_objmap = nullptr;
  e.objmap = nullptr;                                   // worldgen places every creature on its own cell: no slot map
  e.mat = G.mat >= 0 ? smem + G.mat : e.g_mat;          // large world: resolve in place in the pool entry
  e.objs = G.objs >= 0 ? (Obj*)(smem + G.objs) : st.pool_objs + slot * cfg.max_objects;
  e.mt = (uint32_t*)(smem + G.mt);
  e.rec = (EnvRec*)(smem + G.rec);
  e.chunk_order = (uint16_t*)(smem + G.chunk_order);
  e.chunk_seen = smem + G.chunk_seen;
  e.census = (int32_t*)(smem + G.census);
  copy_rules_head(e);
  if (e.mat != e.g_mat) copy_map_in(e);
  const uint32_t* gmt = st.pool_mt + slot * MT_N;
  w.block_for(MT_N, [&](int i) { e.mt[i] = gmt[i]; });
  WorldGen<W> wg(e, smem + G.wg);
  wg.world_reset();
  e.st(&e.rec->status, 0);
  e.mt_pos = st.pool_hdr[slot].mt_pos;   // the stream as gen_seed_body left it: one draw in
  e.rng_invalidate();
  w.sync();
  GEN_STAMP(16);
  wg.draw_world(cells, [&](int k) { GEN_STAMP(17 + k); });   // slots 17 .. 19
  share_registers(e);
  wg.strip_flags(cells);
  GEN_STAMP(20);
  e.recount_space();   // the world's grass / path counts per chunk travel with it (adopt_world copies them)
  GEN_STAMP(21);
  int32_t* gcs = st.pool_census + slot * nch * 5;
  w.block_for(nch * 5, [&](int i) { gcs[i] = e.census[i]; });
  store_pool_tables(e, st, slot, nch);
  w.sync();
  if (w.leader()) {
    publish_pool_entry(e, st.pool_hdr + slot, seq, episode);
    gen_retire<W>(cfg, st, env, episode);
  }
  GEN_STAMP(22);
  GEN_COUNT(31);
}

}  // namespace crafter
