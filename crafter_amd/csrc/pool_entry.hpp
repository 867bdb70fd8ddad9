// The device side of the world-pool protocol: requests, readiness, adoption of a pooled world.
#pragma once
#include "env_stage.hpp"

namespace crafter {

// World pool.  A world depends only on (seed, episode) (env.py:74), so the NEXT episode's world of
// every env is generated ahead of time by gen_body on a side stream and adopted by the step kernel
// the moment the env finishes; Env.reset's worldgen then never sits on the step's critical path.
// Whether an env adopts a pooled world or falls back to reset_body is unobservable: both run the
// same stages of the one generator (worldgen.hpp "the generator's stages") on the same (seed, episode);
// tests/test_generator_forms_host.py and tests/test_gpu_generator_forms.py compare their worlds field by field.

// The pool runs TWO worlds ahead of every env (its two entries, by episode parity): when the env enters episode k it
// asks for every world up to k + 2 that has not been asked for yet -- in steady state exactly one, world k + 2, which is
// then due a whole episode later.  One world ahead was not enough: an episode shorter than the generation latency
// (a few dozen steps) found its successor unfinished and paid an inline regeneration on the launch stream.
// gen_latest[env] = newest episode requested so far; a request is still wanted while it is one of the newest two.
// (gen_latest, PoolHdr.pending and PoolHdr.ready cross concurrently running kernels: W::agent_load / agent_store -- VERDICT r3 1c)
template <class W>
__device__ inline bool gen_wanted(const StatePtrs& st, int env, int episode) { return episode >= W::agent_load(st.gen_latest + env) - 1; }

// one segment of the request ring: count (+3 pad), then up to gen_q_capacity (env, episode) pairs
__host__ __device__ inline int gen_q_capacity(const Config& c) { return 2 * c.num_envs; }
__host__ __device__ inline size_t gen_q_stride(const Config& c) { return (size_t)4 * c.num_envs + 4; }

// pool entry of (env, episode): two entries per env, by episode parity
__device__ inline size_t pool_slot(const Config& c, int env, int episode) {
  return (size_t)(episode & 1) * c.num_envs + env;
}

template <class W>
__device__ __forceinline__ void request_generation(W& w, const Config& cfg, const StatePtrs& st, int gen_parity, int env,
                                          int upto) {
  if (gen_parity < 0 || !st.gen_q || !w.leader()) return;
  int32_t* q = st.gen_q + (size_t)gen_parity * gen_q_stride(cfg);
  int have = W::agent_load(st.gen_latest + env);
  for (int episode = (have + 1 > upto - 1) ? have + 1 : upto - 1; episode <= upto; episode++) {
    // One writer per pool entry at a time: worlds of equal episode parity share an entry.  Normally the older
    // one has long been adopted when the newer one is asked for; after an inline regeneration (the older world was not
    // ready in time) it may still sit in a batch in flight -- then the request is put off (not recorded as requested: the
    // env's next reset asks again), instead of letting two batches write one entry side by side.
    PoolHdr* hdr = st.pool_hdr + pool_slot(cfg, env, episode);
    if (W::agent_load(&hdr->pending) != 0) break;
    int k = w.global_add(q, 1);
    if (k >= gen_q_capacity(cfg)) break;   // full segment (an env would have to reset several times within one batch
                                           // period): not recorded as requested, asked for again at the next reset
    q[4 + 2 * k] = env;
    q[4 + 2 * k + 1] = episode;
    W::agent_store(&hdr->pending, (int32_t)episode);
    W::agent_store(st.gen_latest + env, (int32_t)episode);
  }
}

// the entry already holds this very world, finished (Env.reset generated it itself, crafter_reset_kernel): a queued
// duplicate must not write it again in place -- the entry may be adopted any moment
template <class W>
__device__ inline bool gen_done_already(const Config& c, const StatePtrs& st, int env, int episode) {
  uint64_t r = W::agent_load(&st.pool_hdr[pool_slot(c, env, episode)].ready);
  return (uint32_t)r == (uint32_t)episode && (r >> 32) != 0;
}
// a request is through its batch (generated, superseded or a duplicate): the entry may take the next one
template <class W>
__device__ inline void gen_retire(const Config& c, const StatePtrs& st, int env, int episode) {
  PoolHdr* h = st.pool_hdr + pool_slot(c, env, episode);
  if (W::agent_load(&h->pending) == episode) W::agent_store(&h->pending, (int32_t)0);
}

// true if the pool holds exactly the world `episode` of this env AND its generation batch is known
// complete on the launch stream (ready is one 8-byte word: batch sequence << 32 | episode)

template <class W>
__device__ inline bool pool_ready(const Config& c, const StatePtrs& st, int env, int episode, uint32_t safe_seq) {
  if (!st.pool_hdr) return false;
  uint64_t r = W::agent_load(&st.pool_hdr[pool_slot(c, env, episode)].ready);
  uint32_t seq = (uint32_t)(r >> 32), ep = (uint32_t)r;
  return ep == (uint32_t)episode && seq != 0 && seq <= safe_seq;
}

// Env.reset with a pre-generated world: copies the pool entry into the live state (LDS + HBM).
template <class W, class S>
__device__ __forceinline__ void adopt_world(Env<W, S>& e, const StatePtrs& st, int env, int episode) {
  const Config& c = e.cfg;
  W& w = e.w;
  int cells = c.W * c.H;
  int nch = c.nchunk_x * c.nchunk_y;
  size_t slot = pool_slot(c, env, episode);
  const PoolHdr hdr = st.pool_hdr[slot];
  const uint8_t* pm = st.pool_mat + slot * cells;
  w.sync();
  bool lds_maps = e.mat != e.g_mat && !Env<W, S>::kLane;
  if constexpr (Env<W, S>::kLane) {   // the map goes HBM -> HBM; the window is cut out of the pool entry (read-only)
    const uint4* src = (const uint4*)pm;
    uint4* gm = (uint4*)e.g_mat;
    w.block_for(cells / 16, [&](int i) { gm[i] = src[i]; });
  } else if (cells % 16 == 0) {
    const uint4* src = (const uint4*)pm;
    uint4* lm = (uint4*)e.mat;
    uint4* gm = (uint4*)e.g_mat;
    w.block_for(cells / 16, [&](int i) {
      uint4 v = src[i];
      if (lds_maps) lm[i] = v;
      gm[i] = v;
    });
    uint4 z;
    z.x = z.y = z.z = z.w = 0;
    uint4* lo = (uint4*)e.objmap;
    uint4* go = (uint4*)e.g_objmap;
    if (lds_maps) w.block_for(cells * (int)sizeof(S) / 16, [&](int i) { lo[i] = z; });
    else w.block_for(cells / 8, [&](int i) { go[i] = z; });
  } else {
    if constexpr (!Env<W, S>::kLane)
      w.block_for(cells, [&](int i) {
        uint8_t v = pm[i];
        e.mat[i] = v;
        e.g_mat[i] = v;
        e.objmap[i] = 0;
        if (!lds_maps) e.g_objmap[i] = 0;
      });
  }
  const uint4* pmt = (const uint4*)(st.pool_mt + slot * MT_N);
  uint4* lmt = (uint4*)e.mt;
  w.block_for(MT_N / 4, [&](int i) { lmt[i] = pmt[i]; });
  const uint16_t* pco = st.pool_chunk_order + slot * nch;
  w.block_for(nch, [&](int i) {
    e.chunk_order[i] = pco[i];
    e.chunk_seen[i] = 0;
  });
  w.sync();
  const uint4* po = (const uint4*)(st.pool_objs + slot * c.max_objects);
  uint4* lob = (uint4*)e.objs;
  w.block_for(hdr.nobj, [&](int i) {
    uint4 rec16 = po[i];
    lob[i] = rec16;
    if constexpr (!Env<W, S>::kLane) {
      if (i >= 1) {
        Obj o;   // from the value just copied: reading e.objs[i] back through another type would race the uint4 store
        __builtin_memcpy(&o, &rec16, sizeof(Obj));
        int ci = e.cidx(o.x, o.y);
        e.objmap[ci] = (S)i;
        if (!lds_maps) e.g_objmap[ci] = (uint16_t)i;
      }
    }
  });
  w.block_for(hdr.nchunks_seen, [&](int i) { e.chunk_seen[e.chunk_order[i]] = 1; });
  if constexpr (Env<W, S>::kLane) {
    w.sync();
    Obj p = e.objs[1];   // the new world's player (worldgen puts it at the centre of the map)
    place_window(e, p.x, p.y);
    uint64_t win[(kWinX * kWinY / 8 + W::kThreads - 1) / W::kThreads];
    window_issue(e, pm, win);
    window_commit(e, pm, win);
  }
  // the grass / path counts per chunk came with the world (the generator counted them)
  const int32_t* pcs = st.pool_census + slot * nch * 5;
  w.block_for(nch * 5, [&](int i) { e.census[i] = pcs[i]; });
  e.begin_episode(episode);
  if (w.leader()) {
    e.rec->nchunks_seen = hdr.nchunks_seen;
    e.rec->status |= (uint32_t)hdr.pad;   // e.g. object-table overflow while generating
    if ((uint32_t)hdr.ready != (uint32_t)episode) e.rec->status |= ST_POOL_MISMATCH;   // scheduler invariant broken
  }
  e.mt_pos = hdr.mt_pos;
  e.mark_mt_rewritten();
  e.nobj = hdr.nobj;
  e.dirty_slots = 0;
  if constexpr (Env<W, S>::kFar) {   // the cache held the old world's records: only the new player's entry stands (the frame reads the rest from the table)
    w.block_for(64, [&](int i) { ((uint32_t*)e.ndm)[i] = 0u; });
    if (w.leader()) {
      uint4 p1 = po[1];
      p1.w = 1u;
      *(uint4*)&e.ncache[0] = p1;
      e.ndm[1] = 1;
    }
    e.far_live = hdr.nobj - 1;
    e.far_chunks_staged = -1;
    e.cur_slot = -1;
    e.cur_idx = -1;
    W::drain_stores();   // (the table's new records are read straight from the coherence point: Env::obj_rd_lane)
  }
  w.sync();
  e.occ_rebuild();
}

}  // namespace crafter
