// Authored worlds (crafter_reset_worlds): Env.reset (env.py:70-81) with worldgen.generate_world replaced by "write this map,
// add these objects" -- a second world source for the reset path.  What makes a row steppable is more than the map and the
// object list: the slot table in insertion order, the cell -> slot map, the chunk keys in first-touch order, the per-chunk
// census, nobj and the stream position are derived tables the reference builds by calling World.add / World.move in a
// particular order.  So the caller's records are not copied into the row: they are REPLAYED through Env::obj_add / obj_move
// (env_core.hpp), the same calls worldgen makes, in record order, and everything derived comes out as the reference's.
//
//   author_world   : World.reset and RandomState(world seed) -- the generator's own stages, WorldGen::world_reset and
//                    seed_stream (worldgen.hpp) -- the player at the centre, then the authored function: the map, the
//                    records, the inventory
//   reset_world_body : reset_body (reset_bodies.hpp: the same reset_skeleton) with author_world where reset_env stands
//
// The bank comes from a caller and is never trusted: a value that would index outside a table is repaired or its record is
// skipped, and the env's sticky ST_BAD_WORLD says so (include/crafter_hip.h lists the cases).  The authored function draws
// nothing: the episode's stream starts at the first word of RandomState(world seed).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/crafter_hip.h"
#include "env_kernels.hpp"

namespace crafter {

constexpr uint32_t ST_BAD_WORLD = CRAFTER_ST_BAD_WORLD;   // (the header keeps it beside crafter_reset_worlds)

// crafter_reset_worlds' bank arguments as the kernel gets them (all device pointers; include/crafter_hip.h)
struct WorldBank {
  const int32_t* world_id;   // [num_envs] or null: env % n_worlds
  const uint8_t* mat;        // [n_worlds][W * H]
  const Obj* objs;           // [n_worlds][max_objects]
  const int32_t* nobj;       // [n_worlds]
  const int32_t* inv;        // [n_worlds][rules.n_items] or null: the rules' initial inventory
  int32_t n_worlds;          // >= 1
  int32_t max_objects;       // >= 0: the bank's record capacity per world (not the batch's slot table)
};

// a facing the rules can walk along (objects.py:72,355: one of the four unit axis vectors)
__host__ __device__ inline bool unit_axis(int fx, int fy) { return fx * fx + fy * fy == 1; }

// The world function of an authored reset, behind World.reset / the seeded stream / the player at the centre.  Every wave
// calls; ends on a barrier with the wave-uniform registers (nobj, mt_pos) in wave 0, as reset_env leaves them.
template <class W, class S>
__device__ __forceinline__ void author_world(WorldGen<W, S>& wg, const LevelTable* levels, const WorldBank& bank, int world) {
  Env<W, S>& e = wg.e;
  W& w = e.w;
  const Config& c = e.cfg;
  const Rules& R = e.R;
  EnvRec* rec = e.rec;
  const int cells = c.W * c.H;
  const int episode = rec->episode + 1;
  const uint32_t wseed = level_seed(levels, rec->seed_lane, episode);   // env.py:74, as reset_env seeds it
  w.sync();
  e.begin_episode(episode);
  // player.inventory = inv_j (behind Player.__init__: both _last_health fields keep the initial inventory's health, env.py:77, objects.py:78)
  if (bank.inv) {
    const int32_t* inv = bank.inv + (size_t)world * R.n_items;
    w.block_for(R.n_items, [&](int i) {
      int v = inv[i];
      rec->inv[i] = v < 0 ? 0 : v > R.item_max[i] ? R.item_max[i] : v;
    });
  }
  wg.world_reset();
  // the material map: bank -> registers -> the LDS copy and the env's map in global memory, 16 bytes per load where both
  // rows are aligned, byte by byte for what is left.  A byte that names no material becomes grass on the way.
  {
    const uint8_t* src = bank.mat + (size_t)world * cells;
    const uint32_t nmat = (uint32_t)R.n_materials, grass = (uint32_t)R.mat_grass;
    bool bad = false;
    auto clean = [&](uint32_t m) -> uint32_t {
      if (m - 1u < nmat) return m;
      bad = true;
      return grass;
    };
    const bool aligned = (((uintptr_t)src | (uintptr_t)e.g_mat | (uintptr_t)e.mat) & 15u) == 0;
    const int nvec = aligned ? cells / 16 : 0;
    w.block_for(nvec, [&](int i) {
      vec16 v = ((const vec16*)src)[i];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        uint32_t q = v[k];
        v[k] = clean(q & 0xFFu) | (clean((q >> 8) & 0xFFu) << 8) | (clean((q >> 16) & 0xFFu) << 16) | (clean(q >> 24) << 24);
      }
      ((vec16*)e.mat)[i] = v;
      if (e.g_mat != e.mat) ((vec16*)e.g_mat)[i] = v;
    });
    w.block_for(cells - 16 * nvec, [&](int k) {
      int i = 16 * nvec + k;
      uint8_t m = (uint8_t)clean(src[i]);
      e.mat[i] = m;
      if (e.g_mat != e.mat) e.g_mat[i] = m;
    });
    if (bad) w.lds_or(&rec->status, ST_BAD_WORLD);
  }
  wg.seed_stream(wseed);
  w.sync();
  if (w.wave0()) {
    const int px = c.W / 2, py = c.H / 2;
    e.obj_add(T_PLAYER, px, py, 0, 0, 1, 0);   // facing (0, 1) objects.py:72; slot 1, its chunk the first key
    // The records, one after the other (slot numbers and chunk keys are order sensitive): 64 at a time come into lane
    // registers with one load per lane, each is then read out of its lane (no memory round trip per record).
    int n = bank.nobj[world];
    n = n < 0 ? 0 : n > bank.max_objects ? bank.max_objects : n;
    const Obj* recs = bank.objs + (size_t)world * bank.max_objects;
    uint32_t flags = 0;
    for (int base = 0; base < n; base += 64) {
      w.template lane_set4<4>(base, n, [&](int i, int) -> vec16 { return *(const vec16*)&recs[i]; });
      const int m = n - base < 64 ? n - base : 64;
      for (int l = 0; l < m; l++) {
        const uint32_t w0 = w.lane_read(4, l), w1 = w.lane_read(5, l);
        const int aux = (int)w.lane_read(6, l);
        const int type = (int)(w0 & 0xFFu), health = (int)(int8_t)(w0 >> 8);
        int fx = (int)(int8_t)(w0 >> 16), fy = (int)(int8_t)(w0 >> 24);
        const int x = (int)(w1 & 0xFFFFu), y = (int)(w1 >> 16);
        const bool faces = type == T_PLAYER || type == T_ARROW;   // the other classes keep no facing: (0, 0), as World.add's callers write it
        if (type < T_PLAYER || type > T_PLANT || !e.inside(x, y) || (type == T_PLAYER && base + l != 0)) {
          flags |= ST_BAD_WORLD;
          continue;
        }
        if (!faces) {
          fx = fy = 0;
        } else if (!unit_axis(fx, fy)) {
          flags |= ST_BAD_WORLD;
          fx = 0;
          fy = 1;
        }
        if (type == T_PLAYER) {   // record 0: where the player stands and looks (nothing else is in the world yet)
          if (x != px || y != py) e.obj_move(1, px, py, x, y, true);
          if (w.leader()) {
            e.objs[1].fx = (int8_t)fx;
            e.objs[1].fy = (int8_t)fy;
          }
          w.wsync();
          continue;
        }
        if (W::uni(e.slot_at(x, y)) != 0) {
          flags |= ST_BAD_WORLD;
          continue;
        }
        e.obj_add(type, x, y, health, fx, fy, aux);
      }
    }
    if (flags) {
      e.st(&rec->status, rec->status | flags);
      w.wsync();
    }
  }
  w.sync();
}

// crafter_reset_worlds for one env: reset_body with the authored function where the generator stands.  Returns the episode the
// env is now in, or -1 when its world id names no world of the bank: the row is then left as it is, but for ST_BAD_WORLD.
template <class W>
__device__ __forceinline__ int reset_world_body(W& w, uint8_t* smem, int env, const Config& cfg, const TablePtrs& tb, const StatePtrs& st,
                                                const WorldBank& bank, uint8_t* obs, const LevelTable* levels = nullptr) {
  typedef uint16_t S;
  const int world = W::uni(bank.world_id ? bank.world_id[env] : env % bank.n_worlds);
  if (world < 0 || world >= bank.n_worlds) {
    if (w.leader()) st.rec[env].status |= ST_BAD_WORLD;
    return -1;
  }
  return reset_skeleton<W, S>(w, smem, env, cfg, tb, st, obs, nullptr, [&](Env<W, S>& e, const LdsLayout& L) {
    WorldGen<W, S> wg(e, smem + L.wg);
    author_world(wg, levels, bank, world);
    e.recount_space();
    share_registers(e);
  });
}

}  // namespace crafter
