// Symbolic egocentric observation (crafter_symbolic): the player's local window as class ids and sprite variants, plus the
// inventory and vitals -- what the frame of the same state depicts, as numbers.  Every value is the reference's:
//   which cells        engine.py:155-187  LocalView.__call__: local (x, y) = world player.pos + (x, y) - grid // 2, cells
//                                         outside the world are not drawn (id 0 = None here)
//   plane 0, class ids engine.py:251-264  SemanticView: the material id, n_materials + type where an object stands
//   plane 1, variants  objects.py:85-93, 361-367, 395-403: the texture an object shows (render.hpp sprite_texture) --
//                      player 1 left, 2 right, 3 up, 4 down, 5 sleeping; arrow 1 .. 4 likewise; plant 1 if ripe; else 0
//   stats              env.py:108-115 the inventory in item order, then facing x, facing y, sleeping, and env.py:135-139 the
//                      daylight of the env's step (the table's double rounded to float)
// Read-only: no RNG draw (Env.render() takes a night frame's noise again), no byte of state changes.
//
// One wave per env.  The window (2 * gw * gh bytes: plane 0 then plane 1, cell x * gh + y) is assembled in the wave's own
// LDS strip and leaves as whole dwords; nothing here needs a workgroup barrier, so a masked row or the batch tail returns
// at once.  Two ways to the objects, chosen as the step kernels choose where the cell -> slot map lives:
//   MAP 0  (worlds staged in LDS: StatePtrs.objmap is never written) the lanes stride over slots 1 .. nobj - 1, one
//          16-byte record each, and keep the live ones that stand inside the window.  A cell holds at most one object
//          (engine.py:50-57, 67-80), so two lanes never write the same byte.
//   MAP 1  (maps in global memory, up to 65,535 slots) objmap is state: each window cell reads its slot id and only the
//          records named are loaded.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "types.hpp"

namespace crafter {

constexpr int kSymbolicThreads = 256;                       // four envs per workgroup
constexpr int kSymbolicEnvs = kSymbolicThreads / 64;
constexpr int kSymbolicStatsExtra = 4;                      // facing x, facing y, sleeping, daylight

__host__ __device__ inline int symbolic_local_bytes(const Config& c) { return 2 * c.local_gw * c.local_gh; }
// one wave's LDS strip: the row, up to three bytes in front of it (symbolic_body: the row sits at its global address's
// phase inside a dword), rounded to 16
__host__ __device__ inline int symbolic_strip_bytes(const Config& c) { return (symbolic_local_bytes(c) + 3 + 15) & ~15; }

// plane 1: the sprite variant of an object (render.hpp sprite_texture names the same textures)
__device__ __forceinline__ int symbolic_variant(const Obj& o, bool sleeping) {
  const int f = (o.fx < 0) ? 1 : (o.fx > 0) ? 2 : (o.fy < 0) ? 3 : 4;
  if (o.type == T_PLAYER) return sleeping ? 5 : f;
  if (o.type == T_ARROW) return f;
  if (o.type == T_PLANT) return o.aux > 300 ? 1 : 0;
  return 0;
}

// strip: 4-byte aligned, symbolic_strip_bytes(cfg) bytes of LDS owned by this wave.  local: [N][2][gw][gh] bytes or null;
// stats: [N][n_items + 4] floats or null.
template <class W, int MAP>
__device__ __forceinline__ void symbolic_body(W& w, uint8_t* strip, int env, const Config& cfg, const TablePtrs& tb, const StatePtrs& st,
                                              const uint8_t* mask, uint8_t* local, float* stats) {
  if (env >= cfg.num_envs) return;
  if (mask && !mask[env]) return;
  const EnvRec* rec = st.rec + env;
  const Obj* objs = st.objs + (size_t)env * cfg.max_objects;
  const Obj player = objs[1];   // slot 1 (env.py:76-78: the first object of every world)
  const bool sleeping = rec->sleeping != 0;
  if (local) {
    const int gw = cfg.local_gw, gh = cfg.local_gh, cells = gw * gh, n = 2 * cells;
    const int Wd = cfg.W, H = cfg.H;
    const int x0 = (int)player.x - gw / 2, y0 = (int)player.y - gh / 2;
    const int base = tb.rules->n_materials;   // len(mat_ids) = n_materials + 1 (None); class ids follow (engine.py:256-258)
    uint8_t* row = local + (size_t)env * n;
    // the strip holds the row at the same phase inside a dword as global memory does, so that aligned dwords of the one are
    // aligned dwords of the other
    const int phase = (int)((uintptr_t)row & 3);
    uint8_t* win = strip + phase;
    W::assume_lds(win);
    const uint8_t* mat = st.mat + (size_t)env * Wd * H;
    const uint16_t* objmap = MAP ? st.objmap + (size_t)env * Wd * H : nullptr;
    w.wave_for(cells, [&](int c) {
      const int x = c / gh, y = c - x * gh;
      const int wx = x0 + x, wy = y0 + y;
      int id = 0, var = 0;
      if (wx >= 0 && wx < Wd && wy >= 0 && wy < H) {
        const int cell = wx * H + wy;
        id = mat[cell];
        if (MAP) {
          const int slot = objmap[cell];
          if (slot > 0 && slot < cfg.max_objects) {
            const Obj o = objs[slot];
            id = base + o.type;
            var = symbolic_variant(o, sleeping);
          }
        }
      }
      win[c] = (uint8_t)id;
      win[cells + c] = (uint8_t)var;
    });
    if (!MAP) {
      w.wsync();
      int nobj = rec->nobj;
      if (nobj > cfg.max_objects) nobj = cfg.max_objects;
      w.wave_for(nobj - 1, [&](int k) {
        const Obj o = objs[k + 1];
        const int gx = (int)o.x - x0, gy = (int)o.y - y0;
        if (o.type != T_NONE && gx >= 0 && gx < gw && gy >= 0 && gy < gh) {
          const int c = gx * gh + gy;
          win[c] = (uint8_t)(base + o.type);
          win[cells + c] = (uint8_t)symbolic_variant(o, sleeping);
        }
      });
    }
    w.wsync();
    // out: the bytes in front of the first aligned dword, the dwords, the bytes behind the last one
    int head = (4 - phase) & 3;
    if (head > n) head = n;
    const int nd = (n - head) >> 2, tail0 = head + 4 * nd;
    const uint32_t* src = (const uint32_t*)(win + head);
    uint32_t* dst = (uint32_t*)(row + head);
    w.wave_for(nd, [&](int i) { dst[i] = src[i]; });
    w.wave_for(head + (n - tail0), [&](int i) {
      const int b = i < head ? i : tail0 + (i - head);
      row[b] = win[b];
    });
  }
  if (stats) {
    const int ni = tb.rules->n_items;
    float* srow = stats + (size_t)env * (ni + kSymbolicStatsExtra);
    int step = rec->step;
    if (step >= cfg.n_daylight) step = cfg.n_daylight - 1;   // (ST_STEP_OVERFLOW is already set: never past the table)
    if (step < 0) step = 0;
    w.wave_for(ni + kSymbolicStatsExtra, [&](int i) {
      float v;
      if (i < ni) v = (float)rec->inv[i];
      else if (i == ni) v = (float)player.fx;
      else if (i == ni + 1) v = (float)player.fy;
      else if (i == ni + 2) v = sleeping ? 1.0f : 0.0f;
      else v = (float)tb.daylight[step];
      srow[i] = v;
    });
  }
}

}  // namespace crafter
