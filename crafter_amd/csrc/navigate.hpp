// Navigation queries (crafter_navigate): per env and per target set, the walking distance from the player to the nearest
// target cell, the first move of a shortest walk, and whether the player faces a target now.  The definition is
// include/crafter_hip_navigate.h's: a cell's class is SemanticView's id (engine.py:251-264: n_materials + type where an object
// stands, else the material id), T_k the cells whose class is in targets[k] without the player's own, P the cells whose
// material is in `passable` and that hold no object (Object.is_free, objects.py:44-47) plus the player's cell, dist 0 on T_k
// and 1 + the least neighbour inside P.  Read-only: no RNG draw, no byte of state changes, nothing of the world pool is looked at.
//
// A breadth-first search as a bitboard flood: a board holds one bit per cell, column x as bits y, and one sweep is
//   R' = R | ((R << 1 | R >> 1 | R[x - 1] | R[x + 1]) & P)            R_0 = T_k
// The player's bit enters R in sweep number dist; R stops growing without it where no walk exists.  P has no bit at or beyond
// row H and no column at or beyond W, so nothing a shift or a neighbour column carries there survives the AND.  The first
// move needs no per-cell distance: a neighbour n of the player has dist(n) = dist - 1 exactly when it is in the R the last
// sweep started from.
//
// Two geometries:
//   W <= 64 and H <= 64   navigate_body: one wave per env, no barrier.  Lane x holds column x of a board in a register pair
//                         (lv slots), the neighbour columns come through lane_fetch (ds_bpermute), the two loop tests are one
//                         ballot each.  P is built once, then the targets run one after the other.
//   any other area        navigate_lds_body: one workgroup per env, the boards in LDS as ceil(H / 32) words per column, the
//                         same recurrence with barriers between sweeps.  Correct, not fast.
// Two ways to the objects, as in symbolic.hpp and legal.hpp:
//   MAP 0  (worlds staged in LDS by the step kernels: StatePtrs.objmap is never written) the slot table, slots 1 .. nobj - 1,
//          live records only.  Their cells reach the boards by lds_or: in the register geometry through a staging strip of
//          64 x 2 words per wave.
//   MAP 1  (maps in global memory) objmap is state: a cell's slot, then the record's type.  Holes (slot 0) and free records
//          (T_NONE) do not count.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/crafter_hip_navigate.h"
#include "types.hpp"

namespace crafter {

constexpr int kNavMaxTargets = CRAFTER_NAV_MAX_TARGETS;
constexpr int kNavThreads = 256;                  // register geometry: four envs per workgroup
constexpr int kNavEnvs = kNavThreads / 64;
constexpr int kNavStripWords = 128;               // ... and a wave's staging strip: 64 columns of two words
constexpr int kNavWideThreads = 256;              // LDS geometry: one env per workgroup
constexpr int kNavBoards = 5;                     // P, the object cells, T, and R twice
constexpr int kNavMaxLds = 64 * 1024;

// what travels by value as a kernel argument: nothing on the device to allocate or keep alive
struct NavQuery {
  uint32_t targets[kNavMaxTargets];
  uint32_t passable;
  int32_t k;
};

__host__ __device__ inline bool nav_in_registers(const Config& c) { return c.W <= 64 && c.H <= 64; }
__host__ __device__ inline int nav_col_words(const Config& c) { return (c.H + 31) / 32; }
__host__ __device__ inline size_t nav_lds_bytes(const Config& c) { return ((size_t)kNavBoards * c.W * nav_col_words(c) + 4) * 4; }
// the class ids of the objects, CRAFTER_T_PLAYER .. CRAFTER_T_PLANT
__host__ __device__ inline uint32_t nav_object_classes(int n_materials) { return 0x3Fu << (n_materials + 1); }
// 0 when the query is one crafter_navigate accepts, else the number of the reason (navigate_error_text)
__host__ __device__ inline int nav_check(int n_materials, const uint32_t* targets, int k, uint32_t passable) {
  const int classes = n_materials + 1 + T_PLANT;
  if (classes > 31) return 5;
  if (k < 1 || k > kNavMaxTargets) return 1;
  if (!targets) return 2;
  for (int i = 0; i < k; i++)
    if (targets[i] == 0 || (targets[i] & 1u) || (targets[i] >> classes)) return 3;
  if ((passable & 1u) || (passable >> (n_materials + 1))) return 4;
  return 0;
}
inline const char* nav_error_text(int reason) {
  switch (reason) {
    case 1: return "k must lie in 1 .. CRAFTER_NAV_MAX_TARGETS (16)";
    case 2: return "targets is null";
    case 3: return "targets: a set is empty, names class 0 (none) or a class id at or above the class count";
    case 4: return "passable names material 0 (none) or an id above the materials";
    case 5: return "rules with more than 31 classes";
    default: return "";
  }
}

// the move action of each direction (action_arg 0 .. 3 = left, right, up, down), one byte each, 0xFF: none
__device__ __forceinline__ uint32_t nav_move_actions(const Rules& R) {
  uint32_t acts = 0xFFFFFFFFu;
  for (int a = (R.n_actions < MAX_ACTIONS ? R.n_actions : MAX_ACTIONS) - 1; a >= 0; a--)
    if (R.action_kind[a] == A_MOVE && R.action_arg[a] < 4) acts = (acts & ~(0xFFu << (8 * R.action_arg[a]))) | ((uint32_t)a << (8 * R.action_arg[a]));
  return acts;
}
__device__ __forceinline__ int32_t nav_action_of(uint32_t acts, int dir) {
  const uint32_t a = dir < 0 ? 0xFFu : (acts >> (8 * dir)) & 0xFFu;
  return a == 0xFFu ? -1 : (int32_t)a;
}
__device__ __forceinline__ uint32_t nav_in_set(uint32_t set, int cls) { return cls < 32 ? (set >> cls) & 1u : 0u; }

// ---------------------------------------------------------------------------------------------- boards in registers
template <class W>
__device__ __forceinline__ uint64_t nav_get2(const W& w, int lo, int hi, int l) {
  return (uint64_t)w.lane_get(lo, l) | ((uint64_t)w.lane_get(hi, l) << 32);
}
template <class W>
__device__ __forceinline__ uint64_t nav_fetch2(const W& w, int lo, int hi, int from, int l) {
  return (uint64_t)w.lane_fetch(lo, from, l) | ((uint64_t)w.lane_fetch(hi, from, l) << 32);
}

struct NavQuad {
  uint32_t v[4];
};
// bit y of the result: the material col[y] is in `set`, y < H <= 64.  A column of a multiple of 16 cells is read in 16-byte
// loads (W H is then a multiple of 16 as well: every column starts at a 16-byte aligned address of the buffer)
__device__ __forceinline__ uint64_t nav_mat_column(const uint8_t* col, int H, uint32_t set) {
  uint64_t b = 0;
  if (H % 16 == 0) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (16 * j < H) {
        NavQuad q;
        __builtin_memcpy(&q, __builtin_assume_aligned(col + 16 * j, 16), 16);
#pragma unroll
        for (int i = 0; i < 16; i++) b |= (uint64_t)nav_in_set(set, (int)((q.v[i >> 2] >> (8 * (i & 3))) & 0xFFu)) << (16 * j + i);
      }
    }
  } else {
    for (int y = 0; y < H; y++) b |= (uint64_t)nav_in_set(set, col[y]) << y;
  }
  return b;
}

// MAP 1: bit y = the class of cell (x, y) is in `set`
__device__ __forceinline__ uint64_t nav_class_column(const uint8_t* col, const uint16_t* slots, const Obj* objs, int H, int max_objects,
                                                     int n_materials, uint32_t set) {
  uint64_t b = 0;
  for (int y = 0; y < H; y++) {
    int cls = col[y];
    const int slot = slots[y];
    if (slot > 0 && slot < max_objects) {
      const int type = objs[slot].type;
      if (type != T_NONE) cls = n_materials + type;
    }
    b |= (uint64_t)nav_in_set(set, cls) << y;
  }
  return b;
}

// MAP 0: the cells of the live objects whose class is in `set`, ORed into the wave's (cleared) staging strip
template <class W>
__device__ __forceinline__ void nav_stage(W& w, uint32_t* strip, const Obj* objs, int nobj, int Wd, int H, int n_materials, uint32_t set) {
  w.wsync();
  w.lanes(0, 64, [&](int i, int) { strip[2 * i] = strip[2 * i + 1] = 0u; });
  w.wsync();
  for (int base = 1; base < nobj; base += 64)
    w.lanes(base, nobj, [&](int s, int) {
      const Obj o = objs[s];
      if (o.type != T_NONE && nav_in_set(set, n_materials + o.type) && (int)o.x < Wd && (int)o.y < H)
        w.lds_or(strip + 2 * (int)o.x + ((int)o.y >> 5), 1u << (o.y & 31));
    });
  w.wsync();
}

struct NavEnv {
  const uint8_t* mat;
  const uint16_t* objmap;
  const Obj* objs;
  int Wd, H, nobj, max_objects, n_materials, px, py;
};

// Slots LO, HI := the board of the cells whose class is in `set`; the player's own cell in (player 1) or out (0).  MAP 0 reads the
// board of all object cells from slots 2, 3.
template <class W, int MAP, int LO, int HI>
__device__ __forceinline__ void nav_board(W& w, uint32_t* strip, const NavEnv& e, uint32_t set, int player) {
  const uint32_t objset = set & nav_object_classes(e.n_materials), matset = set & ~nav_object_classes(e.n_materials);
  if (!MAP && objset) nav_stage(w, strip, e.objs, e.nobj, e.Wd, e.H, e.n_materials, objset);
  w.lane_set2(LO, HI, 0, e.Wd, [&](int x, int l) {
    uint64_t b;
    if (MAP) {
      b = nav_class_column(e.mat + x * e.H, e.objmap + x * e.H, e.objs, e.H, e.max_objects, e.n_materials, set);
    } else {
      b = matset ? nav_mat_column(e.mat + x * e.H, e.H, matset) & ~nav_get2(w, 2, 3, l) : 0ull;
      if (objset) b |= (uint64_t)strip[2 * x] | ((uint64_t)strip[2 * x + 1] << 32);
    }
    if (x == e.px) b = player ? b | (1ull << e.py) : b & ~(1ull << e.py);
    return b;
  });
}

// one sweep: slots DL, DH := the board of slots SL, SH grown by one step inside P (slots 0, 1).  Never in place: the CPU
// harness stores lane by lane
template <class W, int SL, int SH, int DL, int DH>
__device__ __forceinline__ void nav_sweep(W& w, int Wd) {
  w.lane_set2_all(DL, DH, [&](int l) {
    const uint64_t r = nav_get2(w, SL, SH, l);
    uint64_t left = nav_fetch2(w, SL, SH, (l + 63) & 63, l), right = nav_fetch2(w, SL, SH, (l + 1) & 63, l);
    if (l == 0) left = 0;            // (no column on that side: the fetch wrapped around)
    if (l >= Wd - 1) right = 0;
    return r | (((r << 1) | (r >> 1) | left | right) & nav_get2(w, 0, 1, l));
  });
}
// after a sweep from S to D: 1 the player's bit is in D, 2 D grew (and the bit is not in it), 0 neither
template <class W, int SL, int SH, int DL, int DH>
__device__ __forceinline__ int nav_progress(W& w, int px, int py) {
  const uint64_t hit = W::uni64(w.ballot(0, 64, [&](int l) { return l == px && ((nav_get2(w, DL, DH, l) >> py) & 1ull) != 0; }));
  if (hit) return 1;
  const uint64_t grew = W::uni64(w.ballot(0, 64, [&](int l) { return nav_get2(w, DL, DH, l) != nav_get2(w, SL, SH, l); }));
  return grew ? 2 : 0;
}
// bit (x, y) of the board in slots LO, HI, for wave-uniform x, y; 0 outside the world
template <class W, int LO, int HI>
__device__ __forceinline__ bool nav_bit(const W& w, int x, int y, int Wd, int H) {
  if (x < 0 || x >= Wd || y < 0 || y >= H) return false;
  const uint32_t lo = w.lane_read(LO, x & 63), hi = w.lane_read(HI, x & 63);
  return (((y < 32 ? lo : hi) >> (y & 31)) & 1u) != 0;
}
// the first direction (left, right, up, down) whose neighbour is in the board of slots LO, HI; -1: none
template <class W, int LO, int HI>
__device__ __forceinline__ int nav_first_dir(const W& w, int px, int py, int Wd, int H) {
  return nav_bit<W, LO, HI>(w, px - 1, py, Wd, H) ? 0 : nav_bit<W, LO, HI>(w, px + 1, py, Wd, H) ? 1 :
         nav_bit<W, LO, HI>(w, px, py - 1, Wd, H) ? 2 : nav_bit<W, LO, HI>(w, px, py + 1, Wd, H) ? 3 : -1;
}

// strip: kNavStripWords words of LDS owned by this wave.  dist, first: [N][q.k]; facing: [N][q.k] or null.
// lv slots: 0, 1 P; 2, 3 the object cells (MAP 0); 4, 5 T_k; 6, 7 and 8, 9 R, by turns.
template <class W, int MAP>
__device__ __forceinline__ void navigate_body(W& w, uint32_t* strip, int env, const Config& cfg, const TablePtrs& tb, const StatePtrs& st,
                                              const uint8_t* mask, const NavQuery& q, int32_t* dist, int32_t* first, uint8_t* facing) {
  if (env >= cfg.num_envs) return;
  if (mask && !mask[env]) return;
  const Rules& R = *tb.rules;
  const EnvRec* rec = st.rec + env;
  NavEnv e;
  e.Wd = cfg.W, e.H = cfg.H, e.max_objects = cfg.max_objects, e.n_materials = R.n_materials;
  e.objs = st.objs + (size_t)env * cfg.max_objects;
  e.mat = st.mat + (size_t)env * e.Wd * e.H;
  e.objmap = MAP ? st.objmap + (size_t)env * e.Wd * e.H : nullptr;
  e.nobj = W::uni(rec->nobj);
  if (e.nobj > cfg.max_objects) e.nobj = cfg.max_objects;
  const Obj player = e.objs[1];   // slot 1 (env.py:76-78: the first object of every world)
  e.px = W::uni((int)player.x), e.py = W::uni((int)player.y);
  if (e.px >= e.Wd || e.py >= e.H) return;   // (never: a record the step kernels would have flagged)
  const int fx = e.px + player.fx, fy = e.py + player.fy;
  const uint32_t acts = nav_move_actions(R);
  if (!MAP) {
    nav_stage(w, strip, e.objs, e.nobj, e.Wd, e.H, e.n_materials, nav_object_classes(e.n_materials));
    w.lane_set2(2, 3, 0, e.Wd, [&](int x, int) { return (uint64_t)strip[2 * x] | ((uint64_t)strip[2 * x + 1] << 32); });
  }
  nav_board<W, MAP, 0, 1>(w, strip, e, q.passable, 1);
  const int K = q.k < kNavMaxTargets ? q.k : kNavMaxTargets;
  for (int t = 0; t < K; t++) {
    nav_board<W, MAP, 4, 5>(w, strip, e, q.targets[t], 0);
    const bool faced = nav_bit<W, 4, 5>(w, fx, fy, e.Wd, e.H);
    w.lane_set2(6, 7, 0, 64, [&](int, int l) { return nav_get2(w, 4, 5, l); });
    int d = 0, dir = -1, found = -1;
    for (;;) {
      nav_sweep<W, 6, 7, 8, 9>(w, e.Wd);
      d++;
      int p = nav_progress<W, 6, 7, 8, 9>(w, e.px, e.py);
      if (p == 1) {
        found = d;
        dir = nav_first_dir<W, 6, 7>(w, e.px, e.py, e.Wd, e.H);
      }
      if (p != 2) break;
      nav_sweep<W, 8, 9, 6, 7>(w, e.Wd);
      d++;
      p = nav_progress<W, 8, 9, 6, 7>(w, e.px, e.py);
      if (p == 1) {
        found = d;
        dir = nav_first_dir<W, 8, 9>(w, e.px, e.py, e.Wd, e.H);
      }
      if (p != 2) break;
    }
    w.lanes(0, 1, [&](int, int) {
      const size_t o = (size_t)env * K + t;
      dist[o] = found;
      first[o] = nav_action_of(acts, dir);
      if (facing) facing[o] = faced ? 1 : 0;
    });
  }
}

// ---------------------------------------------------------------------------------------------- boards in LDS
// lds: nav_lds_bytes(cfg) bytes owned by this workgroup, which serves one env.
template <class W, int MAP>
__device__ __forceinline__ void navigate_lds_body(W& w, uint32_t* lds, int env, const Config& cfg, const TablePtrs& tb, const StatePtrs& st,
                                                  const uint8_t* mask, const NavQuery& q, int32_t* dist, int32_t* first, uint8_t* facing) {
  if (env >= cfg.num_envs) return;
  if (mask && !mask[env]) return;   // (the whole workgroup: no barrier has been met)
  const Rules& R = *tb.rules;
  const EnvRec* rec = st.rec + env;
  const int Wd = cfg.W, H = cfg.H, wpc = nav_col_words(cfg), n = Wd * wpc, nm = R.n_materials;
  const Obj* objs = st.objs + (size_t)env * cfg.max_objects;
  const uint8_t* mat = st.mat + (size_t)env * Wd * H;
  const uint16_t* objmap = MAP ? st.objmap + (size_t)env * Wd * H : nullptr;
  int nobj = rec->nobj;
  if (nobj > cfg.max_objects) nobj = cfg.max_objects;
  const Obj player = objs[1];
  const int px = player.x, py = player.y;
  if (px >= Wd || py >= H) return;
  const int fx = px + player.fx, fy = py + player.fy;
  const uint32_t acts = nav_move_actions(R);
  const int pword = px * wpc + (py >> 5);
  const uint32_t pbit = 1u << (py & 31);
  uint32_t* P = lds;
  uint32_t* OA = lds + n;
  uint32_t* T = lds + 2 * n;
  uint32_t* RA = lds + 3 * n;
  uint32_t* RB = lds + 4 * n;
  uint32_t* flag = lds + 5 * n;
  W::assume_lds(lds);
  auto bit_at = [&](const uint32_t* board, int x, int y) {
    return x >= 0 && x < Wd && y >= 0 && y < H && ((board[x * wpc + (y >> 5)] >> (y & 31)) & 1u) != 0;
  };
  // board := the live objects' cells whose class is in `set`, ORed in (between barriers)
  auto add_objects = [&](uint32_t* board, uint32_t set) {
    w.block_for(nobj - 1, [&](int k) {
      const Obj o = objs[k + 1];
      if (o.type != T_NONE && nav_in_set(set, nm + o.type) && (int)o.x < Wd && (int)o.y < H)
        w.lds_or(board + (int)o.x * wpc + ((int)o.y >> 5), 1u << (o.y & 31));
    });
    w.sync();
  };
  // board := the cells whose class is in `set`, the player's own cell in or out
  auto build = [&](uint32_t* board, uint32_t set, int with_player) {
    w.block_for(n, [&](int i) {
      const int x = i / wpc, j = i - x * wpc;
      uint32_t v = 0;
      for (int b = 0; b < 32 && 32 * j + b < H; b++) {
        const int cell = x * H + 32 * j + b;
        int cls = mat[cell];
        if (MAP) {
          const int slot = objmap[cell];
          if (slot > 0 && slot < cfg.max_objects) {
            const int type = objs[slot].type;
            if (type != T_NONE) cls = nm + type;
          }
        }
        v |= nav_in_set(set, cls) << b;
      }
      if (!MAP) v &= ~OA[i];
      board[i] = v;
    });
    w.sync();
    if (!MAP && (set & nav_object_classes(nm))) add_objects(board, set);
    w.block_for(1, [&](int) { board[pword] = with_player ? board[pword] | pbit : board[pword] & ~pbit; });
    w.sync();
  };
  if (!MAP) {
    w.block_for(n, [&](int i) { OA[i] = 0u; });
    w.sync();
    add_objects(OA, nav_object_classes(nm));
  }
  build(P, q.passable, 1);
  const int K = q.k < kNavMaxTargets ? q.k : kNavMaxTargets;
  for (int t = 0; t < K; t++) {
    build(T, q.targets[t], 0);
    w.block_for(n, [&](int i) { RA[i] = T[i]; });
    uint32_t* src = RA;
    uint32_t* dst = RB;
    int d = 0, found = -1;
    for (;;) {
      w.block_for(1, [&](int) { *flag = 0u; });
      w.sync();
      w.block_for(n, [&](int i) {
        const int x = i / wpc, j = i - x * wpc;
        const uint32_t r = src[i];
        uint32_t nb = (r << 1) | (r >> 1);
        if (j > 0) nb |= src[i - 1] >> 31;
        if (j < wpc - 1) nb |= src[i + 1] << 31;
        if (x > 0) nb |= src[i - wpc];
        if (x < Wd - 1) nb |= src[i + wpc];
        const uint32_t v = r | (nb & P[i]);
        dst[i] = v;
        if (v != r) w.lds_or(flag, 1u);
      });
      w.sync();
      d++;
      const bool hit = (dst[pword] & pbit) != 0, grew = *flag != 0u;
      w.sync();   // (every thread has read the flag before the next sweep clears it)
      if (hit) found = d;
      if (hit || !grew) break;
      uint32_t* tmp = src;
      src = dst;
      dst = tmp;
    }
    w.block_for(1, [&](int) {
      int dir = -1;
      if (found > 0) dir = bit_at(src, px - 1, py) ? 0 : bit_at(src, px + 1, py) ? 1 : bit_at(src, px, py - 1) ? 2 : bit_at(src, px, py + 1) ? 3 : -1;
      const size_t o = (size_t)env * K + t;
      dist[o] = found;
      first[o] = nav_action_of(acts, dir);
      if (facing) facing[o] = bit_at(T, fx, fy) ? 1 : 0;
    });
    w.sync();
  }
}

}  // namespace crafter
