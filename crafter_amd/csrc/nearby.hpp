// Nearby queries (crafter_nearby): per env, what World.nearby(player.pos, distance) and World.count(material) say (engine.py:95-110)
// as counts per class over a window around the player, and the k nearest objects of chosen classes as rows.  The definition --
// the two window rules, the columns, the order of the rows -- is include/crafter_hip_nearby.h's; crafter_amd.nearby_host is the
// numpy mirror, integer for integer.  Read-only: the three outputs are the only stores to global memory, no global atomics, no
// RNG draw, nothing of the world pool is looked at.
//
// Like audit.hpp it indexes NOTHING it has not bounded: rec.nobj is clamped to the table, a record's type / x / y are compared
// with T_PLANT / W / H before they address a counter or form a key, a slot id read from objmap is compared with max_objects, a
// material byte addresses a counter only inside 1 .. n_materials.  cfg and the rules are the handle's own and trusted.
//
// One workgroup per env, its tables in LDS (nearby_lds_words): a head (the number of objects that qualified, the winner of each
// selection round), one counter per class, and -- only with k > 0 -- one sort key per candidate.  Worlds of at most 64 x 64 cells
// take a workgroup of ONE wave (its barriers cost nothing; a masked row, the batch tail and a row never reset leave at once),
// any other world 256 threads.  Four phases between barriers:
//   clear
//   census    the window's columns (column x is H contiguous bytes) in 16-byte loads where H is a multiple of 16 -- every column
//             then starts 16-byte aligned -- kNearRound of them in flight per thread, a byte path for heights such as 30.  A thread
//             counts a RUN of equal bytes in a register and adds it to the class counter with one LDS add: terrain comes in
//             patches, a 16-byte group is two or three runs.  Integer adds commute, so no count depends on lane order.
//   objects   the slot table, lane-strided, 16-byte records (any world); or, where objmap is state (MAP 1) and the window has
//             fewer cells than the table has slots, objmap over the window and only the records it names.  NearQuery::walk
//             forces either (the CPU harness; the library passes -1).  Each object inside the window is counted by class; one
//             whose class is in `classes` stores its key  (dx^2 + dy^2) << 11 | (dx + 511) << 1 | (dy > 0)  at its candidate
//             index (its slot, or its window cell): for equal distance and dx the two possible dy differ in sign, so the key
//             orders by distance, dx, dy, and a cell holds one object, so keys are unique.  |dx| <= 511: kNearMaxSide.
//   select    min(n, k) rounds: every thread takes the least of its keys above the last winner, one lds_min per thread names
//             the round's winner, and the thread that holds that key writes the row.  A minimum does not depend on lane order.
//             Rows from min(n, k) on are written as zeros.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/crafter_hip_nearby.h"
#include "symbolic.hpp"   // symbolic_variant: the facing code is plane 1's
#include "types.hpp"

namespace crafter {

constexpr int kNearMaxEnts = CRAFTER_NEARBY_MAX_ENTS;
constexpr int kNearRow = CRAFTER_NEARBY_ROW;
constexpr int kNearMaxSide = CRAFTER_NEARBY_MAX_SIDE;
constexpr int kNearThreads = 64;          // worlds of at most 64 x 64 cells: one wave per env
constexpr int kNearWideThreads = 256;     // any other world
constexpr int kNearRound = 4;             // 16-byte loads a thread has in flight per round of the census
constexpr int kNearHead = 8 + kNearMaxEnts;   // word 0: the objects that qualified; words 8 ..: the winner of each round
constexpr int kNearBest = 8;
constexpr int kNearClasses = 32;          // counters (the class count is at most 31 + none)
constexpr int kNearMaxLds = 64 * 1024;
constexpr int kNearMaxDistance = 1 << 20; // any larger distance selects the same cells
constexpr uint32_t kNearNone = 0xFFFFFFFFu;

// what travels by value as a kernel argument
struct NearQuery {
  int32_t distance, flags;
  uint32_t classes;
  int32_t k;
  int32_t walk;   // the object pass: -1 whichever is shorter, 0 the slot table, 1 objmap over the window (MAP 1 only)
};

__host__ __device__ inline bool near_in_wave(const Config& c) { return c.W <= 64 && c.H <= 64; }
__host__ __device__ inline size_t near_lds_words(const Config& c, int k) { return (size_t)kNearHead + kNearClasses + (k > 0 ? (size_t)c.max_objects : 0); }
// the class ids of the objects, CRAFTER_T_PLAYER .. CRAFTER_T_PLANT
__host__ __device__ inline uint32_t near_object_classes(int n_materials) { return 0x3Fu << (n_materials + 1); }
// 0 when the query is one crafter_nearby accepts, else the number of the reason (near_error_text)
__host__ __device__ inline int near_check(const Config& c, int n_materials, int distance, int flags, uint32_t classes, int k, const void* counts,
                                          const void* ents, const void* n) {
  if (n_materials + 1 + T_PLANT > 31) return 8;
  if (k < 0 || k > kNearMaxEnts) return 1;
  if (flags != CRAFTER_NEARBY_CLIP && flags != CRAFTER_NEARBY_NUMPY) return 2;
  if (classes & ~near_object_classes(n_materials)) return 3;
  if (flags == CRAFTER_NEARBY_NUMPY && distance < 0) return 4;
  if (!counts) return 5;
  if (k > 0 && (!ents || !n)) return 6;
  if (k > 0 && (c.W > kNearMaxSide || c.H > kNearMaxSide || near_lds_words(c, k) * 4 > (size_t)kNearMaxLds)) return 7;
  return 0;
}
inline const char* near_error_text(int reason) {
  switch (reason) {
    case 1: return "k must lie in 0 .. CRAFTER_NEARBY_MAX_ENTS (32)";
    case 2: return "flags must be CRAFTER_NEARBY_CLIP or CRAFTER_NEARBY_NUMPY";
    case 3: return "classes names a class that is no object class (n_materials + 1 .. n_materials + 6)";
    case 4: return "CRAFTER_NEARBY_NUMPY takes a distance >= 0";
    case 5: return "counts is null";
    case 6: return "ents or n is null with k > 0";
    case 7: return "k > 0 on a world with a side above 512 or a slot table beyond 64 KiB of LDS";
    case 8: return "rules with more than 31 classes";
    default: return "";
  }
}

// one axis of the window, [lo, hi) (empty: lo >= hi), for the player at p on an axis of length L
__host__ __device__ inline void near_axis(int p, int d, int L, int flags, int& lo, int& hi) {
  if (d < 0) {
    lo = 0, hi = L;
    return;
  }
  if (d > kNearMaxDistance) d = kNearMaxDistance;
  lo = p - d;
  if (flags == CRAFTER_NEARBY_NUMPY) {   // a negative slice start counts from the end; one still negative is clipped to 0
    if (lo < 0) lo += L;
  }
  if (lo < 0) lo = 0;
  hi = p + d + 1 < L ? p + d + 1 : L;
}

__device__ __forceinline__ uint32_t near_key(int dx, int dy) {
  return ((uint32_t)(dx * dx + dy * dy) << 11) | ((uint32_t)(dx + kNearMaxSide - 1) << 1) | (dy > 0 ? 1u : 0u);
}

struct NearQuad {
  uint32_t v[4];
};
// 16 bytes at a 16-byte aligned address: one global_load_dwordx4
__device__ __forceinline__ NearQuad near_load16(const void* p) {
  NearQuad q;
  __builtin_memcpy(&q, __builtin_assume_aligned(p, 16), 16);
  return q;
}

// lds: near_lds_words(cfg, q.k) words owned by this workgroup, which serves one env.  MAP 1: objmap is state (maps in global memory).
// counts: [N][1 + n_materials + 6]; ents: [N][q.k][6] and n: [N], or null with q.k == 0.
template <class W, int MAP>
__device__ __forceinline__ void nearby_body(W& w, uint32_t* lds, int env, const Config& cfg, const TablePtrs& tb, const StatePtrs& st,
                                            const uint8_t* mask, const NearQuery& q, int32_t* counts, int16_t* ents, int32_t* n) {
  if (env >= cfg.num_envs) return;
  if (mask && !mask[env]) return;   // (the whole workgroup: no barrier has been met)
  constexpr int NT = W::kThreads;
  const Rules& R = *tb.rules;
  const EnvRec* rec = st.rec + env;
  const int Wd = cfg.W, H = cfg.H, C = cfg.max_objects, nm = R.n_materials, ncls = nm + 1 + T_PLANT;
  const int K = (!ents || !n || q.k < 0) ? 0 : q.k > kNearMaxEnts ? kNearMaxEnts : q.k;
  const Obj* objs = st.objs + (size_t)env * C;
  const uint8_t* mat = st.mat + (size_t)env * Wd * H;
  const uint16_t* objmap = MAP ? st.objmap + (size_t)env * Wd * H : nullptr;
  int32_t* crow = counts + (size_t)env * ncls;
  int16_t* erow = K ? ents + (size_t)env * K * kNearRow : nullptr;
  const int px = W::uni((int)objs[1].x), py = W::uni((int)objs[1].y);   // slot 1 (env.py:76-78: the first object of every world)
  if (W::uni(rec->episode) == 0 || px >= Wd || py >= H) {   // never reset: nothing of the row means anything
    w.block_for(ncls, [&](int i) { crow[i] = 0; });
    w.block_for(K * kNearRow, [&](int i) { erow[i] = 0; });
    if (K) w.block_for(1, [&](int) { n[env] = 0; });
    return;
  }
  int nobj = W::uni(rec->nobj);
  nobj = nobj < 1 ? 1 : nobj > C ? C : nobj;
  const bool sleeping = W::uni(rec->sleeping) != 0;
  int x0, x1, y0, y1;
  near_axis(px, q.distance, Wd, q.flags, x0, x1);
  near_axis(py, q.distance, H, q.flags, y0, y1);
  const int ww = x1 > x0 ? x1 - x0 : 0, hh = y1 > y0 ? y1 - y0 : 0, wcells = ww && hh ? ww * hh : 0;
  // objmap over the window: only where it is state, and with k > 0 only while a cell index fits the key table
  const bool by_map = MAP && (K == 0 || wcells <= C) && (q.walk < 0 ? wcells < nobj - 1 : q.walk != 0);
  const int span = by_map ? wcells : nobj;   // candidate indices: window cells, or slots

  uint32_t* head = lds;
  int32_t* cnt = (int32_t*)(lds + kNearHead);
  uint32_t* keys = lds + kNearHead + kNearClasses;
  W::assume_lds(lds);
  w.block_for(kNearHead + kNearClasses + (K ? span : 0), [&](int i) { lds[i] = (i >= kNearBest && i < kNearHead) || i >= kNearHead + kNearClasses ? kNearNone : 0u; });
  w.sync();

  // the census: bytes lo .. hi - 1 of a group of 16, runs of equal bytes counted in a register
  auto group = [&](const NearQuad& g, int lo, int hi) {
    int cur = 0, run = 0;
    auto flush = [&]() {
      if (run && cur >= 1 && cur <= nm) w.lds_add(cnt + cur, run);
    };
#pragma unroll
    for (int k = 0; k < 4; k++) {   // (unrolled over the words only: g stays in registers, the byte loop stays a loop)
      uint32_t word = g.v[k];
#pragma clang loop unroll(disable)
      for (int j = 4 * k; j < 4 * k + 4; j++, word >>= 8) {
        if (j < lo || j >= hi) continue;
        const int m = (int)(word & 0xFFu);
        if (m != cur) {
          flush();
          cur = m, run = 0;
        }
        run++;
      }
    }
    flush();
  };
  if (wcells && H % 16 == 0) {
    const int g0 = y0 >> 4, ng = ((y1 + 15) >> 4) - g0, items = ww * ng, rounds = (items + NT * kNearRound - 1) / (NT * kNearRound);
    w.block_for(rounds * NT, [&](int i) {
      const int first_item = (i / NT) * NT * kNearRound + i % NT;
      NearQuad g[kNearRound];
      int gy[kNearRound];
#pragma unroll
      for (int r = 0; r < kNearRound; r++) {   // (unpredicated, clamped: all in flight together)
        const int it = first_item + NT * r < items ? first_item + NT * r : items - 1;
        const int cx = it / ng;
        gy[r] = 16 * (g0 + it - cx * ng);
        g[r] = near_load16(mat + (size_t)(x0 + cx) * H + gy[r]);
      }
#pragma unroll
      for (int r = 0; r < kNearRound; r++)
        if (first_item + NT * r < items) group(g[r], y0 - gy[r], y1 - gy[r]);
    });
  } else if (wcells) {   // a column that starts at any byte: sixteen byte loads a group
    const int ng = (hh + 15) >> 4;
    w.block_for(ww * ng, [&](int i) {
      const int cx = i / ng, ys = y0 + 16 * (i - cx * ng);
      const uint8_t* col = mat + (size_t)(x0 + cx) * H;
      NearQuad g = {{0u, 0u, 0u, 0u}};
#pragma unroll
      for (int j = 0; j < 16; j++)   // (unpredicated, clamped: all in flight together)
        g.v[j >> 2] |= (uint32_t)col[ys + j < y1 ? ys + j : y1 - 1] << (8 * (j & 3));
      group(g, 0, y1 - ys);
    });
  }

  // the objects inside the window: counted by class; a key for those whose class is in q.classes
  {
    int found = 0;
    auto object = [&](const Obj& o, int x, int y, int index) {
      const int cls = nm + o.type;
      w.lds_add(cnt + cls, 1);
      if (K && ((q.classes >> cls) & 1u)) {
        keys[index] = near_key(x - px, y - py);
        found++;
      }
    };
    if (by_map) {
      w.block_for(wcells, [&](int i) {
        const int cx = i / hh, x = x0 + cx, y = y0 + i - cx * hh;
        const int slot = objmap[x * H + y];
        if (slot < 1 || slot >= C) return;
        const Obj o = objs[slot];
        if (o.type != T_NONE && o.type <= T_PLANT) object(o, x, y, i);
      });
    } else if (wcells) {
      w.block_for(nobj - 1, [&](int i) {
        const Obj o = objs[i + 1];
        const int x = o.x, y = o.y;
        if (o.type != T_NONE && o.type <= T_PLANT && x >= x0 && x < x1 && y >= y0 && y < y1) object(o, x, y, i + 1);
      });
    }
    if (found) w.lds_add((int32_t*)head, found);
  }
  w.sync();

  w.block_for(ncls, [&](int i) { crow[i] = i == 0 ? wcells : cnt[i]; });
  if (!K) return;
  const int total = W::uni((int)head[0]), rows = total < K ? total : K;
  uint32_t last = 0;
  for (int j = 0; j < rows; j++) {
    w.each_thread([&](int t) {
      uint32_t least = kNearNone;
      for (int i = t; i < span; i += NT) {
        const uint32_t key = keys[i];
        if ((j == 0 || key > last) && key < least) least = key;
      }
      if (least != kNearNone) w.lds_min(head + kNearBest + j, least);
    });
    w.sync();
    last = (uint32_t)W::uni((int)head[kNearBest + j]);
    w.block_for(span, [&](int i) {
      if (keys[i] != last) return;
      int slot = i, x, y;
      if (by_map) {
        const int cx = i / hh;
        x = x0 + cx, y = y0 + i - cx * hh;
        slot = objmap[x * H + y];
        if (slot < 1 || slot >= C) slot = 0;   // (never: the object pass read the same cell)
      }
      const Obj o = objs[slot];
      if (!by_map) x = o.x, y = o.y;
      const int aux = o.aux > 32767 ? 32767 : o.aux < -32768 ? -32768 : o.aux;
      int16_t* row = erow + j * kNearRow;
      row[0] = (int16_t)(nm + o.type);
      row[1] = (int16_t)(x - px);
      row[2] = (int16_t)(y - py);
      row[3] = (int16_t)(o.type == T_PLAYER ? rec->inv[R.item_health] : (int)o.health);
      row[4] = (int16_t)symbolic_variant(o, sleeping);
      row[5] = (int16_t)aux;
    });
  }
  w.block_for((K - rows) * kNearRow, [&](int i) { erow[rows * kNearRow + i] = 0; });
  w.block_for(1, [&](int) { n[env] = total; });
}

}  // namespace crafter
