// Legal-action mask (crafter_legal_actions): legal[env][a] = 1 iff Player.update (objects.py:99-131), run on the env's state as it
// stands with action a, passes every guard of that action's branch -- for every action but a move, 0 means "this step does
// what noop does".  Every value is the reference's; target = pos + facing, (material, obj) = world[target], (None, None)
// outside the world; awake = not (sleeping and energy < max) (objects.py:103-108: a sleeping player short of energy has its
// action replaced by sleep, one with full energy wakes up and its action counts):
//   noop     always
//   move_*   objects.py:174-179, 36-47  awake, and the destination is inside the world, holds no object and its material is
//                                       in player_walkable_mask: legal iff the position would change (a blocked move still turns)
//   do       objects.py:181-212         awake, an object on target: a zombie, skeleton or cow, or a plant with grown > 300
//            objects.py:214-229         awake, none: water, or a collect rule whose `require` the inventory holds (the
//                                       `probability` draw is no guard)
//   sleep    objects.py:117-119         not sleeping and energy < max
//   place_*  objects.py:231-249         awake, no object on target, its material in `where`, `uses` in the inventory
//   make_*   objects.py:251-261         awake, every `nearby` material in World.nearby(pos, 1), `uses` in the inventory.  The
//                                       window has numpy's slice semantics (engine.py:95-98, env_core.hpp make): EMPTY when
//                                       x == 0 or y == 0, clipped at W - 1 / H - 1
// All guards are read from the uploaded rules (tb.rules), never from the compiled-in defaults.  Read-only: no RNG draw, no byte
// of state changes, nothing of the world pool is looked at.  The player is the first object updated (env.py:86-89), so the
// state before the step is all the guards see.
//
// One wave per env, no LDS, no workgroup barrier: a masked row or the batch tail returns at once.  The facts of the env are
// found once, wave-uniform -- the materials of the four neighbour cells and of target, which of the five hold an object, the
// record of the object on target, the OR of 1 << material over the 3 x 3 window (nine lanes, reduced by ballots) -- then lane
// a < n_actions evaluates action a and stores its byte.  Two ways to the objects, as in symbolic.hpp:
//   MAP 0  (worlds staged in LDS: StatePtrs.objmap is never written) the lanes stride over slots 1 .. nobj - 1 and compare each
//          live record's cell with the five cells.
//   MAP 1  (maps in global memory) objmap is state: five reads of it and one record load.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "types.hpp"

namespace crafter {

constexpr int kLegalThreads = 256;                    // four envs per workgroup
constexpr int kLegalEnvs = kLegalThreads / 64;
constexpr int kLegalCells = 5;                        // left, right, up, down (action_arg of a move), target

// every amount of the list is in the inventory
__device__ __forceinline__ bool legal_has(const EnvRec* rec, const ItemList& l) {
  bool ok = true;
  for (int i = 0; i < l.n && i < MAX_USES; i++) ok = ok && rec->inv[l.item[i]] >= l.amount[i];
  return ok;
}

// legal: [N][n_actions] bytes.
template <class W, int MAP>
__device__ __forceinline__ void legal_body(W& w, int env, const Config& cfg, const TablePtrs& tb, const StatePtrs& st,
                                           const uint8_t* mask, uint8_t* legal) {
  if (env >= cfg.num_envs) return;
  if (mask && !mask[env]) return;
  const Rules& R = *tb.rules;
  const EnvRec* rec = st.rec + env;
  const Obj* objs = st.objs + (size_t)env * cfg.max_objects;
  const Obj player = objs[1];   // slot 1 (env.py:76-78: the first object of every world)
  const int Wd = cfg.W, H = cfg.H, px = player.x, py = player.y;
  const uint8_t* mat = st.mat + (size_t)env * Wd * H;
  // the five cells: bit k of `inside` / `occupied`, byte k of `nbmat` (k < 4), `tmat`
  const int cx[kLegalCells] = {px - 1, px + 1, px, px, px + player.fx};
  const int cy[kLegalCells] = {py, py, py - 1, py + 1, py + player.fy};
  uint32_t inside = 0, occupied = 0, nbmat = 0;
  int tmat = 0, tslot = 0;
#pragma unroll
  for (int k = 0; k < kLegalCells; k++) {
    if (cx[k] >= 0 && cx[k] < Wd && cy[k] >= 0 && cy[k] < H) {
      inside |= 1u << k;
      const int m = mat[cx[k] * H + cy[k]];
      if (k < 4) nbmat |= (uint32_t)m << (8 * k);
      else tmat = m;
    }
  }
  if (MAP) {
    const uint16_t* objmap = st.objmap + (size_t)env * Wd * H;
#pragma unroll
    for (int k = 0; k < kLegalCells; k++) {
      if ((inside >> k) & 1u) {
        const int slot = objmap[cx[k] * H + cy[k]];
        if (slot > 0 && slot < cfg.max_objects) {
          occupied |= 1u << k;
          if (k == 4) tslot = slot;
        }
      }
    }
  } else {
    int nobj = W::uni(rec->nobj);
    if (nobj > cfg.max_objects) nobj = cfg.max_objects;
    for (int base = 1; base < nobj; base += 64) {
      // a lane's live record as its packed cell (coordinates are 16 bits wide: no cell packs to all ones)
      w.lane_set(0, base, nobj, [&](int s, int) {
        const Obj o = objs[s];
        return o.type != T_NONE ? (uint32_t)o.x | ((uint32_t)o.y << 16) : 0xFFFFFFFFu;
      });
#pragma unroll
      for (int k = 0; k < kLegalCells; k++) {
        if ((inside >> k) & 1u) {
          const uint64_t hit = W::uni64(w.lane_match(0, base, nobj, (uint32_t)cx[k] | ((uint32_t)cy[k] << 16)));
          if (hit) {
            occupied |= 1u << k;
            if (k == 4) tslot = base + __builtin_ctzll(hit);
          }
        }
      }
    }
  }
  bool hittable = false;   // objects.py:181-212: what `do` does something to
  if (tslot) {
    const Obj t = objs[tslot];
    hittable = t.type == T_ZOMBIE || t.type == T_SKELETON || t.type == T_COW || (t.type == T_PLANT && t.aux > 300);
  }
  // World.nearby(pos, 1): lane i < 9 holds the bit of window cell (i / 3 - 1, i % 3 - 1), nothing where numpy's slice has no cell
  w.lane_set(1, 0, 9, [&](int i, int) {
    const int x = px + i / 3 - 1, y = py + i % 3 - 1;
    return (px > 0 && py > 0 && x < Wd && y < H) ? 1u << (mat[x * H + y] & 31) : 0u;
  });
  uint32_t near = 0;
  for (int m = 1; m <= R.n_materials && m <= MAX_MATERIALS; m++)
    if (w.lane_ballot(1, 1u << m)) near |= 1u << m;

  const bool sleeping = rec->sleeping != 0;
  const bool tired = rec->inv[R.item_energy] < R.item_max[R.item_energy];
  const bool awake = !(sleeping && tired);
  const bool tfree = ((inside >> 4) & 1u) && !((occupied >> 4) & 1u);
  uint8_t* row = legal + (size_t)env * R.n_actions;
  w.lanes(0, R.n_actions < MAX_ACTIONS ? R.n_actions : MAX_ACTIONS, [&](int a, int) {
    const int kind = R.action_kind[a], arg = R.action_arg[a];
    bool ok = false;
    if (kind == A_NOOP) {
      ok = true;
    } else if (kind == A_MOVE) {
      if (arg < 4) {
        const int m = (nbmat >> (8 * arg)) & 0xFF;
        ok = awake && ((inside >> arg) & 1u) && !((occupied >> arg) & 1u) && m < 32 && ((R.player_walkable_mask >> m) & 1u);
      }
    } else if (kind == A_DO) {
      if ((occupied >> 4) & 1u) {
        ok = awake && hittable;
      } else if ((inside >> 4) & 1u) {
        ok = tmat == R.mat_water;
        if (tmat <= MAX_MATERIALS) {
          const CollectRule& cr = R.collect[tmat];
          ok = ok || (cr.valid && legal_has(rec, cr.require));
        }
        ok = ok && awake;
      }
    } else if (kind == A_SLEEP) {
      ok = !sleeping && tired;
    } else if (kind == A_PLACE) {
      if (arg < MAX_PLACE) {
        const PlaceRule& pr = R.place[arg];
        ok = awake && tfree && tmat < 32 && ((pr.where_mask >> tmat) & 1u) && legal_has(rec, pr.uses);
      }
    } else if (kind == A_MAKE) {
      if (arg < MAX_MAKE) {
        const MakeRule& mk = R.make[arg];
        ok = awake && (near & mk.nearby_mask) == mk.nearby_mask && legal_has(rec, mk.uses);
      }
    }
    row[a] = ok ? 1 : 0;
  });
}

}  // namespace crafter
