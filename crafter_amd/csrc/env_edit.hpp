// Edits of envs in place (crafter_edit_envs): `world[x, y] = material`, World.add / remove / move, assignments to an object's
// fields, to the inventory, to the player's counters and to the clock, between two steps.  What makes an edited row steppable
// is the same as for an authored world (env_worlds.hpp): the slot table in insertion order, the cell -> slot map, the chunk keys
// in first-touch order, the per-chunk census, nobj.  So no op writes a derived table: each one is REPLAYED through the calls the
// step kernels make -- Env::set_mat / obj_add / obj_remove / obj_move / set_health / set_aux (env_core.hpp) -- and everything
// derived comes out as the reference's.
//
//   replay_edits : wave 0 walks the env's tape as wave-uniform code
//   edit_body    : one workgroup per named env -- bind_lds, load_env, replay_edits, Env::compact (a step ends on it too: no hole
//                  outlives the kernel that made it), store_env -- under edit_layout (lds_layout.hpp)
//
// The instance is the generic Env<W, uint16_t> the reset kernels run: an LDS-resident world's maps and slot table are staged and
// its slot map derived, as in a step; a large world's maps and slot table are edited where they live, in global memory.  The step
// kernel of large worlds keeps a cache of slot records (env_core.hpp FarSlot), but only for the length of one launch -- it is
// built by the scan at stage-in -- so there is nothing of it an edit between two launches could leave stale.
//
// The tape comes from a caller and is never trusted: an op that would index outside a table, or that the reference would refuse
// with an assertion, is skipped or repaired, and the env's sticky ST_BAD_EDIT says so (include/crafter_hip_edit.h lists the
// cases).  An edit draws nothing: the stream's state is staged with the rest and not stored.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/crafter_hip_edit.h"
#include "env_kernels.hpp"
#include "env_worlds.hpp"

namespace crafter {

constexpr uint32_t ST_BAD_EDIT = CRAFTER_ST_BAD_EDIT;   // (the header keeps it beside crafter_edit_envs)
constexpr int kEditWords = CRAFTER_EDIT_WORDS;
constexpr int kEditThreads = 256;   // the edit workgroup: wave 0 replays, the others help the stage-in and the write-back

// an inclusive range test in one unsigned compare (lo <= hi; the words of a tape are any int32: the differences wrap, unsigned)
__host__ __device__ inline bool edit_within(int v, int lo, int hi) { return (uint32_t)v - (uint32_t)lo <= (uint32_t)hi - (uint32_t)lo; }

// The ops of one env, in order.  Wave 0 only; ends with the wave-uniform registers (nobj) current in wave 0.
// next_step: the env's entry of the dispatch order's hint (step_body.hpp StepCtl::next_step) or null -- a clock edit refreshes it.
template <class W, class S>
__device__ __forceinline__ void replay_edits(Env<W, S>& e, const int32_t* ops, int nops, int32_t* next_step) {
  W& w = e.w;
  const Config& c = e.cfg;
  const Rules& R = e.R;
  EnvRec* rec = e.rec;
  uint32_t flags = 0;
  // the record of a slot's first two words (type, health, facing | position): every lane reads what the leader lane wrote
  auto head = [&](int slot, uint32_t& w0, uint32_t& w1) {
    const uint32_t* rw = (const uint32_t*)&e.objs[slot];
    w0 = (uint32_t)W::uni((int)rw[0]);
    w1 = (uint32_t)W::uni((int)rw[1]);
  };
  auto set_facing = [&](int slot, int fx, int fy) {
    if (w.leader()) {
      e.objs[slot].fx = (int8_t)fx;
      e.objs[slot].fy = (int8_t)fy;
    }
    w.wsync();
  };
  // 64 ops at a time come into lane registers, two 16-byte loads per lane; each is then read out of its lane (no memory round
  // trip per op), as author_world reads its records
  for (int base = 0; base < nops; base += 64) {
    w.template lane_set4<4>(base, nops, [&](int i, int) -> vec16 { return ((const vec16*)ops)[2 * i]; });
    w.template lane_set4<8>(base, nops, [&](int i, int) -> vec16 { return ((const vec16*)ops)[2 * i + 1]; });
    const int m = nops - base < 64 ? nops - base : 64;
    for (int l = 0; l < m; l++) {
      const int kind = (int)w.lane_read(4, l);
      if (kind == CRAFTER_EDIT_NOP) continue;
      const int a1 = (int)w.lane_read(5, l), a2 = (int)w.lane_read(6, l), a3 = (int)w.lane_read(7, l), a4 = (int)w.lane_read(8, l);
      const int a5 = (int)w.lane_read(9, l), a6 = (int)w.lane_read(10, l), a7 = (int)w.lane_read(11, l);
      if (kind == CRAFTER_EDIT_SET_CELL) {   // x y material
        if (!e.inside(a1, a2) || !edit_within(a3, 1, R.n_materials)) {
          flags |= ST_BAD_EDIT;
          continue;
        }
        e.set_mat(a1, a2, a3);
      } else if (kind == CRAFTER_EDIT_ADD) {   // type x y health fx fy aux
        int fx = a5, fy = a6;
        if (a1 < T_COW || a1 > T_PLANT || !e.inside(a2, a3) || W::uni(e.slot_at(a2, a3)) != 0) {
          flags |= ST_BAD_EDIT;
          continue;
        }
        if (a1 != T_ARROW) {   // the other classes keep no facing: (0, 0), as World.add's callers write it
          fx = fy = 0;
        } else if (!unit_axis(fx, fy)) {
          flags |= ST_BAD_EDIT;
          fx = 0;
          fy = 1;
        }
        if (e.nobj >= c.max_objects) {   // a hole -- this tape's REMOVE, or one the lazy compaction of a large world's step kernel left
          e.dirty_slots = 1;             // across launches -- is a free slot: squeeze the table before it is called full
          e.compact();
        }
        e.obj_add(a1, a2, a3, a4, fx, fy, a7);   // (a full table: ST_OBJ_OVERFLOW, set there)
      } else if (kind == CRAFTER_EDIT_REMOVE) {   // x y
        const int slot = e.inside(a1, a2) ? W::uni(e.slot_at(a1, a2)) : 0;
        if (slot <= 1) {   // outside, nobody there, or the player
          flags |= ST_BAD_EDIT;
          continue;
        }
        e.obj_remove(slot);
      } else if (kind == CRAFTER_EDIT_MOVE) {   // x y x2 y2
        const int slot = e.inside(a1, a2) ? W::uni(e.slot_at(a1, a2)) : 0;
        if (slot == 0 || !e.inside(a3, a4)) {
          flags |= ST_BAD_EDIT;
          continue;
        }
        if (a3 == a1 && a4 == a2) continue;
        if (W::uni(e.slot_at(a3, a4)) != 0) {
          flags |= ST_BAD_EDIT;
          continue;
        }
        uint32_t w0, w1;
        head(slot, w0, w1);
        e.obj_move(slot, a1, a2, a3, a4, true, Env<W, S>::creature_col((int)(w0 & 0xFFu)));
      } else if (kind == CRAFTER_EDIT_SET_OBJECT) {   // x y which health fx fy aux
        const int slot = e.inside(a1, a2) ? W::uni(e.slot_at(a1, a2)) : 0;
        if (slot == 0) {
          flags |= ST_BAD_EDIT;
          continue;
        }
        uint32_t w0, w1;
        head(slot, w0, w1);
        const int type = (int)(w0 & 0xFFu);
        int which = a3;
        if (which & ~(CRAFTER_EDIT_HEALTH | CRAFTER_EDIT_FACING | CRAFTER_EDIT_AUX)) {
          flags |= ST_BAD_EDIT;
          which &= CRAFTER_EDIT_HEALTH | CRAFTER_EDIT_FACING | CRAFTER_EDIT_AUX;
        }
        if (type == T_PLAYER && (which & (CRAFTER_EDIT_HEALTH | CRAFTER_EDIT_AUX))) {   // its health is an item, it has no counter
          flags |= ST_BAD_EDIT;
          which &= CRAFTER_EDIT_FACING;
        }
        if (which & CRAFTER_EDIT_HEALTH) {
          e.set_health(slot, a4);
          w.wsync();
        }
        if ((which & CRAFTER_EDIT_FACING) && (type == T_PLAYER || type == T_ARROW)) {
          if (unit_axis(a5, a6))
            set_facing(slot, a5, a6);
          else
            flags |= ST_BAD_EDIT;
        }
        if (which & CRAFTER_EDIT_AUX) {
          e.set_aux(slot, a7);
          w.wsync();
        }
      } else if (kind == CRAFTER_EDIT_SET_ITEM) {   // item value
        if (!edit_within(a1, 0, R.n_items - 1)) {
          flags |= ST_BAD_EDIT;
          continue;
        }
        const int most = R.item_max[a1];
        int v = a2;
        if (!edit_within(v, 0, most)) {
          flags |= ST_BAD_EDIT;
          v = v < 0 ? 0 : most;
        }
        e.st(&rec->inv[a1], v);
        w.wsync();
      } else if (kind == CRAFTER_EDIT_SET_PLAYER) {   // field value
        // what the rules can leave in the counters (objects.py:133-167, in half steps)
        const int lo = a1 == CRAFTER_EDIT_FATIGUE2 ? -20 : a1 == CRAFTER_EDIT_RECOVER2 ? -30 : 0;
        const int hi = a1 == CRAFTER_EDIT_SLEEPING ? 1 : a1 == CRAFTER_EDIT_HUNGER2 ? 50 : a1 == CRAFTER_EDIT_THIRST2 ? 40
                     : a1 == CRAFTER_EDIT_FATIGUE2 ? 60 : 50;
        if (!edit_within(a1, 0, CRAFTER_EDIT_FIELDS - 1) || !edit_within(a2, lo, hi)) {
          flags |= ST_BAD_EDIT;
          continue;
        }
        int32_t* field = a1 == CRAFTER_EDIT_SLEEPING ? &rec->sleeping : a1 == CRAFTER_EDIT_HUNGER2 ? &rec->hunger2
                       : a1 == CRAFTER_EDIT_THIRST2 ? &rec->thirst2 : a1 == CRAFTER_EDIT_FATIGUE2 ? &rec->fatigue2 : &rec->recover2;
        e.st(field, a2);
        w.wsync();
      } else if (kind == CRAFTER_EDIT_SET_CLOCK) {   // step
        if (a1 < 0 || a1 >= c.n_daylight || (c.length > 0 && a1 >= c.length)) {
          flags |= ST_BAD_EDIT;
          continue;
        }
        e.st(&rec->step, a1);
        if (next_step && w.leader()) *next_step = a1 + 1;   // (the number of the step the env runs next, as a step leaves it)
        w.wsync();
      } else {
        flags |= ST_BAD_EDIT;
      }
    }
  }
  if (flags) {
    e.st(&rec->status, rec->status | flags);
    w.wsync();
  }
}

// crafter_edit_envs for one env.  ops: the env's tape, nops ops of kEditWords words, 16-byte aligned.
template <class W>
__device__ __forceinline__ void edit_body(W& w, uint8_t* smem, int env, const Config& cfg, const TablePtrs& tb, const StatePtrs& st,
                                          const int32_t* ops, int nops, int32_t* next_step) {
  typedef uint16_t S;
  const LdsLayout L = edit_layout(cfg);
  w.scratch = (uint32_t*)(smem + L.scratch);
  Env<W, S> e(w, cfg, tb, smem + L.rules);
  bind_lds<W, -1, S>(e, smem, L, st, env);
  load_env(e, st, env, 1);
  if (w.wave0()) {
    replay_edits(e, ops, nops, next_step ? next_step + env : nullptr);
    e.compact();
  }
  share_registers(e);
  // (the stream's state was staged and nothing rewrote it: it does not go back; a large world's slot table was edited in place)
  store_env(e, st, env, L.objs >= 0, true);
}

}  // namespace crafter
