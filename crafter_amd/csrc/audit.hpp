// The audit of env rows (crafter_audit): every derived table of a row -- objmap where it is state, the five census columns per
// chunk, chunk_order / chunk_seen / nchunks_seen -- recounted from the primary state (mat, objs, rec), and per env the set of
// invariants that fail with the lowest offending place of the lowest failing one.  The invariants, their bits and what `detail`
// holds for each are include/crafter_hip_audit.h's; crafter_amd.audit_host is the numpy mirror, integer for integer.
//
// The one kernel whose input is untrusted by definition: NOTHING read from a row is used as an index before it has been bounded.
// rec.nobj and rec.nchunks_seen are clamped to their ranges (and REC is flagged), a record's x / y / type are compared with W / H /
// T_PLANT before they address the board, the counters or objmap, a chunk id is compared with nch before it addresses the position
// table, a material byte is only ever compared.  cfg and the rules are the handle's own and trusted.  Read-only: the two outputs
// are the only stores to global memory, no global atomics, no RNG draw, nothing of the world pool is looked at.
//
// One workgroup per env, its tables in LDS (audit_lds_words):
//   head   16 words: the lowest offending index per bit (kAuditNone: the check holds), the lowest unlisted chunk whose flag is set,
//          the non-zero objmap cells, the live records, two words of the detail phase
//   cnt    nch x 5 recounted census words
//   pos    nch words: a chunk id's first position in chunk_order (kAuditNone: not listed)
//   board  one bit per cell: a valid record stands on it
// Worlds of at most 64 x 64 cells and 256 slots take a workgroup of ONE wave (its barriers cost nothing, a masked row or a row
// never reset leaves at once, 1.4 KB of LDS at the default geometry); any other world a workgroup of 256 threads (20 KB for 256 x
// 256 cells: 484 x 5 counters, 484 positions, an 8 KB board).  Five phases between barriers: clear | the chunk list into pos | the
// passes that only add to the tables -- list and flags, mat (16-byte loads where W H is a multiple of 16, a byte path for areas
// such as 42 x 30, kAuditRound loads of a thread in flight together, a group's grass / path cells counted in registers and added
// per chunk), the slot table (16-byte records, kAuditRound in flight), objmap's non-zero cells | census against cnt | the verdict.
// A row that fails anything pays a sixth, the detail of its lowest bit; a consistent row never enters it.
// "Lowest" everywhere (lds_min): the outputs do not depend on the order the lanes reduce in.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/crafter_hip_audit.h"
#include "types.hpp"

namespace crafter {

constexpr int kAuditBits = CRAFTER_AUDIT_BITS;
constexpr int kAuditThreads = 64;         // worlds of at most kAuditWaveCells cells and kAuditWaveSlots slots: one wave per env
constexpr int kAuditWideThreads = 256;    // any other world
constexpr int kAuditWaveCells = 64 * 64;
constexpr int kAuditWaveSlots = 256;
constexpr int kAuditRound = 4;            // 16-byte loads a thread has in flight per round
constexpr int kAuditHead = 16;
constexpr int kAuditMaxLds = 64 * 1024;
constexpr uint32_t kAuditNone = 0xFFFFFFFFu;
// head words behind the kAuditBits first-index words
constexpr int kAuditUnlisted = 11, kAuditNonzero = 12, kAuditLive = 13, kAuditCount = 14, kAuditSlot = 15;

__host__ __device__ inline bool audit_in_wave(const Config& c) { return c.W * c.H <= kAuditWaveCells && c.max_objects <= kAuditWaveSlots; }
__host__ __device__ inline size_t audit_lds_words(const Config& c) {
  const size_t nch = (size_t)c.nchunk_x * c.nchunk_y, cells = (size_t)c.W * c.H;
  return kAuditHead + 6 * nch + (cells + 31) / 32;
}

struct AuditQuad {
  uint32_t v[4];
};
// 16 bytes at a 16-byte aligned address: one global_load_dwordx4
__device__ __forceinline__ AuditQuad audit_load16(const void* p) {
  AuditQuad q;
  __builtin_memcpy(&q, __builtin_assume_aligned(p, 16), 16);
  return q;
}
__device__ __forceinline__ bool audit_valid(const Obj& o, int Wd, int H) { return o.type <= T_PLANT && (int)o.x < Wd && (int)o.y < H; }
__device__ __forceinline__ int audit_creature_col(int type) { return type == T_ZOMBIE ? 2 : type == T_SKELETON ? 3 : type == T_COW ? 4 : -1; }

// lds: audit_lds_words(cfg) words owned by this workgroup, which serves one env.  MAP 1: objmap is state (maps in global memory).
// flags: [N]; detail: [N][4].
template <class W, int MAP>
__device__ __forceinline__ void audit_body(W& w, uint32_t* lds, int env, const Config& cfg, const TablePtrs& tb, const StatePtrs& st,
                                           const uint8_t* mask, int32_t* flags, int32_t* detail) {
  if (env >= cfg.num_envs) return;
  if (mask && !mask[env]) return;   // (the whole workgroup: no barrier has been met)
  const Rules& R = *tb.rules;
  const EnvRec* rec = st.rec + env;
  int32_t* out = detail + 4 * (size_t)env;
  if (W::uni(rec->episode) == 0) {   // never reset: nothing else of the row means anything
    w.block_for(1, [&](int) {
      flags[env] = CRAFTER_AUDIT_NOT_RESET;
      out[0] = 0;
      out[1] = out[2] = out[3] = -1;
    });
    return;
  }
  constexpr int NT = W::kThreads;
  const int Wd = cfg.W, H = cfg.H, cells = Wd * H, ncy = cfg.nchunk_y, nch = cfg.nchunk_x * ncy, C = cfg.max_objects;
  const int nm = R.n_materials, grass = R.mat_grass, path = R.mat_path;
  const uint8_t* mat = st.mat + (size_t)env * cells;
  const uint16_t* objmap = MAP ? st.objmap + (size_t)env * cells : nullptr;
  const Obj* objs = st.objs + (size_t)env * C;
  const uint16_t* order = st.chunk_order + (size_t)env * nch;
  const uint8_t* seen = st.chunk_seen + (size_t)env * nch;
  const int32_t* census = st.census + (size_t)env * nch * 5;
  uint32_t* first = lds;
  int32_t* cnt = (int32_t*)(lds + kAuditHead);
  uint32_t* pos = lds + kAuditHead + 5 * nch;
  uint32_t* board = pos + nch;
  const int total = (int)audit_lds_words(cfg);
  W::assume_lds(lds);

  // REC: the counts every later phase indexes with, clamped to their ranges
  const int nobj = W::uni(rec->nobj), mt_pos = W::uni(rec->mt_pos), step = W::uni(rec->step), nseen = W::uni(rec->nchunks_seen);
  const int n = nobj < 1 ? 1 : nobj > C ? C : nobj, k = nseen < 0 ? 0 : nseen > nch ? nch : nseen;
  const int rec_bad = n != nobj ? 0 : (mt_pos < 0 || mt_pos > MT_N) ? 1 : (step < 0 || step >= cfg.n_daylight) ? 2 : k != nseen ? 3 : -1;

  w.block_for(total, [&](int i) { lds[i] = (i < kAuditNonzero || i == kAuditSlot || (i >= kAuditHead + 5 * nch && i < kAuditHead + 6 * nch)) ? kAuditNone : 0u; });
  w.sync();
  w.block_for(k, [&](int i) {
    const int id = order[i];
    if (id < nch) w.lds_min(pos + id, (uint32_t)i);
    else w.lds_min(first + 9, (uint32_t)i);
  });
  w.sync();

  // CHUNKS: a position that repeats an id; a listed chunk without its flag (at its position); a flag without a listing
  w.block_for(k, [&](int i) {
    const int id = order[i];
    if (id < nch && pos[id] != (uint32_t)i) w.lds_min(first + 9, (uint32_t)i);
  });
  w.block_for(nch, [&](int c) {
    const bool flag = seen[c] != 0;
    const uint32_t p = pos[c];
    if (p != kAuditNone && !flag) w.lds_min(first + 9, p);
    if (p == kAuditNone && flag) w.lds_min(first + kAuditUnlisted, (uint32_t)c);
  });

  // MATERIAL, and the recount of SPACE: `count` <= 16 cells from cell c0, their bytes in q
  auto group = [&](int c0, int count, const AuditQuad& q) {
    int x = c0 / H, y = c0 - x * H, chunk = -1, g = 0, p = 0;
    auto flush = [&]() {
      if (g) w.lds_add(cnt + chunk * 5, g);
      if (p) w.lds_add(cnt + chunk * 5 + 1, p);
      g = p = 0;
    };
#pragma unroll
    for (int k = 0; k < 4; k++) {   // (unrolled over the words only: q stays in registers, the cell loop stays a loop)
      uint32_t word = q.v[k];
#pragma clang loop unroll(disable)
      for (int j = 4 * k; j < 4 * k + 4 && j < count; j++, word >>= 8) {
        const int m = (int)(word & 0xFFu);
        const int c = (int)((uint32_t)x / (uint32_t)CHUNK) * ncy + (int)((uint32_t)y / (uint32_t)CHUNK);
        if (c != chunk) {
          flush();
          chunk = c;
        }
        if (m < 1 || m > nm) w.lds_min(first + 6, (uint32_t)(c0 + j));
        else if (m == grass) g++;
        else if (m == path) p++;
        if (++y == H) y = 0, x++;
      }
    }
    flush();
  };
  if (cells % 16 == 0) {
    const int nv = cells / 16, rounds = (nv + NT * kAuditRound - 1) / (NT * kAuditRound);
    w.block_for(rounds * NT, [&](int i) {
      const int first_group = (i / NT) * NT * kAuditRound + i % NT;
      AuditQuad q[kAuditRound];
#pragma unroll
      for (int r = 0; r < kAuditRound; r++) {   // (unpredicated, clamped: all in flight together)
        const int j = first_group + NT * r;
        q[r] = audit_load16(mat + 16 * (size_t)(j < nv ? j : nv - 1));
      }
#pragma unroll
      for (int r = 0; r < kAuditRound; r++) {
        const int j = first_group + NT * r;
        if (j < nv) group(16 * j, 16, q[r]);
      }
    });
  } else {   // a row that starts at any byte: sixteen byte loads a group
    const int nu = (cells + 15) / 16;
    w.block_for(nu, [&](int i) {
      AuditQuad q = {{0u, 0u, 0u, 0u}};
#pragma unroll
      for (int j = 0; j < 16; j++)   // (unpredicated, clamped: all in flight together)
        q.v[j >> 2] |= (uint32_t)mat[16 * i + j < cells ? 16 * i + j : cells - 1] << (8 * (j & 3));
      group(16 * i, cells - 16 * i < 16 ? cells - 16 * i : 16, q);
    });
  }

  // the slot table: PLAYER, OBJECT, CELL, SLOTMAP's first clause, the recount of CREATURES, CHUNK_MISSING
  {
    int live = 0;
    const int rounds = (n + NT * kAuditRound - 1) / (NT * kAuditRound);
    w.block_for(rounds * NT, [&](int i) {
      const int first_slot = (i / NT) * NT * kAuditRound + i % NT;
      Obj o[kAuditRound];
#pragma unroll
      for (int r = 0; r < kAuditRound; r++) {
        const int s = first_slot + NT * r;
        o[r] = objs[s < n ? s : n - 1];
      }
#pragma unroll
      for (int r = 0; r < kAuditRound; r++) {
        const int s = first_slot + NT * r;
        if (s < 1 || s >= n || o[r].type == T_NONE) continue;
        live++;
        if ((o[r].type == T_PLAYER) != (s == 1)) w.lds_min(first + 2, (uint32_t)s);
        if (!audit_valid(o[r], Wd, H)) {
          w.lds_min(first + 3, (uint32_t)s);
          continue;
        }
        const int x = o[r].x, y = o[r].y, cell = x * H + y;
        const int chunk = (int)((uint32_t)x / (uint32_t)CHUNK) * ncy + (int)((uint32_t)y / (uint32_t)CHUNK);
        if (w.lds_fetch_or(board + (cell >> 5), 1u << (cell & 31)) & (1u << (cell & 31))) w.lds_min(first + 4, (uint32_t)cell);
        if (MAP && objmap[cell] != s) w.lds_min(first + 5, (uint32_t)cell);
        const int col = audit_creature_col(o[r].type);
        if (col >= 0) w.lds_add(cnt + chunk * 5 + col, 1);
        if (pos[chunk] == kAuditNone) w.lds_min(first + 10, (uint32_t)s);
      }
    });
    if (live) w.lds_add((int32_t*)first + kAuditLive, live);
    // slot 1 free, or behind nobj
    w.block_for(1, [&](int) {
      if (n < 2 || objs[1].type == T_NONE) w.lds_min(first + 2, 1u);
    });
  }

  // SLOTMAP's second clause: the non-zero cells of objmap
  if (MAP) {
    int nonzero = 0;
    if (cells % 8 == 0) {
      const int nv = cells / 8, rounds = (nv + NT * kAuditRound - 1) / (NT * kAuditRound);
      w.block_for(rounds * NT, [&](int i) {
        const int first_group = (i / NT) * NT * kAuditRound + i % NT;
        AuditQuad q[kAuditRound];
#pragma unroll
        for (int r = 0; r < kAuditRound; r++) {
          const int j = first_group + NT * r;
          q[r] = audit_load16(objmap + 8 * (size_t)(j < nv ? j : nv - 1));
        }
#pragma unroll
        for (int r = 0; r < kAuditRound; r++) {
          if (first_group + NT * r >= nv) continue;
#pragma unroll
          for (int j = 0; j < 4; j++) nonzero += ((q[r].v[j] & 0xFFFFu) != 0) + ((q[r].v[j] >> 16) != 0);
        }
      });
    } else {
      w.block_for(cells, [&](int i) { nonzero += objmap[i] != 0; });
    }
    if (nonzero) w.lds_add((int32_t*)first + kAuditNonzero, nonzero);
  }
  w.sync();

  // SPACE, CREATURES: the census against the recount
  w.block_for(nch * 5, [&](int i) {
    if (census[i] != cnt[i]) w.lds_min(first + (i % 5 < 2 ? 7 : 8), (uint32_t)i);
  });
  w.sync();

  uint32_t bits = rec_bad >= 0 ? (uint32_t)CRAFTER_AUDIT_REC : 0u;
  for (int b = 2; b < kAuditBits; b++)
    if (first[b] != kAuditNone) bits |= 1u << b;
  if (first[kAuditUnlisted] != kAuditNone) bits |= CRAFTER_AUDIT_CHUNKS;
  if (MAP && first[kAuditNonzero] != first[kAuditLive]) bits |= CRAFTER_AUDIT_SLOTMAP;
  bits = (uint32_t)W::uni((int)bits);
  if (!bits) {
    w.block_for(1, [&](int) {
      flags[env] = 0;
      out[0] = out[1] = out[2] = out[3] = -1;
    });
    return;
  }

  // the detail of the lowest failing bit.  Every index below is one a check above produced from bounded values.
  const int bit = __builtin_ctz(bits);
  const uint32_t at = (uint32_t)W::uni((int)first[bit]);
  w.sync();   // (every thread has read the head before the detail phase writes to it)
  if ((bit == 4 || bit == 5) && at != kAuditNone) {   // the records on the cell; the lowest of them objmap does not name
    first[kAuditCount] = 0u;   // (every thread stores the same two words)
    first[kAuditSlot] = kAuditNone;
    w.sync();
    w.block_for(n - 1, [&](int i) {
      const int s = i + 1;
      const Obj o = objs[s];
      if (o.type == T_NONE || !audit_valid(o, Wd, H) || (uint32_t)((int)o.x * H + (int)o.y) != at) return;
      w.lds_add((int32_t*)first + kAuditCount, 1);
      if (MAP && objmap[at] != s) w.lds_min(first + kAuditSlot, (uint32_t)s);
    });
    w.sync();
  }
  w.block_for(1, [&](int) {
    int32_t index = at == kAuditNone ? -1 : (int32_t)at, found = -1, expected = -1;
    switch (bit) {
      case 1:
        index = rec_bad;
        found = rec_bad == 0 ? nobj : rec_bad == 1 ? mt_pos : rec_bad == 2 ? step : nseen;
        expected = rec_bad == 0 ? n : rec_bad == 1 ? (mt_pos < 0 ? 0 : MT_N) : rec_bad == 2 ? (step < 0 ? 0 : cfg.n_daylight - 1) : k;
        break;
      case 2:
        found = (int)at < n ? objs[at].type : 0;
        expected = at == 1u ? T_PLAYER : -1;
        break;
      case 3: {
        const Obj o = objs[at];
        if (o.type > T_PLANT) found = o.type, expected = T_PLANT;
        else if ((int)o.x >= Wd) found = o.x, expected = Wd - 1;
        else found = o.y, expected = H - 1;
        break;
      }
      case 4:
        found = (int32_t)first[kAuditCount];
        expected = 1;
        break;
      case 5:
        if (at != kAuditNone) {
          found = MAP ? objmap[at] : 0;
          expected = (int32_t)first[kAuditSlot];
        } else {
          found = (int32_t)first[kAuditNonzero];
          expected = (int32_t)first[kAuditLive];
        }
        break;
      case 6:
        found = mat[at];
        break;
      case 7:
      case 8:
        found = census[at];
        expected = cnt[at];
        break;
      case 9:
        if (at != kAuditNone) {
          const int id = order[at];
          if (id >= nch || pos[id] != at) found = id;
          else found = 0, expected = 1;
        } else {
          found = (int32_t)first[kAuditUnlisted];
        }
        break;
      default: {   // 10
        const Obj o = objs[at];
        found = (int)((uint32_t)o.x / (uint32_t)CHUNK) * ncy + (int)((uint32_t)o.y / (uint32_t)CHUNK);
        break;
      }
    }
    flags[env] = (int32_t)bits;
    out[0] = bit;
    out[1] = index;
    out[2] = found;
    out[3] = expected;
  });
}

}  // namespace crafter
