// State fingerprints (crafter_fingerprint): one 64-bit key per env that says whether two rows are in the same state, hashed from
// exactly what the canonical snapshot (BatchedEnv.snapshot / OracleEnv.snapshot) holds -- never from the raw bytes: free records
// behind nobj keep what was last stored there, step and rollout leave different tails, the large-world instance keeps T_NONE
// holes inside the prefix, and objmap / census / chunk_seen / Obj.pad / the player's Obj.health byte / status / the last-output
// and ep_* fields / env_last_health / unlocked are derived, scratch or bookkeeping.  NOT cryptographic: a mixing hash for
// transposition tables, archives and duplicate checks; anyone who chooses the state can choose a collision.
//
//   mix64      env_levels.hpp (splitmix64's finaliser), G = kGolden64, all arithmetic mod 2^64
//   S_p        = mix64(p + 1), the salt of part p
//   H_p        = mix64(S_p + n + sum_i mix64((u_i ^ S_p) + (i + 1) * G))   over the part's n 64-bit units u_0 .. u_{n-1}
//   K(parts)   = mix64(parts * G + sum_{p in parts} H_p)
// The sum is commutative on purpose: lanes reduce it in any order and get the same bits; the position term keeps the hash
// order-sensitive.  The parts (bit p of `parts` is CRAFTER_FP_*, crafter_hip_types.h) and their units:
//   0 MAP      the env's mat row, 8 bytes per unit, little-endian, the last unit zero-padded: n = ceil(W H / 8)
//   1 OBJECTS  the live objects -- slots 1 .. min(nobj, max_objects) - 1 with type != T_NONE -- in slot order; the object of
//              rank k among them gives unit 2k = type | (health & 0xFF) << 8 | (fx & 0xFF) << 16 | (fy & 0xFF) << 24 | x << 32 |
//              y << 48 (the record's first eight bytes; a PLAYER record's health is inv[item_health], state.live_objects) and
//              unit 2k + 1 = (uint32)aux.  Rank, not slot number: holes do not count
//   2 PLAYER   one unit per value, (uint32) zero-extended: inv[0 .. n_items), ach[0 .. n_achievements), sleeping != 0, hunger2,
//              thirst2, fatigue2, recover2, player_last_health
//   3 CLOCK    (uint32)step
//   4 RNG      mt[2i] | mt[2i + 1] << 32 for i < 312, then (uint32)mt_pos
//   5 CHUNKS   chunk_order[0 .. min(nchunks_seen, nch)), one unit each
//   6 IDENT    seed_lane, then (uint32)episode
//
// One wave per env, four envs per workgroup, no LDS and no barrier: a masked row or the batch tail returns at once.  Read-only: no
// RNG draw, nothing of the world pool is looked at.  A pure read of the mat row, the live prefix of objs, mt, rec and the chunk
// order (8.6 KB per env at the default geometry): 16-byte loads wherever the row's base and stride allow -- mt (2496 bytes a row)
// and objs always, mat when W H is a multiple of 16; any other area takes the byte path --, the loads of a round all issued
// before its first mix64, object ranks by ballot + count_below with a running base per 64 slots, one 64-bit accumulator per part
// per lane, and one reduction per part at the end (W::sum64).  The same body serves worlds whose maps stay in global memory (64 KB
// of mat, 2048 slots): one wave walks the row in rounds of 4 KB.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "env_levels.hpp"
#include "types.hpp"

namespace crafter {

constexpr int kFingerprintThreads = 256;   // four envs per workgroup
constexpr int kFingerprintEnvs = kFingerprintThreads / 64;
constexpr int kFpParts = CRAFTER_FP_PARTS;
constexpr uint32_t kFpAll = CRAFTER_FP_ALL;
constexpr int kFpRound = 4;   // loads a lane has in flight per round

struct FpPair {
  uint64_t lo, hi;
};
// 16 bytes at a 16-byte aligned address: one global_load_dwordx4
__device__ __forceinline__ FpPair fp_load_pair(const void* p) {
  FpPair v;
  __builtin_memcpy(&v, __builtin_assume_aligned(p, 16), 16);
  return v;
}

__host__ __device__ constexpr uint64_t fp_salt(int p) { return mix64((uint64_t)p + 1); }
// unit u at position i of a part whose salt is s
__host__ __device__ constexpr uint64_t fp_term(uint64_t s, uint64_t u, uint64_t i) { return mix64((u ^ s) + (i + 1) * kGolden64); }
__host__ __device__ constexpr uint64_t fp_close(int p, uint64_t n, uint64_t sum) { return mix64(fp_salt(p) + n + sum); }

// The units of the records W::lane_gather4 left in registers 4g .. 4g + 3 (slots base + 64 g + lane, g < kFpRound): a live record's
// rank is `live` + the live ones below it in its group of 64
template <class W, int G>
__device__ __forceinline__ void fp_objs_mix(W& w, int base, int n, uint32_t health, int& live, uint64_t& acc) {
  if constexpr (G < kFpRound) {
    uint64_t m = W::uni64(w.lane_ballot(4 * G, 0xFFu));   // type != T_NONE
    if (base + 64 * G == 0) m &= ~1ull;                     // (slot 0 is reserved, whatever it holds)
    w.lanes(base + 64 * G, n, [&](int, int l) {
      if (!((m >> l) & 1ull)) return;
      const uint64_t k = (uint64_t)w.count_below(m, l, live);
      uint32_t w0 = w.lane_get(4 * G, l);
      if ((w0 & 0xFFu) == T_PLAYER) w0 = (w0 & ~0xFF00u) | ((health & 0xFFu) << 8);
      acc += fp_term(fp_salt(1), w0 | ((uint64_t)w.lane_get(4 * G + 1, l) << 32), 2 * k) +
             fp_term(fp_salt(1), (uint64_t)w.lane_get(4 * G + 2, l), 2 * k + 1);
    });
    live += __builtin_popcountll(m);
    fp_objs_mix<W, G + 1>(w, base, n, health, live, acc);
  }
}

// key: [N] or null; part_hash: [N][kFpParts] or null (then only the parts of `parts` are read).
template <class W>
__device__ __forceinline__ void fingerprint_body(W& w, int env, const Config& cfg, const TablePtrs& tb, const StatePtrs& st,
                                                 const uint8_t* mask, uint32_t parts, uint64_t* key, uint64_t* part_hash) {
  if (env >= cfg.num_envs) return;
  if (mask && !mask[env]) return;
  const Rules& R = *tb.rules;
  const EnvRec* rec = st.rec + env;
  const uint32_t want = part_hash ? kFpAll : parts;
  uint64_t sum[kFpParts] = {0, 0, 0, 0, 0, 0, 0}, count[kFpParts] = {0, 0, 0, 0, 0, 0, 0};

  if (want & CRAFTER_FP_MAP) {
    const int cells = cfg.W * cfg.H;
    const uint8_t* mat = st.mat + (size_t)env * cells;
    const uint64_t s = fp_salt(0);
    uint64_t acc = 0;
    count[0] = (uint64_t)((cells + 7) / 8);
    if (cells % 16 == 0) {   // two units per 16-byte load
      const int nv = cells / 16;
      for (int base = 0; base < nv; base += 64 * kFpRound) {
        w.lanes(base, nv, [&](int i, int) {
          FpPair v[kFpRound];
#pragma unroll
          for (int k = 0; k < kFpRound; k++) {   // (unpredicated, clamped: all in flight together)
            const int j = i + 64 * k;
            v[k] = fp_load_pair(mat + 16 * (size_t)(j < nv ? j : nv - 1));
          }
#pragma unroll
          for (int k = 0; k < kFpRound; k++) {
            const int j = i + 64 * k;
            if (j < nv) acc += fp_term(s, v[k].lo, 2 * (uint64_t)j) + fp_term(s, v[k].hi, 2 * (uint64_t)j + 1);
          }
        });
      }
    } else {   // a row that starts at any byte: a unit from its (up to) eight bytes
      const int nu = (cells + 7) / 8;
      for (int base = 0; base < nu; base += 64) {
        w.lanes(base, nu, [&](int i, int) {
          uint8_t byte[8];
#pragma unroll
          for (int b = 0; b < 8; b++) byte[b] = mat[8 * i + b < cells ? 8 * i + b : cells - 1];   // (unpredicated, clamped: all in flight together)
          uint64_t u = 0;
#pragma unroll
          for (int b = 0; b < 8; b++) u |= 8 * i + b < cells ? (uint64_t)byte[b] << (8 * b) : 0ull;
          acc += fp_term(s, u, (uint64_t)i);
        });
      }
    }
    sum[0] = W::sum64(acc);
  }

  if (want & CRAFTER_FP_OBJECTS) {
    const Obj* objs = st.objs + (size_t)env * cfg.max_objects;
    int n = W::uni(rec->nobj);
    if (n > cfg.max_objects) n = cfg.max_objects;
    const uint32_t health = (uint32_t)rec->inv[R.item_health];
    int live = 0;
    uint64_t acc = 0;
    for (int base = 0; base < n; base += 64 * kFpRound) {
      w.template lane_gather4<0, kFpRound>(base, n, objs);
      fp_objs_mix<W, 0>(w, base, n, health, live, acc);
    }
    count[1] = 2 * (uint64_t)live;
    sum[1] = W::sum64(acc);
  }

  if (want & CRAFTER_FP_PLAYER) {
    const int ni = R.n_items < MAX_ITEMS ? R.n_items : MAX_ITEMS, na = R.n_achievements < MAX_ACH ? R.n_achievements : MAX_ACH;
    const int n = ni + na + 6;   // <= 54: one lane each
    uint64_t acc = 0;
    w.lanes(0, n, [&](int i, int) {
      int32_t v;
      if (i < ni) v = rec->inv[i];
      else if (i < ni + na) v = rec->ach[i - ni];
      else if (i == ni + na) v = rec->sleeping != 0;
      else v = (&rec->hunger2)[i - ni - na - 1];   // hunger2, thirst2, fatigue2, recover2, player_last_health
      acc += fp_term(fp_salt(2), (uint64_t)(uint32_t)v, (uint64_t)i);
    });
    count[2] = (uint64_t)n;
    sum[2] = W::sum64(acc);
  }

  if (want & CRAFTER_FP_RNG) {
    const uint32_t* mt = st.mt + (size_t)env * MT_N;
    constexpr int nv = MT_N / 4, rounds = (nv + 63) / 64;   // 156 loads of 16 bytes: three a lane
    const uint64_t s = fp_salt(4);
    uint64_t acc = 0;
    w.lanes(0, 64, [&](int i, int) {
      FpPair v[rounds];
#pragma unroll
      for (int k = 0; k < rounds; k++) {
        const int j = i + 64 * k;
        v[k] = fp_load_pair(mt + 4 * (j < nv ? j : nv - 1));
      }
#pragma unroll
      for (int k = 0; k < rounds; k++) {
        const int j = i + 64 * k;
        if (j < nv) acc += fp_term(s, v[k].lo, 2 * (uint64_t)j) + fp_term(s, v[k].hi, 2 * (uint64_t)j + 1);
      }
      if (i == 0) acc += fp_term(s, (uint64_t)(uint32_t)rec->mt_pos, (uint64_t)(MT_N / 2));
    });
    count[4] = MT_N / 2 + 1;
    sum[4] = W::sum64(acc);
  }

  if (want & CRAFTER_FP_CHUNKS) {
    const int nch = cfg.nchunk_x * cfg.nchunk_y;
    const uint16_t* order = st.chunk_order + (size_t)env * nch;
    int n = W::uni(rec->nchunks_seen);
    n = n < 0 ? 0 : n > nch ? nch : n;
    uint64_t acc = 0;
    for (int base = 0; base < n; base += 64)
      w.lanes(base, n, [&](int i, int) { acc += fp_term(fp_salt(5), (uint64_t)order[i], (uint64_t)i); });
    count[5] = (uint64_t)n;
    sum[5] = W::sum64(acc);
  }

  // the two parts of one and two record fields, the closing mix and the stores: one lane
  w.lanes(0, 1, [&](int, int) {
    sum[3] = fp_term(fp_salt(3), (uint64_t)(uint32_t)rec->step, 0);
    count[3] = 1;
    sum[6] = fp_term(fp_salt(6), rec->seed_lane, 0) + fp_term(fp_salt(6), (uint64_t)(uint32_t)rec->episode, 1);
    count[6] = 2;
    uint64_t total = 0;
#pragma unroll
    for (int p = 0; p < kFpParts; p++) {
      if (!((want >> p) & 1u)) continue;
      const uint64_t h = fp_close(p, count[p], sum[p]);
      if (part_hash) part_hash[(size_t)env * kFpParts + p] = h;
      if ((parts >> p) & 1u) total += h;
    }
    if (key) key[env] = mix64((uint64_t)parts * kGolden64 + total);
  });
}

}  // namespace crafter
