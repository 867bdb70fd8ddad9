// Level sets (crafter_set_levels) supersede what DESIGN.md 9.0 assumed about a device-side level sampler inside the auto-reset:
// it needs NO pool keyed by (lane, episode).  A generated world is seeded by WorldGen::seed_world alone (worldgen.hpp), which
// both forms of the generator hand level_seed(table, lane, k) below: with a table the level of the env's k-th reset is a pure
// function of (the env's own seed lane, k, the table), so the pool keeps keying its entries by k, the inline and the pooled path
// agree by construction, and entries only have to be emptied when the table itself is replaced (set_levels_body).
//
// Choosing levels (crafter_reseed): an env's world is a pure function of (seed lane, episode) -- env.py:74, mt19937.hpp
// world_seed -- and both live in its record, read by the generators when the env next resets.  Reseeding is therefore an edit
// of the record, plus what keeps the world pool honest: the pool runs two worlds ahead of every env and keys its entries by
// EPISODE ALONE, so after the edit
//   * an entry still holding a world of the old lane under an episode number the env will ask for again would be adopted
//     (pool_ready) or taken for generated (gen_done_already): both entries are emptied -- ready = 0, pending = 0;
//   * gen_latest above the new episode would make gen_wanted refuse every request of the env for good (it would regenerate
//     inline at each episode end, correctly, and never see the pool again): gen_latest = the new rec.episode.
// The host brings the pool to rest before this runs (crafter_reseed: as before crafter_load_envs), so no batch in flight delivers
// a world of the old lane into an emptied entry afterwards and no queued request keeps `pending` set.
// The episode in progress is not touched: it plays on, only its number reads episode - 1 from here on.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "mt19937.hpp"
#include "types.hpp"

namespace crafter {

// ---------------------------------------------------------------------------------------------
// The level table of a handle: one device buffer of fixed capacity, written by set_levels_body in stream order and read by the
// generators.  n == 0: no table.  It stays in global memory (one dependent load at the head of a generation).
constexpr int kMaxLevels = 65536;
struct LevelTable {
  uint64_t key;
  int32_t n;          // 0 .. kMaxLevels
  int32_t weighted;   // cum[] is in force
  uint64_t lane[kMaxLevels];
  int32_t episode[kMaxLevels];   // >= 1
  uint32_t cum[kMaxLevels];      // non-decreasing; cum[n - 1] counts as 2^32 whatever it holds
};

// splitmix64's finaliser and its golden-ratio increment: what `pick` below and the state fingerprints (fingerprint.hpp) mix
// with; crafter_amd.state.mix64 is the numpy mirror.
constexpr uint64_t kGolden64 = 0x9E3779B97F4A7C15ull;
__host__ __device__ constexpr uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// pick(lane, k): the table entry of the reset that takes an env of draw lane `lane` into its k-th episode.  Counter based
// (mix64 over lane + golden * k + key); crafter_amd.levels_pick is its numpy mirror.  t->n >= 1.
__device__ __forceinline__ int level_pick(const LevelTable* t, uint64_t lane, int k) {
  const uint64_t u = mix64(lane + kGolden64 * (uint64_t)k + t->key) >> 32;
  const int n = t->n;
  if (!t->weighted) return (int)((u * (uint64_t)n) >> 32);
  int lo = 0, hi = n - 1;   // first j with cum[j] > u; the last entry takes what is left (at most 16 rounds)
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if ((uint64_t)t->cum[mid] > u)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

// The world seed of (lane, k): env.py:74 on the picked entry, or on (lane, k) itself without a table.
__device__ __forceinline__ uint32_t level_seed(const LevelTable* t, uint64_t lane, int k) {
  if (!t || t->n <= 0) return world_seed(lane, (uint64_t)k);
  const int j = level_pick(t, lane, k);
  return world_seed(t->lane[j], (uint64_t)t->episode[j]);
}

constexpr int kLevelThreads = 256;   // crafter_set_levels / crafter_level_ids: one thread per table entry / env

// crafter_set_levels, thread i of max(n, num_envs, 1): copies table entry i (an episode below 1 is taken as 1; cum null: uniform),
// thread 0 writes the head, and -- where pool words are bound -- empties BOTH pool entries of env i and sets gen_latest[i] =
// rec.episode: what reseed_body does for a named env, without editing the record.  Every pooled world was generated under the
// table that is being replaced; the host has brought the pool to rest (as before crafter_reseed).
template <class W>
__device__ __forceinline__ void set_levels_body(int i, const Config& cfg, const StatePtrs& st, LevelTable* t, const uint64_t* seed_lane,
                                                const int32_t* episode, const uint32_t* cum, int n, uint64_t key) {
  if (i == 0) {
    t->key = key;
    t->n = n;
    t->weighted = (cum && n > 0) ? 1 : 0;
  }
  if (i < n) {
    int ep = episode[i];
    t->lane[i] = seed_lane[i];
    t->episode[i] = ep < 1 ? 1 : ep;
    if (cum) t->cum[i] = cum[i];
  }
  if (i < cfg.num_envs) {
    if (st.pool_hdr)
      for (int e = 0; e < 2; e++) {
        PoolHdr* h = st.pool_hdr + (size_t)e * cfg.num_envs + i;
        W::agent_store(&h->ready, (uint64_t)0);
        W::agent_store(&h->pending, (int32_t)0);
      }
    if (st.gen_latest) W::agent_store(st.gen_latest + i, (int32_t)st.rec[i].episode);
  }
}

// crafter_level_ids: ids[env] = pick(rec.seed_lane, rec.episode) under the table in force -- the level of the episode in
// progress IF that episode began while this table was set --, -1 without a table.  Read-only; rows with a zero mask byte untouched.
__device__ __forceinline__ void level_ids_body(int env, const Config& cfg, const StatePtrs& st, const LevelTable* t, const uint8_t* mask,
                                               int32_t* ids) {
  if (env >= cfg.num_envs) return;
  if (mask && !mask[env]) return;
  ids[env] = (t && t->n > 0) ? level_pick(t, st.rec[env].seed_lane, st.rec[env].episode) : -1;
}

// ---------------------------------------------------------------------------------------------
// crafter_reseed

constexpr int kReseedThreads = 256;   // one thread per env

// mask: uint8 [N] or null (all); seed_lane: uint64 [N]; episode: int32 [N] or null (1).  The env's next reset starts episode
// max(episode[env], 1) of that lane.  Rows with a zero mask byte: nothing read, nothing written.  Pool words only where bound.
template <class W>
__device__ __forceinline__ void reseed_body(int env, const Config& cfg, const StatePtrs& st, const uint8_t* mask,
                                            const uint64_t* seed_lane, const int32_t* episode) {
  if (env >= cfg.num_envs) return;
  if (mask && !mask[env]) return;
  int ep = episode ? episode[env] : 1;
  if (ep < 1) ep = 1;
  EnvRec* rec = st.rec + env;
  rec->seed_lane = seed_lane[env];
  rec->episode = ep - 1;   // Env.reset increments first (env.py:71)
  if (st.pool_hdr)
    for (int e = 0; e < 2; e++) {
      PoolHdr* h = st.pool_hdr + (size_t)e * cfg.num_envs + env;
      W::agent_store(&h->ready, (uint64_t)0);
      W::agent_store(&h->pending, (int32_t)0);
    }
  if (st.gen_latest) W::agent_store(st.gen_latest + env, (int32_t)(ep - 1));
}

}  // namespace crafter
