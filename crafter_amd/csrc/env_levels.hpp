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

#include "types.hpp"

namespace crafter {

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
