// TEST INFRASTRUCTURE -- crafter_nearby's body (csrc/nearby.hpp) on the CPU through WaveHost (see wave_host.hpp).
#include <string.h>

#include <vector>

#include "wave_host.hpp"
#include "../../crafter_amd/csrc/launch_plan.hpp"   // LaunchPlan::maps_in_lds: the chooser between the two object paths, as the library's
#include "../../crafter_amd/csrc/nearby.hpp"

using namespace crafter;

// WaveHost plus the primitive nearby.hpp takes from the wave policy beyond it (wave_gfx950.hpp lds_min).
struct NearWaveHost : WaveHost {
  void lds_min(uint32_t* p, uint32_t v) const {
    if (v < *p) *p = v;
  }
};

extern "C" {

int hostsim_nearby_map_is_state(const Config* cfg) { return launch_plan(*cfg, false).maps_in_lds ? 0 : 1; }
int hostsim_nearby_in_wave(const Config* cfg) { return near_in_wave(*cfg) ? 1 : 0; }
int hostsim_nearby_lds_bytes(const Config* cfg, int k) { return (int)(near_lds_words(*cfg, k) * 4); }

// cfg / tb / st: a HostSimEnv's.  counts: [N][1 + n_materials + 6]; ents: [N][k][6] and n: [N], or null with k == 0.  force_map: -1
// the instance the library would take with the walk it would choose, 0 / 1 the instance that reads the slot table only / the one
// that may read objmap; walk: NearQuery::walk (-1 whichever is shorter, 0 the slot table, 1 objmap over the window).
// -> 0, or what crafter_nearby refuses: the number of near_check's reason.
int hostsim_nearby(const Config* cfg, const TablePtrs* tb, const StatePtrs* st, const uint8_t* mask, int32_t distance, int32_t flags,
                   uint32_t classes, int32_t k, int32_t* counts, int16_t* ents, int32_t* n, int force_map, int walk) {
  if (const int why = near_check(*cfg, tb->rules->n_materials, distance, flags, classes, k, counts, ents, n)) return why;
  const NearQuery q = {distance, flags, classes, k, walk};
  const bool map_is_state = force_map < 0 ? !launch_plan(*cfg, false).maps_in_lds : force_map != 0;
  const size_t words = near_lds_words(*cfg, k);
  // the "LDS" in a buffer of exactly its size, filled with another pattern for every env: the body must clear what it reads.
  // One env beyond the batch, as a grid rounded up would bring: must return without touching anything
  for (int env = 0; env < cfg->num_envs + 1; env++) {
    std::vector<uint32_t> lds(words, 0xC3C3C3C3u + (uint32_t)env);
    NearWaveHost w;
    if (map_is_state) nearby_body<NearWaveHost, 1>(w, lds.data(), env, *cfg, *tb, *st, mask, q, counts, ents, n);
    else nearby_body<NearWaveHost, 0>(w, lds.data(), env, *cfg, *tb, *st, mask, q, counts, ents, n);
  }
  return 0;
}

const char* hostsim_nearby_error(int reason) { return near_error_text(reason); }

}  // extern "C"
