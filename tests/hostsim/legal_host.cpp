// TEST INFRASTRUCTURE -- crafter_legal_actions' body (csrc/legal.hpp) on the CPU through WaveHost (see wave_host.hpp).
#include <string.h>

#include "wave_host.hpp"
#include "../../crafter_amd/csrc/launch_plan.hpp"   // LaunchPlan::maps_in_lds: the chooser between the two object paths, as the library's
#include "../../crafter_amd/csrc/legal.hpp"

using namespace crafter;

extern "C" {

int hostsim_legal_map_is_state(const Config* cfg) { return launch_plan(*cfg, false).maps_in_lds ? 0 : 1; }

// cfg / tb / st: a HostSimEnv's.  legal: [N][n_actions] bytes.
int hostsim_legal(const Config* cfg, const TablePtrs* tb, const StatePtrs* st, const uint8_t* mask, uint8_t* legal) {
  const bool map_is_state = !launch_plan(*cfg, false).maps_in_lds;
  // one env beyond the batch, as the last workgroup's spare waves: must return without touching anything
  for (int env = 0; env < cfg->num_envs + 1; env++) {
    WaveHost w;
    if (map_is_state)
      legal_body<WaveHost, 1>(w, env, *cfg, *tb, *st, mask, legal);
    else
      legal_body<WaveHost, 0>(w, env, *cfg, *tb, *st, mask, legal);
  }
  return 0;
}

}  // extern "C"
